"""Case table shared by tests/test_pool_refs.py (CPU) and tests/test_gpu_pool_resize_edges.py (GPU): the float64 definitions of the
pooling, resize, optimizer and conversion contracts of include/dmlnet_hip.h, the seeded input generators, the case tables and
the error bars derived from the arithmetic a kernel is allowed to do.  A plain module (no fixtures, no hooks, numpy only);
nothing here looks at a kernel's output or imports the library.  bf16_round / store / stored_bar / vec come from bn_cases.

eps32 = 2^-24 is float32's unit roundoff; a bfloat16 store adds half an ulp of the value's binade (bn_cases.stored_bar).

Two kinds of input, as in bn_cases.py:
  exact  small dyadic values and dyadic parameters (bilinear at x4, x2, x1, x1/2 and the two whole-image shrinks whose source
         coordinate is an integer or a half; SGD with lr = mu = 0.5, wd = 0.25, gscale in {2, 1, 0.25}; integer sums, with HW a
         power of two where 1 / HW comes in): every intermediate is a float32 value in any order and under contraction, so the
         kernel must EQUAL the float64 result -- its single rounding store(ref, "bf16") for a bfloat16 output;
  real   seeded Gaussians and the data that hurts (max pool: rounded ReLU data with > 40 % zeros, a constant image, windows
         of -inf, a NaN; reductions: a channel with |mean| / std = 1e4), against bars that count float32 roundings:
           a sum of n terms in any order            (n - 1) eps32 sum |x|, one more eps32 |result| per scaling;
           a bilinear weight                        the float32 source coordinate s = scale (d + 0.5) - 0.5 carries three roundings
                                                    (the quotient, the product, the difference): |ds| <= 3 eps32 (s + 0.5); a
                                                    weight is a hat function of s (slope 1, continuous across the index change)
                                                    and 1 - l1 is rounded once more: |dw| <= |ds| + eps32, for every source
                                                    index within 1 + |ds| of s;
           a bilinear value                         (Ey |Wx| + |Wy| Ex + Ey Ex) |v| + 5 eps32 |Wy| |Wx| |v|  (two products, two
                                                    sums per term, the fifth unit for the second order);
           its transpose                            the same with (n + 3) eps32, n the most destination pixels one source pixel
                                                    gathers (two products and n - 1 additions per term);
           SGD                                      v: 3 eps32 (|mu v| + |gscale g| + |wd p|);  p: lr bar_v + 3 eps32 (|p| + |lr v|).
No bar is measured on a kernel.  Nothing here had to be measured against a CPU float32 evaluation either: every bar above is
derived, and tests/test_pool_refs.py only checks that plain float32 evaluations (contracted and not) stay inside.
"""
import numpy as np

from bn_cases import EPS32, F32, F64, bf16_round, store, stored_bar, vec  # noqa: F401  (re-exported for the two test files)

# grid_for's cap times the 256 threads of a workgroup, per kernel (the "above the cap" cases must exceed these)
CAP_2048 = 2048 * 256                          # sgd (float4 items), fill, convert, broadcast_hw (vector items), adaptive finish
CAP_4096 = 4096 * 256                          # scalar bilinear_fwd / bilinear_bwd (four-channel items)
CAP_8192 = 8192 * 256                          # upsample_to_nchw (four-pixel items)
BIG_N = CAP_2048 + 300


def q(a, dtype):
    """float32 array a kernel input of `dtype` holds"""
    a = np.asarray(a, F64).astype(F32)
    return bf16_round(a) if dtype == "bf16" else a


def grid(rs, lo, hi, step, shape):
    return rs.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape).astype(F64) * step


def same(a, b):
    """elementwise equality with NaN equal to NaN"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------
# max pool 3x3 s2 p1
# ---------------------------------------------------------------------------------------------------------------------
def pool_out(n):
    return (n - 1) // 2 + 1


def _taps(H, W):
    """(r, s, row slice, column slice) into the image padded by one: tap (r, s) of window (yo, xo) is padded pixel (2 yo + r, 2 xo + s)"""
    Ho, Wo = pool_out(H), pool_out(W)
    return [(r, s, slice(r, r + 2 * Ho, 2), slice(s, s + 2 * Wo, 2)) for r in range(3) for s in range(3)]


def maxpool_fwd(x):
    """x[B, H, W, C] -> (y, tap): the window maximum and the FIRST maximum in tap order r * 3 + s among the in-bounds taps; an all
    -inf window gives -inf and its first in-bounds tap; a NaN in the window gives NaN (here with the first NaN's tap, which the
    contract does not pin)"""
    x = np.asarray(x, F64)
    B, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = np.zeros((B, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = x
    inb = np.zeros((H + 2, W + 2), bool)
    inb[1:-1, 1:-1] = True
    best = np.full((B, Ho, Wo, C), -np.inf)
    tap = np.full((B, Ho, Wo, C), -1, np.int64)
    for r, s, ys, xs in _taps(H, W):
        v = xp[:, ys, xs]
        ok = inb[ys, xs][None, :, :, None]
        with np.errstate(invalid="ignore"):
            take = ok & ((tap < 0) | (v > best) | (np.isnan(v) & ~np.isnan(best)))
        best = np.where(take, v, best)
        tap = np.where(take, r * 3 + s, tap)
    assert (tap >= 0).all()
    return best, tap.astype(np.uint8)


def maxpool_bwd(dy, tap, H, W):
    """dx[B, H, W, C]: every window's gradient goes to the pixel of its tap; summed where windows overlap"""
    dy = np.asarray(dy, F64)
    B, Ho, Wo, C = dy.shape
    dx = np.zeros((B, H + 2, W + 2, C))
    for r, s, ys, xs in _taps(H, W):
        dx[:, ys, xs] += np.where(tap == r * 3 + s, dy, 0.0)
    assert (dx[:, 0] == 0).all() and (dx[:, -1] == 0).all() and (dx[:, :, 0] == 0).all() and (dx[:, :, -1] == 0).all()
    return dx[:, 1:-1, 1:-1]


def window_taps(H, W):
    """in-bounds taps per window, [Ho, Wo]"""
    inb = np.zeros((H + 2, W + 2), np.int64)
    inb[1:-1, 1:-1] = 1
    return sum(inb[ys, xs] for _, _, ys, xs in _taps(H, W))


def tied_share(x):
    """share of the windows whose maximum is attained at more than one in-bounds tap"""
    x = np.asarray(x, F64)
    B, H, W, C = x.shape
    y, _ = maxpool_fwd(x)
    xp = np.full((B, H + 2, W + 2, C), np.nan)
    xp[:, 1:-1, 1:-1] = x
    cnt = sum((xp[:, ys, xs] == y).astype(np.int64) for _, _, ys, xs in _taps(H, W))
    return float((cnt >= 2).mean())


MAXPOOL_HW = [(h, w) for h in (1, 2, 3, 4) for w in (1, 2, 3, 4)] + [(5, 8), (7, 9)]
MAXPOOL_B = (1, 3)
MAXPOOL_C = {"f32": (4, 12), "bf16": (8, 24)}
MAXPOOL_KINDS = ("gauss", "relu", "const", "special")
TIE_HEAVY = ("relu", "const")                  # ... at every geometry whose windows have more than one tap (H W > 1)


def maxpool_cases(dtype):
    return [(B, H, W, C) for (H, W) in MAXPOOL_HW for B in MAXPOOL_B for C in MAXPOOL_C[dtype]]


def maxpool_input(kind, B, H, W, C, dtype, seed=0):
    """float32 x[B, H, W, C] (bfloat16 values for bf16).  gauss: continuous; relu: what a ReLU of coarse activations
    leaves -- 77 % zeros, 1 where z > 3/4 and 2.5 where z > 2, so that the positive maxima tie as well; const: 1.25 everywhere; special: Gaussian with channel 0 of
    image 0 all -inf, one NaN in channel 1 of the last image and -inf in the top-left 3 x 3 pixels of channel 2"""
    rs = np.random.RandomState(2000 + seed + 1000 * MAXPOOL_KINDS.index(kind) + 97 * B + 31 * H + 7 * W + C)
    z = rs.standard_normal((B, H, W, C))
    if kind == "relu":
        for _ in range(100):                   # (the small images are redrawn until the sample has the shares it is meant to have)
            z = np.where(z > 0.75, np.where(z > 2.0, 2.5, 1.0), 0.0)
            if (z == 0).mean() >= 0.4 and (H * W == 1 or tied_share(z) >= 0.4):
                break
            z = rs.standard_normal((B, H, W, C))
    elif kind == "const":
        z[:] = 1.25
    elif kind == "special":
        z[0, :, :, 0] = -np.inf
        z[B - 1, H // 2, W // 2, 1] = np.nan
        z[0, :3, :3, 2] = -np.inf
    with np.errstate(invalid="ignore"):
        return q(z, dtype)


def maxpool_grad(B, H, W, C, seed=0):
    """multiples of 1/4 in [-8, 8]: the sum of the four windows that can meet in a pixel is exact in float32 and bfloat16"""
    rs = np.random.RandomState(2500 + seed + 97 * B + 31 * H + 7 * W + C)
    return grid(rs, -8, 8, 0.25, (B, pool_out(H), pool_out(W), C))


# ---------------------------------------------------------------------------------------------------------------------
# sums over HW, broadcasts
# ---------------------------------------------------------------------------------------------------------------------
def sum_hw(x, scale=1.0):
    """out[b][c] = scale sum_p x[b][p][c]"""
    return np.asarray(x, F64).sum(1) * scale


def broadcast_hw(v, HW):
    return np.repeat(np.asarray(v, F64)[:, None, :], HW, 1)


def avgpool_bwd(dv, HW, dx0=None):
    """dx[b][p][c] = dv[b][c] / HW (set), + dx0 (add)"""
    out = broadcast_hw(np.asarray(dv, F64) / HW, HW)
    return out if dx0 is None else out + np.asarray(dx0, F64)


def sum_bar(x, scale, scale_exact):
    """(n - 1) eps32 sum |x| for the sum in any order; one rounding for the product with the scale and, unless the scale is a
    float32 value, one for the scale itself"""
    x = np.abs(np.asarray(x, F64))
    s = x.sum(1) * abs(scale)
    return (x.shape[1] - 1) * EPS32 * s + (0 if scale == 1.0 else (1 if scale_exact else 2)) * EPS32 * s * (1 + 2.0 ** -20)


def avgpool_bwd_bar(dv, HW, dx0=None):
    """1 / HW rounded, the product rounded, the sum with the old content rounded"""
    t = np.abs(broadcast_hw(np.asarray(dv, F64) / HW, HW))
    return 2 * EPS32 * t if dx0 is None else 3 * EPS32 * (t + np.abs(np.asarray(dx0, F64)))


def pow2(n):
    return n & (n - 1) == 0


RED_HW = (1, 31, 32, 33, 127, 128, 129, 160)   # one row per lane and fewer; the 4 x 32 body: none, one trip exactly, one and a tail
RED_CV = (1, 7, 8, 9)                          # vector columns: one, one short of a workgroup's eight, eight, nine (a second blockIdx.y)
RED_B = 2
BC_HW = (1, 33)
BC_BIG = (1, 8192, 65)                         # (B, HW, vector columns): 532 480 vector items > CAP_2048, HW a power of two


def layouts(C, V):
    """(ld, offset): dense, and a slice that starts one 16-byte vector into a wider row"""
    return [(C, 0), (C + 2 * V, V)]


def reduce_input(kind, B, HW, C, dtype, seed=0):
    """x[B, HW, C].  exact: integers in [-8, 8]; channel 0 is 256, 1, 0, 0, ... (HW >= 2), whose sum 257 is no bfloat16 value.
    real: Gaussians with a per-channel mean and spread, channel 0 with |mean| / std = 1e4"""
    rs = np.random.RandomState(3000 + seed + 53 * HW + 11 * C + B + (500 if kind == "real" else 0))
    if kind == "exact":
        x = grid(rs, -8, 8, 1.0, (B, HW, C))
        if HW >= 2:
            x[:, :, 0] = 0.0
            x[:, 0, 0], x[:, 1, 0] = 256.0, 1.0
        return q(x, dtype)
    std, mu = rs.uniform(0.5, 2.0, C), rs.standard_normal(C) * 3.0
    std[0], mu[0] = 1.0, 1e4
    return q(rs.standard_normal((B, HW, C)) * std + mu, dtype)


def broadcast_input(kind, B, HW, C, dtype, seed=0):
    """(v[B, C], dx0[B, HW, C]): multiples of 1/4 in [-8, 8] (exact) or Gaussians (real)"""
    rs = np.random.RandomState(3500 + seed + 53 * (HW % 1000) + 11 * C + B + (500 if kind == "real" else 0))
    if kind == "exact":
        return q(grid(rs, -8, 8, 0.25, (B, C)), dtype), q(grid(rs, -8, 8, 0.25, (B, HW, C)), dtype)
    return q(rs.standard_normal((B, C)) * 3.0, dtype), q(rs.standard_normal((B, HW, C)), dtype)


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize, align_corners = False
# ---------------------------------------------------------------------------------------------------------------------
def src_index(out, inn):
    """PyTorch's area_pixel_compute_source_index: s = max(scale (dst + 0.5) - 0.5, 0), i0 = floor(s), i1 = i0 + (i0 < in - 1);
    returns (i0, i1, l0, l1, s)"""
    s = np.maximum((inn / out) * (np.arange(out, dtype=F64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1, s


def lerp_matrix(out, inn):
    """W[out, in]: dst = W src along one axis"""
    i0, i1, l0, l1, _ = src_index(out, inn)
    W = np.zeros((out, inn))
    np.add.at(W, (np.arange(out), i0), l0)
    np.add.at(W, (np.arange(out), i1), l1)
    return W


def lerp_err(out, inn):
    """E[out, in]: how far a float32 weight may be from W (module docstring)"""
    _, _, _, _, s = src_index(out, inn)
    ds = 3 * EPS32 * (s + 0.5) * (1 + 2.0 ** -20)
    near = np.abs(s[:, None] - np.arange(inn)[None, :]) <= 1 + ds[:, None]
    return np.where(near, ds[:, None] + EPS32, 0.0)


def bilinear_fwd(x, H, W):
    """x[B, h, w, C] -> [B, H, W, C], by index (gathers)"""
    x = np.asarray(x, F64)
    _, h, w, _ = x.shape
    y0, y1, ly0, ly1, _ = src_index(H, h)
    x0, x1, lx0, lx1, _ = src_index(W, w)
    a0, a1 = lx0[None, None, :, None], lx1[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    return ly0[None, :, None, None] * (a0 * r0[:, :, x0] + a1 * r0[:, :, x1]) + \
        ly1[None, :, None, None] * (a0 * r1[:, :, x0] + a1 * r1[:, :, x1])


def _sep(My, Mx, a, transpose):
    """transpose False: out[b, Y, X, c] = sum My[Y, y] Mx[X, x] a[b, y, x, c]; True: out[b, y, x, c] = sum My[Y, y] Mx[X, x] a[b, Y, X, c]"""
    if transpose:
        My, Mx = My.T, Mx.T
    t = np.einsum("Yy,byxc->bYxc", My, a, optimize=True)
    return np.einsum("Xx,bYxc->bYXc", Mx, t, optimize=True)


def bilinear_bwd(dy, h, w):
    """the exact transpose of bilinear_fwd: dx[B, h, w, C] from dy[B, H, W, C]"""
    dy = np.asarray(dy, F64)
    return _sep(lerp_matrix(dy.shape[1], h), lerp_matrix(dy.shape[2], w), dy, True)


def bilinear_bar(a, h, w, H, W, bwd):
    """bar of a float32 bilinear_fwd of a[B, h, w, C] (bwd: of bilinear_bwd of a[B, H, W, C])"""
    A = np.abs(np.asarray(a, F64))
    Wy, Wx, Ey, Ex = lerp_matrix(H, h), lerp_matrix(W, w), lerp_err(H, h), lerp_err(W, w)
    n = int((Ey > 0).sum(0).max() * (Ex > 0).sum(0).max()) + 3 if bwd else 5
    return _sep(Ey, Wx, A, bwd) + _sep(Wy, Ex, A, bwd) + _sep(Ey, Ex, A, bwd) + n * EPS32 * _sep(Wy, Wx, A, bwd)


# (h, w) -> (H, W); the issue's eight, then a x2 and a x1/2
BILINEAR_GEOMS = [(5, 7, 20, 28), (5, 7, 13, 17), (1, 1, 6, 5), (8, 8, 8, 8), (13, 10, 5, 4), (7, 9, 1, 1), (6, 5, 1, 9),
                  (33, 33, 129, 129), (3, 5, 6, 10), (6, 10, 3, 5)]
# dyadic weights: x4, identity, 7 -> 1 and 9 -> 1 (source coordinates 3 and 4), x2, x1/2
BILINEAR_EXACT = [(5, 7, 20, 28), (8, 8, 8, 8), (7, 9, 1, 1), (3, 5, 6, 10), (6, 10, 3, 5)]
BILINEAR_C = (4, 12, 8, 24)                    # 4, 12: the scalar kernels; 8, 24: the bf16 -> bf16 16-byte kernels
BILINEAR_FLAGS = [(1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 0, 0)]      # (dtype bf16?, in_f32, out_f32)
BILINEAR_B = 2
# (source, destination) slices as (ld - C, offset): dense; a destination with ld > C at a 16-byte offset; a start 4 elements in --
# 8 bytes for bfloat16, which sends a bf16 -> bf16 call to the scalar fall-back
BILINEAR_LAYOUTS = {"dense": ((0, 0), (0, 0)), "slice": ((8, 8), (16, 8)), "half_vector": ((8, 4), (8, 4))}
BILINEAR_BIG_FWD = (1, 33, 33, 129, 129, 256)  # B, h, w, H, W, C: 129 * 129 * 64 = 1 065 024 four-channel items > CAP_4096
BILINEAR_BIG_BWD = (1, 64, 64, 64, 64, 1028)   # identity: 64 * 64 * 257 = 1 052 672 source items > CAP_4096


def bilinear_input(shape, exact, dtype, seed=0):
    """[B, rows, cols, C]: multiples of 1/4 in [-8, 8] (exact) or Gaussians"""
    rs = np.random.RandomState(4000 + seed + sum(p * int(n) for p, n in zip((1, 3, 17, 5), shape)) % 100003 + (7 if exact else 0))
    return q(grid(rs, -8, 8, 0.25, shape) if exact else rs.standard_normal(shape) * 2.0, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# adaptive average pool, NHWC -> NCHW upsample
# ---------------------------------------------------------------------------------------------------------------------
def bins(n, S):
    return [((i * n) // S, -((-(i + 1) * n) // S)) for i in range(S)]


def adaptive_avgpool(x, S):
    """x[B, H, W, C] -> ([B, S, S, C], sum of |x| per bin, pixels per bin)"""
    x = np.asarray(x, F64)
    B, H, W, C = x.shape
    y, mag, cnt = np.empty((B, S, S, C)), np.empty((B, S, S, C)), np.empty((S, S))
    for i, (y0, y1) in enumerate(bins(H, S)):
        for j, (x0, x1) in enumerate(bins(W, S)):
            blk = x[:, y0:y1, x0:x1]
            cnt[i, j] = (y1 - y0) * (x1 - x0)
            y[:, i, j] = blk.sum((1, 2)) / cnt[i, j]
            mag[:, i, j] = np.abs(blk).sum((1, 2))
    return y, mag, cnt


def adaptive_bar(mag, cnt):
    """a sum of n pixels in any order, then one division"""
    c = cnt[None, :, :, None]
    return (c - 1 + 1) * EPS32 * mag / c * (1 + 2.0 ** -20)


# (B, H, W, C, ld): the three of test_ppm_model.py's kernel test; bins * C = 8 * 36 * 2048 = 589 824 > CAP_2048 at S = 6;
# 53 rows: 18 and 19 rows per bin at S = 3 (more than the 16 row slices, not divisible)
ADAPTIVE_CASES = [(2, 11, 17, 64, 96), (1, 64, 37, 2048, 2048), (3, 6, 6, 16, 16), (8, 6, 6, 2048, 2048), (1, 53, 7, 8, 16)]
ADAPTIVE_S = (1, 2, 3, 6)


def adaptive_input(B, H, W, C, dtype, seed=0):
    rs = np.random.RandomState(5000 + seed + 3 * H + 5 * W + C + B)
    return q(rs.standard_normal((B, H, W, C)) * rs.uniform(0.5, 2.0, C) + rs.standard_normal(C), dtype)


def upsample_nchw(src, H, W, alpha, dst0=None):
    """dst[B, C, H, W] (+)= alpha bilinear(src[B, h, w, C]); alpha the float32 the kernel gets"""
    out = float(F32(alpha)) * bilinear_fwd(src, H, W).transpose(0, 3, 1, 2)
    return out if dst0 is None else out + np.asarray(dst0, F64)


def upsample_bar(src, H, W, alpha, dst0=None):
    """the bilinear value's bar times |alpha|, one rounding for the product with alpha, one for the sum with the old content"""
    a = abs(float(F32(alpha)))
    _, h, w, _ = np.shape(src)
    val = a * np.abs(bilinear_fwd(np.abs(np.asarray(src, F64)), H, W)).transpose(0, 3, 1, 2)
    bar = a * bilinear_bar(src, h, w, H, W, False).transpose(0, 3, 1, 2) + EPS32 * val
    return bar if dst0 is None else bar + EPS32 * (val + np.abs(np.asarray(dst0, F64)))


UPSAMPLE_W = (1, 3, 4, 7, 8)
# name -> (h, H, source width for destination width W, alpha): rows x2 and the columns unchanged -- dyadic weights -- or 3 x 5 -> 7 x W
UPSAMPLE_KINDS = {"exact": (2, 4, None, 0.5), "real": (3, 7, 5, 0.3)}
UPSAMPLE_B, UPSAMPLE_C, UPSAMPLE_LD = 2, 3, 5
UPSAMPLE_BIG = (1, 512, 1368, 3, 1024, 2736)   # B, h, w, C, H, W (x2): 3 * 1024 * 684 = 2 101 248 four-pixel items > CAP_8192


def upsample_input(kind, W, seed=0):
    """(src[B, h, w, C], dst0[B, C, H, W], H, alpha)"""
    h, H, w, alpha = UPSAMPLE_KINDS[kind]
    w = W if w is None else w
    rs = np.random.RandomState(6000 + seed + 13 * W + (1 if kind == "real" else 0))
    shape, dshape = (UPSAMPLE_B, h, w, UPSAMPLE_C), (UPSAMPLE_B, UPSAMPLE_C, H, W)
    if kind == "exact":
        return q(grid(rs, -8, 8, 0.25, shape), "f32"), q(grid(rs, -8, 8, 0.25, dshape), "f32"), H, alpha
    return q(rs.standard_normal(shape) * 2.0, "f32"), q(rs.standard_normal(dshape), "f32"), H, alpha


# ---------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------
def sgd_step(p, g, v, lr, mu, wd, gscale):
    """v = mu v + (gscale g + wd p); p -= lr v, with the float32 parameters the kernel gets; returns (p, v, bar_p, bar_v)"""
    lr, mu, wd, gscale = (float(F32(a)) for a in (lr, mu, wd, gscale))
    p, g, v = (np.asarray(a, F64) for a in (p, g, v))
    nv = mu * v + (gscale * g + wd * p)
    bar_v = 3 * EPS32 * (np.abs(mu * v) + np.abs(gscale * g) + np.abs(wd * p))
    np_ = p - lr * nv
    bar_p = lr * bar_v + 3 * EPS32 * (np.abs(p) + np.abs(lr * nv))
    return np_, nv, bar_p, bar_v


SGD_NS = (1, 2, 3, 4, 5, 7, 1027, 4 * (CAP_2048 + 300) + 3)
# (lr, mu, wd, gscale)
SGD_EXACT = [(0.5, 0.5, 0.25, 2.0), (0.5, 0.5, 0.25, 1.0), (0.5, 0.5, 0.25, 0.25), (0.5, 0.5, 0.0, 2.0), (0.5, 0.0, 0.25, 2.0)]
SGD_REAL = [(0.01, 0.9, 1e-4, 1.0), (0.01, 0.9, 1e-4, 0.25), (0.01, 0.9, 0.0, 0.25), (0.01, 0.0, 1e-4, 1.0)]
SGD_STEPS = 3


def sgd_input(kind, n, seed=0):
    """float32 (p, v, [g of each step])"""
    rs = np.random.RandomState(7000 + seed + n % 9973 + (1 if kind == "real" else 0))
    if kind == "exact":
        return (q(grid(rs, -8, 8, 0.25, n), "f32"), q(grid(rs, -8, 8, 0.25, n), "f32"),
                [q(grid(rs, -8, 8, 0.25, n), "f32") for _ in range(SGD_STEPS)])
    return (q(rs.standard_normal(n), "f32"), q(rs.standard_normal(n) * 0.1, "f32"),
            [q(rs.standard_normal(n) * 0.3, "f32") for _ in range(SGD_STEPS)])


# ---------------------------------------------------------------------------------------------------------------------
# fill, convert
# ---------------------------------------------------------------------------------------------------------------------
FILL_NS = (1, 255, 257, BIG_N)
FILL_VALUES = (1.5, -0.0, float("inf"), float("nan"))
CONVERT_DIRS = [("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16")]

# float32 bit patterns.  Ties between two bfloat16 neighbours with an even (0x3f80, 0xbf80) and an odd (0x3f81, 0xbf81) lower
# neighbour, one unit either side of a tie; the largest finite bfloat16, the float32 just below the tie above it (stays finite),
# that tie and the largest float32 (both inf); float32 denormals (the smallest, ties at 0x0000 / 0x0001, the largest -- which
# rounds to the smallest normal); +-0, +-inf, NaNs (quiet, payload in the low half only, all ones)
SPECIAL_BITS = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
                         0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7F7FFF,
                         0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x80018000,
                         0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)


def to_bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16): round to nearest even on the bits; NaN stays NaN (quiet bit set)"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16).reshape(np.shape(x))


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(F32).reshape(np.shape(b))


def convert_input(n, src, seed=0):
    """n source values as bit patterns (uint32 for f32, uint16 for bf16): the special patterns (n = 1: the first tie), cycled through
    the array's whole length in blocks, and Gaussians over twelve decades"""
    rs = np.random.RandomState(8000 + seed + n % 9973)
    x = (rs.standard_normal(n) * 10.0 ** rs.uniform(-6, 6, n)).astype(F32).view(np.uint32)
    k = len(SPECIAL_BITS)
    for at in range(0, n, 4096):
        m = min(k, n - at)
        x[at:at + m] = SPECIAL_BITS[:m]
    x[max(0, n - k):] = SPECIAL_BITS[:min(k, n)]
    if src == "f32":
        return x
    return np.where((x & 0x7FFFFFFF) > 0x7F800000, (x >> 16) | 0x40, x >> 16).astype(np.uint16)      # truncated: any bfloat16 will do


def convert_ref(bits, src, dst):
    """destination bit patterns"""
    if src == dst:
        return bits
    return to_bf16_bits(bits.view(F32)) if dst == "bf16" else from_bf16_bits(bits).view(np.uint32)


def bits_same(got, ref, dst):
    """bit for bit; a NaN only has to be a NaN"""
    f = (lambda b: from_bf16_bits(b)) if dst == "bf16" else (lambda b: b.view(F32))
    return (got == ref) | (np.isnan(f(np.ascontiguousarray(got))) & np.isnan(f(np.ascontiguousarray(ref))))
