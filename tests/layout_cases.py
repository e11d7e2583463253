"""Case table shared by tests/test_layout_refs.py (CPU) and tests/test_gpu_layout_edges.py (GPU): plain numpy definitions of the
weight-layout, input-packing, space-to-depth, tap-gather and bias-gradient contracts of include/dmlnet_hip.h (the non-elementwise
half of csrc/optim_layout.hip), the seeded inputs and the case tables.  A plain module (no fixtures, no hooks, numpy only);
nothing here looks at a kernel's output or imports the library.

The layouts are written as reshape / transpose of numpy arrays, never as a kernel's index arithmetic, and are compared bit for
bit: a float32 output is a copy (the pure copies carry -0.0, subnormals, infinities and NaN payloads), a bfloat16 output the
single round-to-nearest-even of the float32 master, a padding channel +0.  The two accumulating copies (dml_unpad_wgrad,
dml_s2d_wgrad) add ONE float32 value to one float32 value: numpy's float32 addition is that single rounding.

Bias gradient, two kinds of input:
  exact  integers in [-3, 3] (db beforehand: integers in [-8, 8]): every partial sum in any order is an integer below 2^24, so the
         kernel must EQUAL the float64 sum;
  real   seeded Gaussians, per column against the float64 sum of the same (float32, or bfloat16-rounded) inputs with the bar
             c * 2^-24 * (|db before| + sum_m |dy[m][n]|)
         -- the call accumulates, so the value db held before is one more term of the sum -- where c is the number of additions
         on the longest chain a term goes through, counted from the code by bias_chain() below:
           vector kernel (N % V == 0, ldy % V == 0, dy 16-byte aligned; V = 4 float32 / 8 bfloat16; NV = N / V, rt = 256 // NV row
           lanes, rpb = ceil(M / 1024) rows per workgroup, grid = ceil(M / rpb) workgroups)
             walk    ceil(rpb / rt)    a thread adds every rt-th row of its workgroup's rpb rows into its accumulator
             LDS     rt                one thread per channel adds the rt row lanes
             then    grid              atomics: the workgroups' sums arrive at db one after another, in any order
             or      ceil(grid / rf) + rf + 1     workspace: bias_grad_fold_kernel walks the grid partial rows with rf = 256 // N
                                       lanes, adds the rf lanes through LDS and adds the result to db
           scalar kernel (anything else; rt = 256 // N row lanes, grid = min(512, ceil(M / rt)) workgroups, fewer when the
           workspace holds fewer than grid * rt rows)
             walk    ceil(M / (grid * rt))
             then    grid * rt         atomics: every row lane of every workgroup adds to db itself
             or      ceil(grid * rt / rt) + rt + 1 = grid + rt + 1    workspace: the fold over grid * rt partial rows
         First-order in 2^-24: the two additions to an accumulator that starts at zero are exact, which covers the second order
         (c^2 2^-48 / 2 is below 0.04 of one unit at the longest chain here).
No bar is measured on a kernel.
"""
import numpy as np

from bn_cases import EPS32, F32, F64, bf16_round, vec  # noqa: F401  (re-exported)

U32, U16 = np.uint32, np.uint16
CAP_2048 = 2048 * 256                          # prep_weight, unpad_wgrad (elements)
CAP_4096 = 4096 * 256                          # pack_input (pixels), pack_input_s2d (half-size pixels), gather_taps (float4)

SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00ABC,
                         0x7F7FFFFF, 0x00800000], U32)     # -0, subnormals, infinities, NaN payloads, the largest / smallest normal


def values(shape, seed, special=False):
    """float32 Gaussians; special: every 7th element (from the 3rd) is one of SPECIAL_BITS in turn"""
    a = np.random.RandomState(5000 + seed).standard_normal(int(np.prod(shape))).astype(F32)
    if special:
        idx = np.arange(3, a.size, 7)
        a.view(U32)[idx] = SPECIAL_BITS[np.arange(idx.size) % SPECIAL_BITS.size]
    return a.reshape(shape)


def ints(shape, seed, lo=-3, hi=3):
    return np.random.RandomState(6000 + seed).randint(lo, hi + 1, shape).astype(F32)


def bits(a, dtype):
    """the bit patterns a buffer of `dtype` holds for the float32 array a: itself, or its round-to-nearest-even to bfloat16"""
    a = np.ascontiguousarray(a, F32)
    if dtype == "f32":
        return a.view(U32).copy()
    assert np.isfinite(a).all()
    return (bf16_round(a).view(U32) >> 16).astype(U16)


def tile_major(m):
    """[rows][K] -> [rows / 64][K / 32][64][32] (DmlPrepDesc.w_tiled / wt_tiled), flat"""
    rows, K = m.shape
    assert rows % 64 == 0 and K % 32 == 0
    return m.reshape(rows // 64, 64, K // 32, 32).transpose(0, 2, 1, 3).reshape(-1)


def tiled_ok(N, RS, Cp):
    """(w may be tiled, wt may be tiled): the header's rows % 64 == 0 and K % 32 == 0"""
    return (N % 64 == 0 and (RS * Cp) % 32 == 0), (Cp % 64 == 0 and (RS * N) % 32 == 0)


def prep_ref(master, Cp, dtype, w_tiled=0, wt_tiled=0):
    """master[N][RS][Cm] float32 -> (w, wt) flat bit patterns: w[N][RS][Cp] zero padded, wt[Cp][RS][N] its transpose"""
    N, RS, Cm = master.shape
    w = np.zeros((N, RS, Cp), F32)
    w.view(U32)[:, :, :Cm] = master.view(U32)
    wb = bits(w, dtype)
    wtb = np.ascontiguousarray(wb.transpose(2, 1, 0))
    fw = tile_major(wb.reshape(N, RS * Cp)) if w_tiled else wb.reshape(-1)
    fwt = tile_major(wtb.reshape(Cp, RS * N)) if wt_tiled else wtb.reshape(-1)
    return fw, fwt


def unpad_ref(src, dst0, Cm):
    """dst[N][RS][Cm] += src[N][RS][Cp]"""
    return (np.asarray(dst0, F32) + np.asarray(src, F32)[:, :, :Cm]).astype(F32)


def pack_input_ref(x, Cp, dtype):
    """x[B][C][H][W] -> NHWC with C padded to Cp, flat bit patterns"""
    B, C, H, W = x.shape
    y = np.zeros((B, H, W, Cp), F32)
    y.view(U32)[..., :C] = x.view(U32).transpose(0, 2, 3, 1)
    return bits(y, dtype).reshape(-1)


def pack_s2d_ref(x):
    """x[B][C][H][W] -> x2[B][H/2][W/2][4 C], channel (dy 2 + dx) C + c = x[b][c][2 y2 + dy][2 x2 + dx]"""
    B, C, H, W = x.shape
    return np.ascontiguousarray(x.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 2, 4, 3, 5, 1)).reshape(B, H // 2, W // 2, 4 * C)


def s2d_weights_ref(w):
    """w[N][k][k][C] -> w2[N][k2][k2][4 C], k2 = (k + 1) / 2: w2[n][r2][s2][(dy 2 + dx) C + c] = w[n][2 r2 + dy - 1][2 s2 + dx - 1][c],
    zero outside 0 .. k - 1: one zero row and column in front, then the same regrouping as the image's"""
    N, k, _, C = w.shape
    k2 = (k + 1) // 2
    wp = np.zeros((N, 2 * k2, 2 * k2, C), w.dtype)
    wp[:, 1:, 1:] = w
    return np.ascontiguousarray(wp.reshape(N, k2, 2, k2, 2, C).transpose(0, 1, 3, 2, 4, 5)).reshape(N, k2, k2, 4 * C)


def s2d_scatter(g2, k):
    """the adjoint of s2d_weights_ref: g2[N][k2][k2][4 C] -> g[N][k][k][C] (every w2 element has at most one source)"""
    N, k2, _, C4 = g2.shape
    C = C4 // 4
    gp = g2.reshape(N, k2, k2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * k2, 2 * k2, C)
    return np.ascontiguousarray(gp[:, 1:, 1:])


def s2d_wgrad_ref(dw2, dw0, k):
    return (np.asarray(dw0, F32) + s2d_scatter(np.asarray(dw2, F32), k)).astype(F32)


def gather_ref(src, taps):
    """src[rows][taps_src][n] -> dst[rows][len(taps)][n]"""
    return np.ascontiguousarray(src[:, list(taps), :])


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
# (N, RS, Cm, Cp, with wt, [(w_tiled, wt_tiled), ...])
ALL4 = [(0, 0), (1, 0), (0, 1), (1, 1)]
PREP_TABLE = [
    (24, 9, 304, 320, True, [(0, 0)]),          # the head's 24 rows: a ragged tile in n, ten tiles in c
    (33, 1, 35, 40, True, [(0, 0)]),            # ragged both ways, padding channels inside a tile
    (64, 49, 3, 8, False, [(0, 0)]),            # wt = NULL
    (1, 1, 1, 1, True, [(0, 0)]),
    (96, 49, 96, 96, True, [(0, 0)]),           # 3 * 3 * 49 = 441 tiles > 256 workgroups: the blockIdx.x stride
    # the header allows a tile-major wt only with Cp % 64 == 0 (a 32-row wt would be written past its Cp * RS * N elements):
    # the 32-channel shape runs the two w layouts, the 64-channel one beside it all four
    (64, 1, 32, 32, True, [(0, 0), (1, 0)]),
    (64, 1, 64, 64, True, ALL4),
    (128, 9, 60, 64, True, ALL4),
]


def prep_descs():
    """the heterogeneous table: one descriptor per (shape, layout combination)"""
    out = []
    for N, RS, Cm, Cp, has_wt, combos in PREP_TABLE:
        okw, okt = tiled_ok(N, RS, Cp)
        for wtl, wttl in combos:
            assert (okw or not wtl) and (okt or not wttl) and (has_wt or not wttl)
            out.append((N, RS, Cm, Cp, has_wt, wtl, wttl))
    return out


def prep_master(N, RS, Cm, dtype, seed):
    return values((N, RS, Cm), seed, special=dtype == "f32")


PREP_BIG = (130, 9, 449, 456)                   # 533 520 elements > CAP_2048: prep_weight's second trip, ragged channels
UNPAD_CASES = [(5, 9, 13, 16), (7, 3, 24, 24), (1, 1, 5, 8), (130, 9, 449, 456), (130, 9, 456, 456)]      # (N, RS, Cm, Cp)

PACK_CCP = [(3, 8), (1, 8), (8, 8), (3, 3)]
PACK_MAPS = [(2, 1, 1), (2, 7, 9), (1, 5, 3)]    # (B, H, W)
PACK_BIG = (1, 1025, 1024)                       # 1 049 600 pixels > CAP_4096
S2D_PACK = [(2, 1, 2, 2), (2, 1, 6, 4), (2, 3, 2, 2), (1, 3, 6, 4)]     # (B, C, H, W)
S2D_PACK_BIG = (1, 3, 2050, 2050)                # 1 050 625 half-size pixels > CAP_4096
S2D_K, S2D_N, S2D_C = (3, 7, 11), (1, 24), (1, 3)
S2D_BAD_K = (1, 4, 5, 9)

# (rows, taps_src, n, taps)
GATHER_CASES = [(3, 9, 4, (4,)), (5, 9, 8, (8, 0)), (2, 9, 12, (6, 6, 2)), (4, 9, 4, (7, 5, 2, 0)), (1, 1, 4, (0, 0, 0, 0)),
                (7, 4, 20, (3, 1))]
GATHER_BIG = (257, 9, 4096, (8, 2, 5, 0))        # 257 * 4 * 1024 = 1 052 672 float4 > CAP_4096

# ---------------------------------------------------------------------------------------------------------------------
# bias gradient
# ---------------------------------------------------------------------------------------------------------------------
BIAS_N = (1, 4, 8, 12, 13, 16, 24, 255, 256)
BIAS_VEC_M = (1023, 1024, 1025, 2049)
WS_ROWS = 1024                                  # the header's workspace: 1024 * N floats


def bias_kernel(N, ldy, dtype, aligned=True):
    V = vec(dtype)
    return "vec" if (N % V == 0 and ldy % V == 0 and aligned) else "scalar"


def bias_rt(N, dtype, kern):
    return 256 // (N // vec(dtype)) if kern == "vec" else 256 // N


def bias_ms(N, dtype):
    """M around the kernel's row lanes, the vector kernel's change of rows per workgroup, the scalar kernel's grid cap"""
    kern = bias_kernel(N, N, dtype)
    rt = bias_rt(N, dtype, kern)
    ms = {1, rt - 1, rt, rt + 1}
    ms |= set(BIAS_VEC_M) if kern == "vec" else {512 * rt + 1}
    return sorted(m for m in ms if m >= 1)


def ceil_div(a, b):
    return -(-a // b)


def bias_grid(M, N, dtype, kern, ws_elems=None):
    """(workgroups, partial rows in the workspace)"""
    if kern == "vec":
        rpb = ceil_div(M, 1024)
        g = ceil_div(M, rpb)
        return g, g
    rt = 256 // N
    g = min(512, ceil_div(M, rt))
    if ws_elems is not None and g * rt * N > ws_elems:
        g = ws_elems // (rt * N)
    return g, g * rt


def bias_chain(M, N, dtype, kern, ws_elems=None):
    """additions on the longest chain (see the module docstring)"""
    g, rows = bias_grid(M, N, dtype, kern, ws_elems)
    if kern == "vec":
        rt = bias_rt(N, dtype, kern)
        c = ceil_div(ceil_div(M, 1024), rt) + rt
    else:
        rt = 256 // N
        c = ceil_div(M, g * rt)
    if ws_elems is None:
        return c + rows
    rf = 256 // N
    return c + ceil_div(rows, rf) + rf + 1


def bias_input(kind, M, N, dtype, seed=0):
    """(dy[M][N], db before [N]) as float32 values a buffer of `dtype` holds exactly"""
    if kind == "exact":
        return ints((M, N), seed + M + 7 * N), ints((N,), seed + 1 + N, -8, 8) * 2 + 1
    dy = values((M, N), seed + M + 7 * N)
    dy = bf16_round(dy) if dtype == "bf16" else dy
    return dy, values((N,), seed + 3 + N) + F32(0.5)


def bias_ref(dy, db0):
    return np.asarray(db0, F64) + np.asarray(dy, F64).sum(0)


def bias_bar(dy, db0, c):
    return c * EPS32 * (np.abs(np.asarray(db0, F64)) + np.abs(np.asarray(dy, F64)).sum(0))
