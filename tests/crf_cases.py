"""The float64 definition of the Gaussian dense-CRF confidence (`--ood crf-gauss`, dml_crf_gauss) in numpy, the seeded inputs
and the case list that tests/test_crf_refs.py (CPU) and tests/test_gpu_crf_gauss.py (GPU) share.

For one image, L [C, H, W] the scores of the classes taken part, y the row and x the column:
    U_c    = -log(min(max(softmax_c(L), clip), 1))                                     (pydensecrf's unary_from_softmax)
    kx(d)  = exp(-d^2 / (2 sx^2)) for |d| <= Rx = ceil(6 sx), else 0; ky, Ry alike; sums over the pixels inside the image,
             the pixel itself included
    nx(x)  = 1 / sqrt(sum_x' kx(x - x')), ny(y) alike                (densecrf's NORMALIZE_SYMMETRIC, which factorises)
    M_c    = ny(y) nx(x) sum_y' ky(y - y') ny(y') sum_x' kx(x - x') nx(x') Q_c(y', x')
    Q^0    = softmax_c(-U),  Q^{t+1} = softmax_c(-U + compat M(Q^t))
    conf   = max_c Q^iters,  map = argmax_c Q^iters (lowest index on a tie)
The 1-D kernels are dense matrices here and every sum a matrix product: nothing is shared with the device code's tiling.
"""
import functools
import math

import numpy as np

F64 = np.float64
CLIP = 1e-5
GPU_BAR = 1e-5               # |conf - conf64| on every pixel: about 10 x the float32 numpy restatement's deviation
TIE_GAP = 1e-4               # pixels whose two largest float64 Q are closer than this may differ in `map`
MAX_CLASSES, MAX_SIGMA = 32, 8.0


def radius(sigma):
    return int(math.ceil(6.0 * sigma))


def kernel_matrix(n, sigma, R="6sigma", dtype=F64):
    """K[i, j] = exp(-(i - j)^2 / (2 sigma^2)) for |i - j| <= R (R=None: no cut), in float64, then cast"""
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    k = np.exp(-(d.astype(F64) ** 2) / (2.0 * float(sigma) ** 2))
    if R is not None:
        k = np.where(np.abs(d) <= (radius(sigma) if R == "6sigma" else R), k, 0.0)
    return k.astype(dtype)


def softmax0(a):
    e = np.exp(a - a.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def unary(L, clip=CLIP):
    return -np.log(np.minimum(np.maximum(softmax0(L), L.dtype.type(clip)), L.dtype.type(1.0)))


def filters(H, W, sx, sy, R="6sigma", dtype=F64):
    """the two normalised 1-D operators: message = Ay @ Q_c @ Ax^T with A = diag(n) K diag(n)"""
    Kx, Ky = kernel_matrix(W, sx, R, dtype), kernel_matrix(H, sy, R, dtype)
    nx, ny = 1.0 / np.sqrt(Kx.sum(axis=1)), 1.0 / np.sqrt(Ky.sum(axis=1))
    return (nx[:, None] * Kx * nx[None, :]).astype(dtype), (ny[:, None] * Ky * ny[None, :]).astype(dtype)


def message(Q, Ax, Ay):
    return np.einsum("yv,cvw,xw->cyx", Ay, Q, Ax, optimize=True)


def mean_field(L, sx=3.0, sy=None, compat=3.0, iters=100, clip=CLIP, R="6sigma", dtype=F64):
    """L [C, H, W] -> Q^iters [C, H, W], everything in `dtype` (float64: the definition; float32: its restatement in the
    device's number format)"""
    L = np.asarray(L).astype(dtype)
    sy = sx if sy is None else sy
    C, H, W = L.shape
    U = unary(L, clip)
    Ax, Ay = filters(H, W, sx, sy, R, dtype)
    Q = softmax0(-U)
    for _ in range(iters):
        Q = softmax0(-U + dtype(compat) * message(Q, Ax, Ay))
    return Q


def score_ref(lg, k_first=0, **kw):
    """lg [B, K, H, W] float32 -> {"conf" [B, H, W], "map" int64, "tie" bool: top-2 gap below TIE_GAP}, image by image"""
    conf, lab, tie = [], [], []
    for img in lg:
        Q = mean_field(img[k_first:], **kw)
        top = np.sort(Q, axis=0)
        conf.append(Q.max(axis=0))
        lab.append(Q.argmax(axis=0).astype(np.int64))
        tie.append((top[-1] - top[-2]) < TIE_GAP if Q.shape[0] > 1 else np.zeros(Q.shape[1:], bool))
    return {"conf": np.stack(conf), "map": np.stack(lab), "tie": np.stack(tie)}


def logits(shape, scale, seed):
    """scale * (a low-resolution field, each value replicated over 8 x 8 pixels, + 0.3 * per-pixel noise): smooth regions
    with noisy borders, so that the CRF changes 7 - 12 % of the labels"""
    B, K, H, W = shape
    rng = np.random.default_rng(seed)
    low = rng.standard_normal((B, K, (H + 7) // 8, (W + 7) // 8))
    pix = rng.standard_normal((B, K, H, W))
    up = np.repeat(np.repeat(low, 8, axis=2), 8, axis=3)[:, :, :H, :W]
    return (scale * (up + 0.3 * pix)).astype(np.float32)


def case(shape, iters, scale, seed, sxy=3.0, compat=3.0, k_first=0):
    sx, sy = sxy if isinstance(sxy, tuple) else (sxy, sxy)
    return {"shape": shape, "iters": iters, "scale": scale, "seed": seed, "sx": float(sx), "sy": float(sy),
            "compat": float(compat), "k_first": k_first, "clip": CLIP}


# The device's tiles: the row launch owns 4 rows x 256 columns of the B C H rows, the column launch 64 columns x 32 rows
# (C <= 16) or x 16 rows (C > 16).  "over" / "under" sit one pixel past / one pixel short of a tile edge in both directions.
CASES = {
    "tiny_it0": case((1, 13, 5, 7), 0, 2.0, 11),              # image smaller than the radius in both directions
    "tiny_it1": case((1, 13, 5, 7), 1, 2.0, 11),
    "tiny_it100": case((1, 13, 5, 7), 100, 2.0, 11),
    "odd_it5": case((1, 12, 23, 37), 5, 1.0, 12),             # odd sizes, W % 4 != 0
    "odd_it100": case((1, 12, 23, 37), 100, 1.0, 12),
    "kfirst_it100": case((1, 14, 40, 56), 100, 4.0, 13, k_first=1),
    "tiles_batch_it100": case((2, 13, 70, 130), 100, 2.0, 14),
    "tiles_over_it5": case((2, 13, 33, 257), 5, 2.0, 15),
    "tiles_under_it5": case((1, 13, 31, 255), 5, 1.0, 16),
    "c2_it5": case((1, 2, 9, 33), 5, 2.0, 17),                # smallest and largest C
    "c32_it5": case((1, 32, 9, 33), 5, 2.0, 18),
    "c32_tiles_it5": case((1, 32, 17, 65), 5, 4.0, 19),       # the 16-row tile of C > 16, one pixel past it
    "c17_it5": case((1, 17, 15, 63), 5, 1.0, 20),             # the first C of that kernel, one pixel short of its tile
    "c16_it5": case((1, 16, 15, 63), 5, 1.0, 20),             # the last C of the 32-row kernel
    "row_it5": case((1, 13, 1, 40), 5, 2.0, 21),              # degenerate axes
    "col_it5": case((1, 13, 40, 1), 5, 2.0, 22),
    "aniso_it5": case((1, 13, 23, 37), 5, 2.0, 23, sxy=(1.5, 4.0)),
    "wide_it5": case((1, 13, 23, 37), 5, 2.0, 23, sxy=(8.0, 8.0)),     # the largest radius, 48, on a frame half its size
    "plain_it5": case((1, 13, 23, 37), 5, 4.0, 24),           # compat = 0, offset pointer
    "plain_it100": case((1, 13, 23, 37), 100, 4.0, 24),       # two runs
}
BATCH_CASES = ("tiles_batch_it100", "tiles_over_it5")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(logits [B, K, H, W] float32, read-only; the float64 definition on them) -- computed once per process"""
    c = CASES[name]
    lg = logits(c["shape"], c["scale"], c["seed"])
    lg.setflags(write=False)
    ref = score_ref(lg, c["k_first"], sx=c["sx"], sy=c["sy"], compat=c["compat"], iters=c["iters"], clip=c["clip"])
    for v in ref.values():
        v.setflags(write=False)
    return lg, ref
