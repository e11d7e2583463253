"""Case table shared by tests/test_knn_refs.py (CPU) and tests/test_gpu_knn_score.py (GPU): the float64 definition of the
kNN cosine-similarity anomaly score (dml_knn_cosine_score; `--ood knn`, anomaly/eval_ood_traditional.py:511-530 of the
reference), its seeded inputs and the error bar.  A plain module in the style of tests/novel_cases.py (no fixtures, no
hooks); nothing here looks at a kernel's output.

The definition, R = neighbor_size - 1:
    n(b,y,x)     = f(b,:,y,x) / max(|f(b,:,y,x)|_2, 1e-8)
    score(b,y,x) = sum_{i=1..R} sum_{j=1..R} n(b,y,x) . n(b,y+i,x+j) + n(b,y,x) . n(b,y-i,x-j)
with 0 for a neighbour outside the image.  T(p) = sum_c |n_c(p)| sum_o |n_c(p+o)| over the same 2 R^2 offsets bounds every
partial sum of every evaluation order, with or without the factorisation sum_c n_c(p) sum_o n_c(p+o) (T >= sum_o |cos_o|).

The bar, per pixel: 256 * 2^-24 * T(p).  Any summation order of either kernel form chains fewer than 256 rounded
operations per output -- the norm (up to 32 products and additions), the square root, the division and up to
32 + 2 * 16^2 products and additions for the largest supported case -- and each is relative to a partial sum bounded by T.
A dropped or doubled neighbour moves a pixel by up to 1, about a thousand bars.  No pixel is left out of a comparison.
"""
import numpy as np

EPS32 = 2.0 ** -24
MAXC = 32                       # csrc/common.h
MAX_NEIGHBOR_SIZE = 17
CLAMP = 1e-8                    # ATen's cosine_similarity eps, applied to each vector's norm on its own
BAR_OPS = 256

# name -> ((B, C, H, W), neighbor_size, flavour).  Flavours: "plain"; "subeps" -- a block of pixels with components in
# 1e-12 .. 1e-9, norms below the clamp; "big" -- everything scaled by 1e15 (the squares stay finite in fp32; |f| <= 1e18
# is the documented input range).  Every case is 2.5 N(0,1) with the pixels (y % 5 == 1, x % 7 == 1) set to the zero vector.
CASES = {
    "one_pixel": ((1, 13, 1, 1), 9, "plain"),
    "short": ((1, 13, 3, 40), 9, "plain"),               # smaller than the neighbourhood in one direction
    "narrow": ((1, 13, 40, 3), 9, "plain"),
    "size_R": ((1, 13, 8, 8), 9, "plain"),               # exactly R: no in-image far corner neighbour
    "size_R1": ((1, 13, 9, 9), 9, "plain"),              # R + 1: the first one appears
    "c1": ((2, 1, 20, 33), 9, "plain"),                  # every cosine is +-1 or 0: an integer score, compared exactly
    "c32_big": ((2, 32, 17, 70), 9, "big"),              # largest C, a batch of two
    "seams": ((1, 13, 70, 130), 9, "subeps"),            # odd sizes over several tiles both ways
    "scalar": ((1, 13, 70, 131), 9, "plain"),            # W % 4 != 0
    "ns1": ((1, 13, 40, 50), 1, "plain"),                # all zeros
    "ns2": ((1, 13, 40, 50), 2, "plain"),                # R = 1
    "ns17": ((1, 13, 40, 50), 17, "plain"),              # the supported maximum
    # beyond the issue's table: the 16-byte load path over several tiles, and R that is no multiple of 4 on both paths
    "vec_seams": ((1, 13, 40, 132), 9, "plain"),
    "vec_ns2": ((1, 5, 36, 72), 2, "plain"),
    "vec_ns4": ((1, 5, 36, 72), 4, "plain"),
    "vec_ns6": ((1, 5, 36, 72), 6, "plain"),
    "vec_ns17": ((2, 5, 36, 72), 17, "plain"),
    "scalar_ns4": ((1, 5, 36, 71), 4, "plain"),
    "scalar_ns6": ((1, 5, 36, 71), 6, "plain"),
}
OFFSET_CASES = ("seams", "vec_seams")                    # run again with the features pointer offset by one float
SUBEPS_BLOCK = (slice(11, 23), slice(60, 75))            # rows, columns of the "subeps" block


def features(name):
    """the seeded float32 input [B, C, H, W] of a case"""
    (B, C, Hh, Ww), _, flavour = CASES[name]
    rs = np.random.RandomState(4100 + sorted(CASES).index(name))
    f = 2.5 * rs.standard_normal((B, C, Hh, Ww))
    if flavour == "subeps":
        ys, xs = SUBEPS_BLOCK
        blk = f[:, :, ys, xs]
        f[:, :, ys, xs] = np.sign(blk) * 10.0 ** rs.uniform(-12.0, -9.0, blk.shape)
    if flavour == "big":
        f *= 1e15
    f[:, :, 1::5, 1::7] = 0.0
    return f.astype(np.float32)


def score_ref(feats, neighbor_size):
    """float64 of the definition on float32 feats [B, C, H, W] -> (score [B, H, W], T [B, H, W])"""
    f = feats.astype(np.float64)
    B, C, Hh, Ww = f.shape
    R = neighbor_size - 1
    n = f / np.maximum(np.sqrt((f * f).sum(axis=1, keepdims=True)), CLAMP)
    a = np.abs(n)
    S = np.zeros_like(n)
    SA = np.zeros_like(n)
    for i in range(1, min(R, Hh - 1) + 1):
        for j in range(1, min(R, Ww - 1) + 1):
            S[:, :, :Hh - i, :Ww - j] += n[:, :, i:, j:]          # the neighbour at (y + i, x + j)
            S[:, :, i:, j:] += n[:, :, :Hh - i, :Ww - j]          # the neighbour at (y - i, x - j)
            SA[:, :, :Hh - i, :Ww - j] += a[:, :, i:, j:]
            SA[:, :, i:, j:] += a[:, :, :Hh - i, :Ww - j]
    return (n * S).sum(axis=1), (a * SA).sum(axis=1)


def bar(T):
    return BAR_OPS * EPS32 * T


_REFS = {}


def reference(name):
    """(feats, score, T) of a case, computed once and shared (callers must not modify it)"""
    if name not in _REFS:
        f = features(name)
        s, T = score_ref(f, CASES[name][1])
        for arr in (f, s, T):
            arr.setflags(write=False)
        _REFS[name] = (f, s, T)
    return _REFS[name]
