"""Case table shared by tests/test_head_refs.py (CPU) and tests/test_gpu_head_edges.py (GPU): the float64 definitions of the four
distance-head contracts of include/dmlnet_hip.h (dml_proto_dist_fwd, dml_upsample_dist_fwd, dml_proto_dist_bwd,
dml_proto_dist_nhwc), the seeded input generators, the case tables, the dispatch conditions of the entry points as a pure
function, the error bars and the comparison functions both test files use.  A plain module (numpy only): nothing here imports the
library or looks at a kernel's output other than as the `got` argument of a comparison.  The bilinear stage is
pool_cases.bilinear_fwd / bilinear_bar; there is no second resize definition.

eps32 = 2^-24 is float32's unit roundoff.  Two kinds of input, as in pool_cases.py:
  exact  embeddings that are integers in [-2, 2], prototypes 3 I ("eye"), a small-integer matrix ("int") and one with two identical
         rows ("dup"); resize ratios x4, x2, x1 and x1/2 on both axes ("dyadic" geometries: weights are multiples of 1/8).  Every
         interpolated feature is a multiple of 1/64, every squared difference a multiple of 2^-12, and the magnitudes one pixel sums
         over channels and prototypes stay below 2^12: every intermediate is a float32 value in any order and under contraction
         (tests/test_head_refs.py asserts it case by case), so the kernel must EQUAL the float64 result.  Pixel 0 of every exact
         input is a tie: it sits on the duplicated prototype ("dup") or at (1, 1, 0, ...), equidistant from rows 0 and 1 of 3 I; the
         expected index is the first.  The upsampled head runs its exact inputs on the dyadic geometries only (upsample_kinds):
         elsewhere integer data is not exact, and its interpolated ties would make the argmax check idle;
  real   seeded Gaussians (features x 1.5, prototypes 3 I + 0.05 N) and the data that hurts: pixel 0 equals a prototype (d = 0),
         the middle pixel has magnitude 1e3, and -- where the arithmetic of kernel and definition is the same, term for term, i.e.
         dml_proto_dist_fwd and dml_proto_dist_nhwc -- one inf, one NaN and one -0.0 feature.  The upsampled head gets its inf and
         NaN in cases of their own (UP_SPECIAL): every output pixel with a tap of non-zero weight on them must be non-finite, every
         pixel whose taps and their neighbouring columns are clean must be as good as without them; what a kernel makes of a zero
         weight times inf in between is not part of the contract (include/dmlnet_hip.h).

Bars, each the count of float32 roundings (never measured on a kernel):
  distance      d = sum of C terms fl(fl(f - m)^2) >= 0 in any order, contracted or not: one rounding for the difference (twice, it
                is squared), one for the square, C - 1 for the sum, one unit for the second order: (C + 3) eps32 d;
  dissum        K logits summed in any order: (K - 1) eps32 sum_k |logit_k| + sum_k bar_k;
  upsampled     Df = pool_cases.bilinear_bar of the embedding; the logit bar adds sum_c (2 |f_c - m_kc| Df_c + Df_c^2);
  backward      df_c = -2 (gs f_c - gm_c) (+ gf_c) with gs = sum_k g_k and gm_c = sum_k g_k m_kc.  With A = sum_k |g_k| |f_c| and
                M = sum_k |g_k m_kc|:  gs, K - 1 additions: (K - 1) eps32 A;  the product gs f_c: eps32 A;  gm_c, K products and
                K - 1 additions: K eps32 M;  the difference: eps32 (A + M);  the factor -2 is exact.  Together
                2 (K + 1) eps32 (A + M); the optional addition of gf_c: eps32 (2 (A + M) + |gf_c|).  Both times (1 + 2^-18) for the
                second order (at most 40 roundings compound).  The bar is absolute: a channel where gs f and gm cancel is compared
                against the magnitudes that entered, not against the small result;
  NHWC          the distance bar with the Kp channels the kernel sums (the pad channels add zeros).
Argmax: the first maximum (a NaN logit never wins; no logit above -inf gives 0).  On real data a pixel must equal the float64 first
maximum wherever the float64 margin between the top two logits exceeds the sum of their two bars; elsewhere it must name a class
whose logit is within the bars of the maximum.  The share of pixels excused this way is at most ARGMAX_EXCUSED_CAP per case -- a
condition on the inputs, asserted on the reference alone by tests/test_head_refs.py; exact cases excuse nothing.
"""
import itertools

import numpy as np

import pool_cases as PC
from bn_cases import EPS32, F32, F64

MAXC, MAXK = 32, 33                            # what head.hip supports
CAP_4096 = 4096 * 256                          # grid_for(..., 256, 256 * 16): items of the generic forward / upsample / backward kernels
CAP_2048 = 2048 * 256                          # grid_for's default: rows of proto_dist_nhwc_kernel
ARGMAX_EXCUSED_CAP = 1e-3
SECOND = 1 + 2.0 ** -18
PROTO_KINDS = ("eye", "int", "dup")            # of exact inputs; real inputs have "real"


# ---------------------------------------------------------------------------------------------------------------------
# float64 definitions
# ---------------------------------------------------------------------------------------------------------------------
def first_max(logits):
    """logits[B, K, ...] -> the first k of the largest logit; a NaN never wins, and with no logit above -inf the answer is 0"""
    lg = np.asarray(logits, F64)
    return np.argmax(np.where(np.isnan(lg), -np.inf, lg), 1).astype(np.uint8)


def head_fwd(f, P, Df=None, bars=True):
    """f[B, H, W, C] features (NHWC), P[K, C] -> dict: logits[B, K, H, W] = -sum_c (f - P_k)^2 (NCHW), lbar, argmax[B, H, W] (first
    maximum), dissum[B, H, W] = -sum_k logits, dbar.  Df: the bar of f itself (the upsampled head)."""
    f, P = np.asarray(f, F64), np.asarray(P, F64)
    B, H, W, C = f.shape
    K = P.shape[0]
    logits = np.empty((B, K, H, W))
    lbar = np.empty((B, K, H, W)) if bars else None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            t = f - P[k]
            d = (t * t).sum(-1)
            logits[:, k] = -d
            if bars:
                lbar[:, k] = (C + 3) * EPS32 * d
                if Df is not None:
                    lbar[:, k] += (2 * np.abs(t) * Df + Df * Df).sum(-1)
        out = {"logits": logits, "lbar": lbar, "argmax": first_max(logits), "dissum": -logits.sum(1), "dbar": None}
        if bars:
            out["dbar"] = (K - 1) * EPS32 * np.abs(logits).sum(1) + lbar.sum(1)
    return out


def upsample_head(e, P, H, W, exact):
    """e[B, h, w, C] low-resolution embedding -> (features f[B, H, W, C], their bar or None, head_fwd of them)"""
    _, h, w, _ = np.shape(e)
    f = PC.bilinear_fwd(e, H, W)
    Df = None if exact else PC.bilinear_bar(e, h, w, H, W, False)
    return f, Df, head_fwd(f, P, Df, bars=not exact)


def head_bwd(g, f, P, gf=None, bars=True):
    """g[B, K, H, W], f[B, H, W, C], P[K, C], gf[B, H, W, C] or None -> (df[B, H, W, C] = -2 sum_k g_k (f - P_k) (+ gf), bar)"""
    g, f, P = np.asarray(g, F64).transpose(0, 2, 3, 1), np.asarray(f, F64), np.asarray(P, F64)
    K = P.shape[0]
    df = -2.0 * (g.sum(-1, keepdims=True) * f - g @ P)
    bar = None
    if bars:
        AM = np.abs(g).sum(-1, keepdims=True) * np.abs(f) + np.abs(g) @ np.abs(P)
        bar = 2 * (K + 1) * EPS32 * AM * SECOND
    if gf is not None:
        df = df + np.asarray(gf, F64)
        if bars:
            bar = bar + EPS32 * (2 * AM + np.abs(np.asarray(gf, F64))) * SECOND
    return df, bar


def nhwc_dist(e, P, K, bars=True):
    """e[M, Kp], P[K, Kp] (pad channels zero in both) -> (out[M, Kp]: -sum_c (e - P_k)^2 for k < K and exactly 0 for K <= k < Kp, bar)"""
    e, P = np.asarray(e, F64), np.asarray(P, F64)
    M, Kp = e.shape
    out, bar = np.zeros((M, Kp)), np.zeros((M, Kp))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            t = e - P[k]
            d = (t * t).sum(-1)
            out[:, k] = -d
            bar[:, k] = (Kp + 3) * EPS32 * d
    return out, (bar if bars else None)


# ---------------------------------------------------------------------------------------------------------------------
# comparisons (the GPU tests and the mutants of tests/test_head_refs.py go through the same three functions)
# ---------------------------------------------------------------------------------------------------------------------
def check_close(what, got, ref, bar, exact):
    """exact: got == ref everywhere (NaN equal to NaN).  Otherwise |got - ref| <= bar where ref is finite, and the same inf / a NaN where
    it is not.  Raises AssertionError; returns (largest error, its bar) of the element that takes the largest share of its bar."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    if exact:
        ok = PC.same(got, ref)
        assert ok.all(), "%s: %d of %d elements differ from the exact value, the first at %s" % (
            what, int((~ok).sum()), ok.size, np.unravel_index(int(np.argmin(ok)), ok.shape))
        return 0.0, 0.0
    bar = np.broadcast_to(np.asarray(bar, F64), ref.shape)
    fin = np.isfinite(ref)
    ok = PC.same(got, ref) | fin
    assert ok.all(), "%s: %d non-finite values were not propagated" % (what, int((~ok).sum()))
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        lim = np.where(fin, bar, 0.0)
    assert np.isfinite(err).all(), "%s: %d non-finite values where the definition is finite" % (what, int((~np.isfinite(err)).sum()))
    share = np.where(err > lim, np.inf, err / np.maximum(lim, 1e-300))
    k = int(np.argmax(share)) if share.size else 0
    assert (err <= lim).all(), "%s: error %.3e above the bar %.3e, %d elements above theirs" % (
        what, err.flat[k], lim.flat[k], int((err > lim).sum()))
    return (float(err.flat[k]), float(lim.flat[k])) if share.size else (0.0, 0.0)


def argmax_excused(logits, lbar):
    """[B, H, W] bool: pixels whose float64 margin between the top two logits does not exceed the sum of their two bars.  Pixels with a
    logit that is not finite are never excused: there the first maximum of the definition is demanded."""
    lg = np.asarray(logits, F64)
    K = lg.shape[1]
    if K == 1:
        return np.zeros(lg[:, 0].shape, bool)
    fin = np.isfinite(lg).all(1)
    L = np.where(np.isnan(lg), -np.inf, lg)
    a1 = np.argmax(L, 1)
    top1 = np.take_along_axis(L, a1[:, None], 1)[:, 0]
    L2 = L.copy()
    np.put_along_axis(L2, a1[:, None], -np.inf, 1)
    a2 = np.argmax(L2, 1)
    top2 = np.take_along_axis(L2, a2[:, None], 1)[:, 0]
    b1 = np.take_along_axis(lbar, a1[:, None], 1)[:, 0]
    b2 = np.take_along_axis(lbar, a2[:, None], 1)[:, 0]
    with np.errstate(invalid="ignore"):
        return fin & ~(top1 - top2 > b1 + b2)


def check_argmax(what, got, ref, exact):
    """got[B, H, W] against ref = head_fwd(...): the first maximum; on real data a near-tie may name any class within the bars of the
    maximum.  Returns the excused share."""
    got = np.asarray(got).astype(np.int64)
    want = ref["argmax"].astype(np.int64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    K = ref["logits"].shape[1]
    assert ((got >= 0) & (got < K)).all(), "%s: a class index outside [0, %d)" % (what, K)
    if exact:
        bad = got != want
        assert not bad.any(), "%s: %d of %d pixels are not the first maximum, the first at %s (%d, expected %d)" % (
            what, int(bad.sum()), bad.size, np.unravel_index(int(np.argmax(bad)), bad.shape), got.flat[int(np.argmax(bad))], want.flat[int(np.argmax(bad))])
        return 0.0
    exc = argmax_excused(ref["logits"], ref["lbar"])
    share = float(exc.mean())
    assert share <= ARGMAX_EXCUSED_CAP, "%s: %.2e of the pixels are near-ties" % (what, share)
    bad = (got != want) & ~exc
    assert not bad.any(), "%s: %d pixels with a clear margin are not the first maximum" % (what, int(bad.sum()))
    lg, lb = ref["logits"], ref["lbar"]
    with np.errstate(invalid="ignore"):
        mine = np.take_along_axis(lg, got[:, None], 1)[:, 0] + np.take_along_axis(lb, got[:, None], 1)[:, 0]
        best = np.take_along_axis(lg, want[:, None], 1)[:, 0] - np.take_along_axis(lb, want[:, None], 1)[:, 0]
        bad = exc & ~(mine >= best)
    assert not bad.any(), "%s: %d near-tie pixels name a class outside the bars of the maximum" % (what, int(bad.sum()))
    return share


def check_propagation(what, got, ref, f, Df, must, may):
    """the upsampled head on an embedding with an inf and a NaN: got against ref / f / Df of the CLEAN embedding.  must[B, H, W]: every
    logit, the dissum and a feature are non-finite and the argmax, with no logit above -inf, is 0; outside may[B, H, W]: logits,
    features and dissum inside the usual bars"""
    keep = ~may
    assert must.any() and keep.any() and not (must & keep).any()
    lg = np.asarray(got["logits"], F64).transpose(0, 2, 3, 1)
    assert (~np.isfinite(lg[must])).all(), what + ": a logit of a pixel that interpolates inf / NaN is finite"
    assert (~np.isfinite(np.asarray(got["feats"], F64)[must])).any(-1).all(), what + ": inf / NaN did not reach the features"
    seen = {"logits": check_close(what + " logits", lg[keep], ref["logits"].transpose(0, 2, 3, 1)[keep], ref["lbar"].transpose(0, 2, 3, 1)[keep], False),
            "feats": check_close(what + " feats", np.asarray(got["feats"])[keep], f[keep], Df[keep], False)}
    if got.get("argmax") is not None:
        assert (np.asarray(got["argmax"])[must] == 0).all(), what + ": the argmax of a pixel without a logit above -inf is not 0"
    if got.get("dissum") is not None:
        assert (~np.isfinite(np.asarray(got["dissum"], F64)[must])).all(), what + ": the dissum of a pixel that interpolates inf / NaN is finite"
        seen["dissum"] = check_close(what + " dissum", np.asarray(got["dissum"])[keep], ref["dissum"][keep], ref["dbar"][keep], False)
    return seen


def check_head(what, got, ref, f, Df, exact):
    """got: dict with any of logits / feats / argmax / dissum (a missing or None entry is not checked) against ref = head_fwd(f, ...).
    Returns {name: (error, bar)} of what was compared."""
    seen = {}
    if got.get("logits") is not None:
        seen["logits"] = check_close(what + " logits", got["logits"], ref["logits"], ref["lbar"], exact)
    if got.get("feats") is not None:
        seen["feats"] = check_close(what + " feats", got["feats"], f, 0.0 if Df is None else Df, exact or Df is None)
    if got.get("dissum") is not None:
        seen["dissum"] = check_close(what + " dissum", got["dissum"], ref["dissum"], ref["dbar"], exact)
    if got.get("argmax") is not None:
        seen["argmax"] = (check_argmax(what + " argmax", got["argmax"], ref, exact), ARGMAX_EXCUSED_CAP)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return (9000 + sum(p * int(n) for p, n in zip((1, 3, 17, 5, 29, 101, 211, 13), parts))) % (2 ** 31 - 1)


def protos(pkind, K, C, seed=0):
    """float32 P[K, C]: "real" 3 I + 0.05 N; "eye" 3 I; "int" integers in [-2, 2]; "dup" the same with row K - 1 a copy of row K // 3"""
    rs = np.random.RandomState(_seed(K, C, PROTO_KINDS.index(pkind) if pkind in PROTO_KINDS else 7, seed))
    eye = 3.0 * np.eye(K, C)
    if pkind == "real":
        return (eye + 0.05 * rs.standard_normal((K, C))).astype(F32)
    if pkind == "eye":
        return eye.astype(F32)
    P = rs.randint(-2, 3, (K, C)).astype(F32)
    if pkind == "dup" and K >= 2:
        P[K - 1] = P[K // 3]
    return P


def tie_pixel(pkind, P):
    """a feature vector that ties two prototypes: the duplicated row, or (1, 1, 0, ...) between rows 0 and 1 of 3 I; None without one"""
    K, C = P.shape
    if pkind == "dup" and K >= 2:
        return P[K // 3].copy()
    if pkind == "eye" and K >= 2 and C >= 2:
        v = np.zeros(C, F32)
        v[:2] = 1.0
        return v
    return None


def features(kind, shape, P, pkind, special=False, seed=0):
    """float32 f[B, H, W, C] (for the upsampled head: the low-resolution embedding).  exact: integers in [-2, 2], pixel 0 a tie.  real:
    1.5 N; pixel 0 equals prototype min(1, K - 1); with three pixels or more the middle one is multiplied by 1e3; special (six
    pixels or more): channel 0 of the last pixel is inf, the last channel of the one before it NaN, channel 0 of pixel 1 is -0.0.
    The upsampled head's embeddings are large but not special: a zero weight times inf is a NaN wherever a kernel multiplies a tap it
    does not need, which the contract leaves open (UP_SPECIAL has those cases)."""
    rs = np.random.RandomState(_seed(*shape, 1 if kind == "real" else 0, seed))
    C = shape[-1]
    n = int(np.prod(shape[:-1]))
    if kind == "exact":
        f = rs.randint(-2, 3, (n, C)).astype(F32)
        t = tie_pixel(pkind, P)
        if t is not None:
            f[0] = t
        return f.reshape(shape)
    f = (1.5 * rs.standard_normal((n, C))).astype(F32)
    f[0] = P[min(1, P.shape[0] - 1)]
    if n >= 3:
        f[n // 2] *= F32(1e3)
    if special and n >= 6:
        f[n - 1, 0] = np.inf
        f[n - 2, C - 1] = np.nan
        f[1, 0] = -0.0
    return f.reshape(shape)


REDRAWS = 32


def plain_input(kind, pkind, case, special=True):
    """(f[B, H, W, C], P) of a dml_proto_dist_fwd case (B, H, W, C, K).  A real sample is redrawn until the float64 reference alone has
    at most ARGMAX_EXCUSED_CAP near-ties (at these sizes: none)"""
    B, H, W, C, K = case
    P = protos(pkind, K, C)
    for seed in range(REDRAWS):
        f = features(kind, (B, H, W, C), P, pkind, special=special, seed=seed)
        if kind == "exact":
            return f, P
        ref = head_fwd(f, P)
        if argmax_excused(ref["logits"], ref["lbar"]).mean() <= ARGMAX_EXCUSED_CAP:
            return f, P
    raise AssertionError("no sample of %s without near-ties" % (case,))


def upsample_kinds(case):
    """the input kinds a dml_upsample_dist_fwd case runs with: exact ones only where the resize is exact"""
    return ("exact", "real") if dyadic(*case[1:5]) else ("real",)


def upsample_input(kind, pkind, case):
    """(e[B, h, w, C], P) of a dml_upsample_dist_fwd case; a real sample is redrawn as in plain_input"""
    B, h, w, H, W, C, K = case[:7]
    P = protos(pkind, K, C)
    for seed in range(REDRAWS):
        e = features(kind, (B, h, w, C), P, pkind, seed=seed)
        if kind == "exact":
            return e, P
        ref = upsample_head(e, P, H, W, False)[2]
        if argmax_excused(ref["logits"], ref["lbar"]).mean() <= ARGMAX_EXCUSED_CAP:
            return e, P
    raise AssertionError("no sample of %s without near-ties" % (case,))


def upsample_special(case):
    """(the embedding with one inf and one NaN in interior pixels, the clean embedding, P, must[B, H, W], may[B, H, W]): must -- a tap of
    non-zero weight is not finite; may -- one of the source pixels in rows y0, y1 and columns x0 - 1 .. x1 + 1 is not (the staged x4
    kernel blends three columns per lane, with weight zero for the one a pixel does not need)"""
    B, h, w, H, W, C, K = case[:7]
    e, P = upsample_input("real", "real", case)
    bad = e.copy()
    bad[0, h // 2, w // 2, 0] = np.inf
    bad[B - 1, h // 2, w // 2, C - 1] = np.nan
    src = ~np.isfinite(bad).all(-1)
    y0, y1, ly0, ly1, _ = PC.src_index(H, h)
    x0, x1, lx0, lx1, _ = PC.src_index(W, w)
    must, may = np.zeros((B, H, W), bool), np.zeros((B, H, W), bool)
    for yi, ly in ((y0, ly0), (y1, ly1)):
        for xi, lx in ((x0, lx0), (x1, lx1)):
            must |= src[:, yi][:, :, xi] & (ly[None, :, None] > 0) & (lx[None, None, :] > 0)
        for xi in (np.maximum(x0 - 1, 0), x0, x1, np.minimum(x1 + 1, w - 1)):
            may |= src[:, yi][:, :, xi]
    return bad, e, P, must, may


def gradients(kind, B, K, H, W, C, P, seed=0):
    """float32 (g[B, K, H, W], f[B, H, W, C], gf[B, H, W, C]).  Pixel 1 (where there is one) has every g_k = 0; in real inputs channel 0 of
    the last pixel holds the float32 nearest to gm_0 / gs, so that gs f and gm cancel there"""
    rs = np.random.RandomState(_seed(B, K, H, W, C, 1 if kind == "real" else 0, seed, 5))
    n = B * H * W
    if kind == "exact":
        gp, f, gf = (rs.randint(-2, 3, s).astype(F32) for s in ((n, K), (n, C), (n, C)))
    else:
        gp = rs.standard_normal((n, K)).astype(F32)
        f = (1.5 * rs.standard_normal((n, C))).astype(F32)
        gf = rs.standard_normal((n, C)).astype(F32)
    if n >= 2:
        gp[1] = 0.0
    if kind == "real":
        gs = gp[n - 1].astype(F64).sum()
        if gs != 0:
            f[n - 1, 0] = F32((gp[n - 1].astype(F64) * P[:, 0].astype(F64)).sum() / gs)
    g = np.ascontiguousarray(gp.reshape(B, H, W, K).transpose(0, 3, 1, 2))
    return g, f.reshape(B, H, W, C), gf.reshape(B, H, W, C)


def nhwc_inputs(kind, M, K, Kp, pkind, seed=0):
    """float32 (e[M, Kp], P[K, Kp]): K carried channels, pad channels zero in both"""
    P = np.zeros((K, Kp), F32)
    P[:, :K] = protos(pkind, K, K, seed)
    e = np.zeros((M, Kp), F32)
    e[:, :K] = features(kind, (M, K), P[:, :K], pkind, special=True, seed=seed)
    return e, P


# ---------------------------------------------------------------------------------------------------------------------
# dispatch: which kernel an entry point of head.hip / pool_resize.hip launches
# ---------------------------------------------------------------------------------------------------------------------
INSTANTIATIONS = ("fwd_c16", "fwd<4,16>", "fwd<4,32>", "fwd<1,16>", "fwd<1,32>",
                  "up_x4", "up_c16", "up<4,16>", "up<4,32>", "up<1,16>", "up<1,32>",
                  "bwd_c16", "bwd<4,16>", "bwd<4,32>", "bwd<1,16>", "bwd<1,32>", "nhwc")
assert len(INSTANTIATIONS) == 5 + 6 + 5 + 1   # forward, upsample, backward, NHWC


def dispatch(entry, C=0, K=0, H=0, W=0, h=0, w=0, argmax=False, dissum=False):
    """the kernel instantiation dml_<entry> launches for these arguments (head.hip's entry points, condition by condition)"""
    cm = 16 if C <= 16 else 32
    if entry == "nhwc":
        return "nhwc"
    if entry in ("fwd", "bwd"):
        if (H * W) % 4 == 0 and C == 16 and K == 16:
            return entry + "_c16"
        return "%s<%d,%d>" % (entry, 4 if (H * W) % 4 == 0 else 1, cm)
    assert entry == "up"
    plain = C == 16 and K == 16 and not argmax and not dissum
    if plain and H == 4 * h and W == 4 * w:
        return "up_x4"
    if plain and W % 4 == 0:
        return "up_c16"
    return "up<%d,%d>" % (4 if W % 4 == 0 else 1, cm)


def items(entry, B, H, W):
    """work items of the generic kernels' grid-stride loop"""
    if entry == "up":
        return B * H * (W // 4) if W % 4 == 0 else B * H * W
    return B * H * W // 4 if (H * W) % 4 == 0 else B * H * W


def dyadic(h, w, H, W):
    """both axes x4, x2, x1 or x1/2"""
    return all(o in (4 * i, 2 * i, i) or 2 * o == i for o, i in ((H, h), (W, w)))


# ---------------------------------------------------------------------------------------------------------------------
# case tables: the smallest shapes that reach every instantiation and every tail
# ---------------------------------------------------------------------------------------------------------------------
# dml_proto_dist_fwd / dml_proto_dist_bwd, C = K = 16, H W % 4 == 0: one 4-pixel group per lane, 64 per wave, 256 per workgroup.
# (B, H, W): one group; 15 groups, one wave over three images; 63, 64, 65 groups; 257 (a second workgroup with one lane); 514 over two
C16_SHAPES = [(1, 1, 4), (3, 1, 20), (1, 4, 63), (1, 16, 16), (1, 4, 65), (1, 4, 257), (2, 2, 514)]
NULL_SHAPE = (3, 1, 20)                        # every combination of NULL and non-NULL logits / feats / argmax / dissum
NULL_COMBOS = list(itertools.product((True, False), repeat=4))
# (C, K) of the generic kernels: C in {1, 3, 4, 13, 16} (CM = 16) and {17, 20, 24, 32} (CM = 32), K in {1, 2, 16, 17, 33} and the class
# counts 3, 5, 13, 21
PAIRS = [(1, 1), (3, 2), (4, 16), (13, 17), (16, 5), (16, 33), (17, 1), (20, 16), (32, 33), (24, 21), (5, 3), (16, 13)]
# four pixels per item: 3 groups per image and a wave over both images; 65 groups; 257
PX4_SHAPES = [(2, 3, 4), (1, 4, 65), (1, 2, 514)]
# one pixel per item: H W in {1, 3, 35}; 259 pixels (a second workgroup)
PX1_SHAPES = [(2, 1, 1), (2, 1, 3), (2, 5, 7), (1, 7, 37)]
# above grid_for's cap of 4096 workgroups: (B, H, W, C, K)
BIG_PX1 = (1, 1025, 1025, 4, 2)                # 1 050 625 pixels
BIG_PX4 = (1, 2052, 2048, 4, 2)                # 1 050 624 four-pixel groups

# dml_upsample_dist_fwd: (h, w, H, W), B = 2
UP_B = 2
UP_X4 = [(h, w, 4 * h, 4 * w) for h, w in ((1, 1), (3, 5), (2, 64), (2, 65))]      # W = 256: one whole segment; 260: a second one of one lane
UP_C16 = [(3, 5, 7, 12), (6, 10, 3, 4), (4, 4, 4, 4), (3, 4, 6, 8)]
# the generic four-pixel kernel: (C, K, argmax, dissum) -- another K, another C (24: CM = 32; 5: scalar taps), or C = K = 16 with a map
UP_PX4_WAYS = [(16, 13, True, True), (16, 21, True, True), (24, 13, True, True), (24, 21, True, True), (5, 3, True, True),
               (16, 16, True, False), (16, 16, False, True)]
UP_PX4_GEOMS = [(3, 5, 12, 20), (3, 5, 7, 12), (3, 4, 6, 8), (6, 10, 3, 4)]
UP_PX1_WAYS = [(16, 13, True, True), (24, 21, True, True), (5, 3, True, True), (16, 16, False, False), (16, 16, True, True)]
UP_PX1_GEOMS = [(3, 5, 7, 9), (1, 1, 3, 3), (5, 7, 5, 7)]
# one inf and one NaN in the embedding, on dyadic geometries (the float32 taps are the float64 ones): staged, gathered, generic
UP_SPECIAL = [(UP_B, 3, 5, 12, 20, 16, 16, False, False), (UP_B, 4, 4, 4, 4, 16, 16, False, False), (UP_B, 3, 4, 6, 8, 16, 16, False, False),
              (UP_B, 3, 5, 12, 20, 16, 13, True, True), (UP_B, 3, 5, 12, 20, 5, 3, True, True), (UP_B, 5, 7, 5, 7, 16, 13, True, True),
              (UP_B, 5, 7, 5, 7, 24, 21, True, True)]
UP_BIG_PX4 = (1, 1026, 1024, 2052, 2048, 4, 2)  # B, h, w, H, W, C, K: x2, 1 050 624 four-pixel groups
UP_BIG_PX1 = (1, 1025, 1025, 1025, 1025, 4, 2)  # x1, 1 050 625 pixels

# dml_proto_dist_nhwc
NHWC_M = (1, 255, 256, 257)
NHWC_KKP = [(1, 1), (13, 16), (16, 16), (21, 24), (32, 32)]
NHWC_BIG = (CAP_2048 + 300, 2, 4)              # M, K, Kp


def nhwc_pitches(Kp):
    """(lde, ldo): dense, and both above Kp"""
    return [(Kp, Kp), (Kp + 3, Kp + 5)]


def plain_cases():
    """(B, H, W, C, K) of dml_proto_dist_fwd and dml_proto_dist_bwd, the above-the-cap ones last"""
    out = [(B, H, W, 16, 16) for (B, H, W) in C16_SHAPES]
    out += [(B, H, W, C, K) for (C, K) in PAIRS for (B, H, W) in PX4_SHAPES + PX1_SHAPES]
    out += [(B, H, W, 16, 16) for (B, H, W) in PX1_SHAPES]                     # C = K = 16 without the fast path
    return out + [BIG_PX1, BIG_PX4]


def upsample_cases():
    """(B, h, w, H, W, C, K, argmax, dissum) of dml_upsample_dist_fwd, the above-the-cap ones last"""
    out = [(UP_B,) + g + (16, 16, False, False) for g in UP_X4 + UP_C16]
    out += [(UP_B,) + g + way for way in UP_PX4_WAYS for g in UP_PX4_GEOMS]
    out += [(UP_B,) + g + way for way in UP_PX1_WAYS for g in UP_PX1_GEOMS]
    return out + [UP_BIG_PX4 + (True, True), UP_BIG_PX1 + (True, True)]


def covered():
    """every instantiation the case tables reach"""
    hit = set()
    for B, H, W, C, K in plain_cases():
        hit.add(dispatch("fwd", C, K, H, W))
        hit.add(dispatch("bwd", C, K, H, W))
    for B, h, w, H, W, C, K, am, ds in upsample_cases():
        hit.add(dispatch("up", C, K, H, W, h, w, am, ds))
    hit.add(dispatch("nhwc"))
    return hit
