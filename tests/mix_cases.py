"""Case table shared by tests/test_mix_refs.py (CPU) and tests/test_gpu_mix_score.py (GPU): the float64 definition of the
"EDS + MMSP" anomaly score (dml_dissum_msp_score; `--ood dissum_msp`; anomaly/eval_ood_traditional.py:302-305,434-435,
447-448 and test_embedding.py:366-369 of the reference), its seeded inputs and the per-pixel error bar.  A plain module in the
style of tests/knn_cases.py (no fixtures, no hooks); nothing here looks at a kernel's output.

The definition, per image and pixel p, over the classes k_first <= k < K (Kn = K - k_first of them), every minimum and maximum
over the image alone:
    s(p)    = min(-(sum_k L_k(p)) + 0.0, clip)
    m(p)    = 1 / sum_k exp(L_k(p) - max_k L_k(p))      (prob "softmax")      = max_k L_k(p)      (prob "logit")
    d(p)    = (s(p) - min s) / (max s - min s)           q(p) = (m(p) - min m) / (max m - min m)
    c(p)    = 1 / (1 + exp(slope (d(p) - threshold)))    conf(p) = c(p) d(p) + (1 - c(p)) q(p)
A constant s or m map gives 0/0 = NaN, and then conf is NaN on every pixel of the image (0 * NaN is NaN).

The bar, by first-order propagation through the form the kernel evaluates.
  s: a sequential fp32 sum of Kn terms, |err| <= (Kn - 1) eps32 sum_k |L_k(p)|; the negation, the + 0.0 and the clip
     (1-Lipschitz) add nothing.  E_s is the largest such bound of the image.
  m: the maximum is exact.  The softmax denominator is formed in the two-read form -- the maximum first, then
     sum_k exp(L_k - max) over the plain values, whether they come from registers or from a second read -- with no
     rescaling step: Kn roundings of the argument (|a| e^a <= 1/e each), Kn expf at <= 2 ulp on terms whose sum is <= Kn,
     Kn - 1 additions and the division: (2 Kn + 4) eps32 absolute on m <= 1, as open_set_cases.msp_bar counts it.
     E_m is that for the softmax and 0 for the maximum logit.
  d, q: an error E on every value moves the numerator by 2 E and the denominator by 2 E, and the ratio is <= 1: the
     quotient moves by <= 2 E / range to first order (as open_set_cases.dissum_bar), plus the subtraction, the denominator's
     subtraction and the division:
         e_d = 2 E_s / (max s - min s) + 3 eps32          e_q = 2 E_m / (max m - min m) + 3 eps32
  c: dc/dd = -slope c (1 - c).  The argument slope (d - threshold) carries two roundings relative to itself, expf <= 2 ulp,
     the addition and the division one each: a relative error (|slope (d - threshold)| + 4) eps32 on exp, times c (1 - c).
  conf = q + c (d - q):  dconf/dd = c - (d - q) slope c (1 - c), dconf/dq = 1 - c, dconf/dc = d - q; the two products, the
     1 - c and the sum (or the fused multiply-add in their place) round once each, on values <= 1: 4 eps32.
    bar(p) = 2 x [ (c + |d - q| slope c (1 - c)) e_d + |d - q| c (1 - c) (|slope (d - threshold)| + 4) eps32
                   + (1 - c) e_q + 4 eps32 ]
The factor 2 is slack.  Swapping the two weights moves a pixel by up to 1, thousands of bars.

Inputs: negative squared distances of random K-dimensional features to the prototypes 3 e_k, the features N(0, sigma^2)
with sigma^2 = (0.85 clip - 9 Kn) / Kn^2 (at least 0.04), so that the mean distance sum is 0.85 clip and the clip bites without
swallowing the image.  Every third pixel (flat index % 3 == 1) is pushed towards one prototype (3 e_j + 0.3 N(0, 1)): its
maximum softmax is 1 to rounding and its distance sum is 18 (Kn - 1), roughly.  Pixel 0 of every image has its second largest
component set 0.1 below its largest, the two best classes 0.6 apart in logit and a maximum softmax of at most 0.65, so that even a two-pixel frame of two classes, whose other pixels all have a softmax that is 1
in float32 and in float64, keeps a range of m that is no rounding artefact.
"""
import numpy as np

import open_set_cases as OC

EPS32 = OC.EPS32
MAX_CLASSES = 32                # csrc/common.h: MAXC
REG_CLASSES = 16                # csrc/scores.hip: MIX_KREG, up to which pass 1 keeps the logits in registers
PASS1_GRID = {True: 512, False: 2048}     # csrc/scores.hip: MIX_GRID_REG, MIX_GRID_REREAD -- workgroups per image at most
KS = (2, 13, 16, 19, 32)
PROBS = ("softmax", "logit")
CLIPS = (400.0, 1000.0)
SHAPES = {"px1": (1, 1, 1), "px2": (1, 1, 2), "odd": (1, 3, 5), "batch": (2, 33, 129), "scalar": (1, 70, 131),
          "vec": (1, 40, 132)}
STAT_SHAPES = ("batch", "scalar", "vec")      # enough pixels for the conditions on shares and means
THRESHOLD, SLOPE = 0.2, 50.0


def _case(kind, K, shape, clip, prob, k_first=0, threshold=THRESHOLD, slope=SLOPE):
    return {"kind": kind, "K": K, "shape": shape, "clip": clip, "prob": prob, "k_first": k_first, "threshold": threshold,
            "slope": slope}


def _table():
    c = {}
    for sname, shape in SHAPES.items():
        for K in KS:
            for prob in PROBS:
                for clip in CLIPS:
                    c["%s_k%d_%s_%d" % (sname, K, prob, clip)] = _case("dist", K, shape, clip, prob)
    for prob in PROBS:
        c["zero_row_%s" % prob] = _case("signed_zero", 4, (1, 1, 3079), 400.0, prob)
        # --exclude_back on 14 classes; the DeepLab recipe's threshold on the logit form
        c["kfirst_%s" % prob] = _case("dist", 14, (2, 33, 129), 400.0, prob, k_first=1,
                                      threshold=0.3 if prob == "logit" else THRESHOLD)
        c["kfirst_vec_%s" % prob] = _case("dist", 14, (1, 40, 132), 400.0, prob, k_first=1)
        c["steep_%s" % prob] = _case("dist", 13, (1, 40, 132), 400.0, prob, slope=200.0)
        c["flat_%s" % prob] = _case("dist", 13, (1, 70, 131), 400.0, prob, slope=0.0)
        # NaN on every pixel
        c["all_clipped_%s" % prob] = _case("all_clipped", 13, (1, 3, 5), 400.0, prob)
        c["uniform_%s" % prob] = _case("uniform", 13, (1, 3, 5), 400.0, prob)
    # more pixels than one sweep of pass 1's grid covers (PASS1_GRID workgroups of 256 lanes): the lanes loop
    c["loop_scalar_softmax"] = _case("dist", 2, (1, 363, 363), 400.0, "softmax")      # 131,769 pixels, one per lane
    c["loop_vec_softmax"] = _case("dist", 2, (1, 726, 724), 400.0, "softmax")         # 131,406 groups of four
    c["loop_reread_logit"] = _case("dist", 17, (1, 725, 725), 1000.0, "logit")        # 525,625 pixels, one per lane
    c["one_class_softmax"] = _case("dist", 14, (1, 3, 5), 400.0, "softmax", k_first=13)
    c["k1_softmax"] = _case("dist", 1, (1, 33, 129), 400.0, "softmax")
    return c


CASES = _table()
NAN_CASES = tuple(n for n, c in CASES.items() if n.startswith(("px1_", "all_clipped_", "uniform_"))) + (
    "one_class_softmax", "k1_softmax")
CLIP_CASES = tuple(n for n, c in CASES.items() if c["kind"] == "dist" and n not in NAN_CASES
                   and (n.split("_")[0] in STAT_SHAPES or n.startswith(("kfirst_", "steep_", "flat_", "loop_"))))
OFFSET_CASES = ("vec_k13_softmax_400", "vec_k19_logit_1000", "scalar_k13_softmax_400")


def dist_logits(K, shape, clip, Kn, seed):
    """float32 [B, K, H, W] of the generator described above; sigma is sized for the Kn classes that take part"""
    B, Hh, Ww = shape
    rs = np.random.RandomState(seed)
    sigma = np.sqrt(max((0.85 * clip - 9.0 * Kn) / Kn ** 2, 0.04))
    f = sigma * rs.uniform(0.2, 1.5, (B, Hh * Ww, 1)) * rs.standard_normal((B, Hh * Ww, K))
    pushed = np.arange(Hh * Ww) % 3 == 1
    n_p = int(pushed.sum())
    for b in range(B):
        near = 0.3 * rs.standard_normal((n_p, K))
        near[np.arange(n_p), rs.randint(K - Kn, K, n_p)] += 3.0
        f[b, pushed] = near
    if Kn >= 2:                               # pixel 0: the runner-up class 0.1 below the best one
        for b in range(B):
            order = np.argsort(f[b, 0, K - Kn:]) + K - Kn
            f[b, 0, order[-2]] = f[b, 0, order[-1]] - 0.1
    f = f.astype(np.float32).astype(np.float64)
    sq = (f ** 2).sum(-1)
    lg = np.empty((B, K, Hh * Ww), np.float32)
    for k in range(K):                        # |f - 3 e_k|^2 = |f|^2 - 6 f_k + 9
        lg[:, k] = -(sq - 6.0 * f[..., k] + 9.0)
    return lg.reshape(B, K, Hh, Ww)


def logits(name):
    """the seeded float32 input [B, K, H, W] of a case"""
    c = CASES[name]
    K, (B, Hh, Ww), kind = c["K"], c["shape"], c["kind"]
    seed = 5200 + sorted(CASES).index(name)
    if kind == "dist":
        return dist_logits(K, c["shape"], c["clip"], K - c["k_first"], seed)
    if kind == "signed_zero":
        return OC.dissum_signed_zero(last=True)
    if kind == "all_clipped":
        rs = np.random.RandomState(seed)
        return (-5000.0 / K - rs.rand(B, K, Hh, Ww)).astype(np.float32)
    if kind == "uniform":
        return np.full((B, K, Hh, Ww), -7.25, np.float32)
    raise KeyError(kind)


def score_ref(lg, clip, threshold, slope, prob, k_first=0):
    """float64 of the definition on float32 logits [B, K, H, W] -> dict of [B, H, W] arrays conf, bar, d, q, c, s (raw) and
    the per-image clipped share; NaN (conf and bar) on the images with a constant map"""
    x = lg[:, k_first:].astype(np.float64)
    B, Kn = x.shape[:2]
    s = -x.sum(axis=1) + 0.0
    clipped = s >= clip
    s = np.where(clipped, clip, s)
    best = x.max(axis=1)
    m = best if prob == "logit" else 1.0 / np.exp(x - best[:, None]).sum(axis=1)
    E_s = (Kn - 1) * EPS32 * np.abs(x).sum(axis=1).reshape(B, -1).max(axis=1)
    E_m = 0.0 if prob == "logit" else (2 * Kn + 4) * EPS32
    out = {k: np.empty(s.shape) for k in ("conf", "bar", "d", "q", "c")}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            rs, rm = s[b].max() - s[b].min(), m[b].max() - m[b].min()
            d = (s[b] - s[b].min()) / rs
            q = (m[b] - m[b].min()) / rm
            arg = slope * (d - threshold)
            c = 1.0 / (1.0 + np.exp(arg))
            e_d = 2.0 * E_s[b] / rs + 3.0 * EPS32
            e_q = 2.0 * E_m / rm + 3.0 * EPS32
            gap = np.abs(d - q)
            out["conf"][b] = c * d + (1.0 - c) * q
            out["bar"][b] = 2.0 * ((c + gap * slope * c * (1.0 - c)) * e_d
                                   + gap * c * (1.0 - c) * (np.abs(arg) + 4.0) * EPS32 + (1.0 - c) * e_q + 4.0 * EPS32)
            out["d"][b], out["q"][b], out["c"][b] = d, q, c
    out["s"] = s
    out["clipped"] = clipped
    return out


_REFS = {}


def reference(name):
    """(logits, ref) of a case, ref as score_ref returns it; computed once and shared (callers must not modify it)"""
    if name not in _REFS:
        c = CASES[name]
        lg = logits(name)
        ref = score_ref(lg, c["clip"], c["threshold"], c["slope"], c["prob"], c["k_first"])
        lg.setflags(write=False)
        for arr in ref.values():
            arr.setflags(write=False)
        _REFS[name] = (lg, ref)
    return _REFS[name]
