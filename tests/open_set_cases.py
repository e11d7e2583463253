"""Case table shared by tests/test_open_set_refs.py (CPU) and tests/test_gpu_open_set_scores.py (GPU): seeded inputs,
the float64 definitions the kernels are compared with, and the error bars derived from the arithmetic a kernel is
allowed to do.  A plain module (no fixtures, no hooks); nothing here looks at a kernel's output.

eps32 = 2^-24 and eps64 = 2^-53 are the unit roundoffs.
"""
import numpy as np

EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
FLT_MAX = np.float32(np.finfo(np.float32).max)
MAXC = 32                                     # csrc/common.h: MAXC, embedding dim supported by the head kernels
EXCLUDE_CAP = 1e-3                            # share of pixels whose fp64 decision margin may lie below the fp32 bound


def up(x):
    """next float32 towards +inf"""
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


# ---------------------------------------------------------------------------------------------------------------------
# argmax / max-softmax-probability
# ---------------------------------------------------------------------------------------------------------------------
MSP_KS = (1, 2, 13, 16, 19, 32)
MSP_SHAPES = ((1, 1, 1), (3, 5, 7), (2, 33, 129))
MSP_BIG = (16, (1, 1024, 2048))
MSP_KINDS = ("dist", "ties", "gap", "uniform")


def msp_logits(kind, K, shape, seed=101):
    """float32 [B, K, H, W]; every image of a batch gets its own draw"""
    B, Hh, Ww = shape
    rs = np.random.RandomState(seed + 7 * K + Hh)
    if kind == "dist":                        # negative squared distances of random features to the 3 I prototypes
        f = rs.standard_normal((B, Hh, Ww, K)).astype(np.float32) * np.float32(2.5)
        sq = (f.astype(np.float64) ** 2).sum(-1)
        lg = np.empty((B, K, Hh, Ww), np.float32)
        for k in range(K):                    # |f - 3 e_k|^2 = |f|^2 - 6 f_k + 9
            lg[:, k] = -(sq - 6.0 * f[..., k] + 9.0)
        return lg
    if kind == "ties":                        # small integers: ties everywhere, all classes equal at every third pixel
        lg = rs.randint(-3, 1, (B, K, Hh, Ww)).astype(np.float32)
        flat = lg.reshape(B, K, -1)
        flat[:, :, ::3] = -2.0
        if K > 2:                             # a pairwise tie of the last two classes above everything else
            flat[:, K - 2:, 1::3] = 1.0
        return lg
    if kind == "gap":                         # one class at -1e-3, the others at -1e4: exp underflows, MSP is exactly 0
        lg = np.full((B, K, Hh * Ww), -1e4, np.float32)
        win = rs.randint(0, K, (B, Hh * Ww))
        for b in range(B):
            lg[b, win[b], np.arange(Hh * Ww)] = -1e-3
        return lg.reshape(B, K, Hh, Ww)
    if kind == "uniform":
        return np.full((B, K, Hh, Ww), -7.25, np.float32)
    raise KeyError(kind)


def msp_ref(lg):
    """argmax (first maximal index) and 1 - max softmax, float64 on the float32 inputs"""
    x = lg.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    den = np.exp(x - m).sum(axis=1)
    return np.argmax(lg, axis=1).astype(np.int64), 1.0 - 1.0 / den


def msp_bar(K):
    """den <= K, terms exp(a), a <= 0: rounding of a (|a| e^a <= 1/e), expf (<= 2 ulp), K - 1 additions, one division, one
    subtraction: about (2 K + 4) eps32 absolute on 1 - 1/den; x2 slack"""
    return 2.0 * (2 * K + 4) * EPS32


# ---------------------------------------------------------------------------------------------------------------------
# dissum
# ---------------------------------------------------------------------------------------------------------------------
DISSUM_MODES = ((1000.0, False), (400.0, True))
DISSUM_KS = (1, 13, 16, 19)
DISSUM_HW = (1, 63, 64, 65, 255, 257, 1024 * 2048 + 1)


def dissum_ref(lg_khw, clip, inclusive):
    """float64 of the definition on one image: -sum_k, clipped, min-max normalised (0/0 = NaN for a constant image)"""
    s = -lg_khw.astype(np.float64).sum(axis=0)
    s = np.where((s >= clip) if inclusive else (s > clip), clip, s) + 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s - s.min()) / (s.max() - s.min()), s


def dissum_bar(lg_khw, clip, inclusive):
    """sequential fp32 sum of K terms: |err| <= (K - 1) eps32 sum_k |logit_k| per pixel (clipping is min(s, clip):
    1-Lipschitz); after normalisation 2 max_err / (hi - lo) + 3 eps32; x2 slack.  Returns (bar, max_err)."""
    K = lg_khw.shape[0]
    max_err = float((K - 1) * EPS32 * np.abs(lg_khw.astype(np.float64)).sum(axis=0).max())
    _, s = dissum_ref(lg_khw, clip, inclusive)
    rng = float(s.max() - s.min())
    return (2.0 * (2.0 * max_err / rng + 3.0 * EPS32) if rng > 0 else np.nan), max_err


def dissum_batch(K, seed=202, hw=(17, 31)):
    """B = 3, per-image ranges 1 : 100 : 10000; mixed signs (negative scores next to positive ones) in every image; image 2
    straddles both clips"""
    rs = np.random.RandomState(seed + K)
    g = rs.standard_normal((3, K) + hw)
    return np.stack([0.01 * g[0], g[1], 100.0 * (g[2] - 0.5)]).astype(np.float32)


def dissum_flat(K, hw, seed=303):
    """one image of hw pixels as 1 x hw, scores on both sides of both clips"""
    rs = np.random.RandomState(seed + K + hw % 1000)
    return (rs.standard_normal((1, K, 1, hw)) * (600.0 / K) - 500.0 / K).astype(np.float32)


def dissum_on_clip(K):
    """scores exactly 400 / 1000, one ulp either side, and others around -- from logits that sum exactly in fp32
    (one non-zero logit per pixel, at a different k each)"""
    want = [0.0, 100.0, down(400), 400.0, up(400), 700.0, down(1000), 1000.0, up(1000), 2000.0, -3.0, 4096.0]
    lg = np.zeros((1, K, 1, len(want)), np.float32)
    for i, s in enumerate(want):
        lg[0, i % K, 0, i] = -np.float32(s)
    return lg


def dissum_all_clip_but_one(K, hw=65):
    lg = np.full((1, K, 1, hw), -5000.0 / K, np.float32)
    lg[0, :, 0, 41] = -0.25
    return lg


def dissum_signed_zero(last):
    """K = 4, dyadic positive "logits" (every score negative, exact in fp32) except one pixel whose logits are all +0.0:
    its score -0.0 / +0.0 is the image's maximum.  last=False: 300 pixels, the zero at pixel 5.  last=True: 3079 pixels,
    the zero is the last pixel (last workgroup) and the minimum sits at pixel 0."""
    hw = 3079 if last else 300
    rs = np.random.RandomState(404 + hw)
    lg = (rs.randint(1, 64, (1, 4, 1, hw)) / 4.0).astype(np.float32)
    lg[0, :, 0, 0] = 32.0                     # the minimum score, -128
    lg[0, :, 0, hw - 1 if last else 5] = 0.0
    return lg


# ---------------------------------------------------------------------------------------------------------------------
# novel relabel
# ---------------------------------------------------------------------------------------------------------------------
RELABEL_CS = (1, 16, MAXC)
RELABEL_KS = (1, 16, 19)
RELABEL_LABELS = (16, 19, 255)


def relabel_ref(preds_hw, lg_khw, feats_hwc, proto, thresh, new_label):
    """float64 of the definition; also returns d and the decision margin min(|d - thresh|, |d - max_k logit|)"""
    d = -((feats_hwc.astype(np.float64) - proto.astype(np.float64)) ** 2).sum(axis=-1)
    best = lg_khw.astype(np.float64).max(axis=0)
    out = preds_hw.copy()
    out[(d > np.float64(thresh)) & (d > best)] = new_label
    return out, d, np.minimum(np.abs(d - np.float64(thresh)), np.abs(d - best))


def relabel_err(d, C):
    """fp32 evaluation of -sum_c (f_c - p_c)^2: one rounding in the difference (2 eps32 on the square), one in the
    square, C - 1 additions: (C + 2) eps32 |d|"""
    return (C + 2) * EPS32 * np.abs(d)


def relabel_exact(C, K, new_label):
    """One row of pixels whose d is exact in fp32 (differences 1, 0.5, 0).  Returns feats [2,1,n,C], logits [2,K,1,n],
    proto [C], preds [2,1,n], and per threshold the pixels that must be relabelled.  Image 1 is image 0 reversed, so a
    batch-stride slip cannot pass."""
    proto = (np.arange(C) % 5 - 2).astype(np.float32)
    t125 = np.zeros(C, np.float32)
    t15 = np.zeros(C, np.float32)
    t4 = np.zeros(C, np.float32)
    t4[0] = 2.0
    if C >= 3:
        t125[[0, C - 1]] = (1.0, 0.5)                                   # d = -1.25
        t15[[0, 1, C - 1]] = (1.0, 0.5, 0.5)                             # d = -1.5
        dm, dt = np.float32(-1.25), np.float32(-1.5)
    else:                                                                # C = 1: only squares of one dyadic number
        t125[0], t15[0] = 0.5, 1.0
        dm, dt = np.float32(-0.25), np.float32(-1.0)
    # (difference to the prototype, max logit, prediction before)
    px = [(t15, -10.0, 3), (t125, dm, 3), (t125, down(dm), 3), (t125, -10.0, new_label), (t4, -10.0, 255),
          (t125, up(dm), 3), (np.zeros(C, np.float32), -10.0, 255), (t125, -10.0, 0)]
    n = len(px)
    feats = np.stack([proto + t for t, _, _ in px])[None, None]           # [1,1,n,C]
    lg = np.full((1, K, 1, n), -50.0, np.float32)
    for i, (_, m, _) in enumerate(px):
        lg[0, (K - 1 - i) % K, 0, i] = m                                  # the maximum sits at a different k per pixel
    preds = np.array([p for _, _, p in px], np.int64)[None, None]
    feats = np.concatenate([feats, feats[:, :, ::-1]]).astype(np.float32)
    lg = np.concatenate([lg, lg[:, :, :, ::-1]])
    preds = np.concatenate([preds, preds[:, :, ::-1]])
    # relabelled pixels of image 0 per threshold: d > thresh and d > max logit
    d = np.array([dt, dm, dm, dm, -4.0, dm, 0.0, dm], np.float64)
    expect = {}
    for th in (np.float32(-1.5), np.float32(0.0), dt, down(dt), down(0.0), np.float32(-5.0)):
        expect[float(th)] = [i for i in range(n) if d[i] > np.float64(th) and d[i] > np.float64(px[i][1])]
    return feats, lg, proto, preds, expect


def relabel_random(seed=505, C=16, K=16, shape=(2, 96, 160)):
    rs = np.random.RandomState(seed)
    B, Hh, Ww = shape
    proto = rs.standard_normal(C).astype(np.float32)
    feats = (proto + rs.standard_normal((B, Hh, Ww, C)) * rs.uniform(0.05, 0.6, (B, Hh, Ww, 1))).astype(np.float32)
    lg = (-np.abs(rs.standard_normal((B, K, Hh, Ww))) * 2.0 - 0.3).astype(np.float32)
    preds = rs.randint(0, K, (B, Hh, Ww)).astype(np.int64)
    preds[rs.rand(B, Hh, Ww) < 0.05] = 255
    return feats, lg, proto, preds


# ---------------------------------------------------------------------------------------------------------------------
# confusion matrix
# ---------------------------------------------------------------------------------------------------------------------
CONF_NS = (1, 2, 19, 64)
CONF_COUNTS = (0, 1, 2, 3, 511, 512, 513, 2 * 2048 * 256 + 1)


def confusion_ref(lt, lp, n):
    """bincount over the pixels whose label AND prediction are classes (the kernel drops a prediction outside [0, n)
    where the reference's bincount would leave the n x n shape)"""
    lt, lp = lt.reshape(-1), lp.reshape(-1)
    ok = (lt >= 0) & (lt < n) & (lp >= 0) & (lp < n)
    return np.bincount(n * lt[ok] + lp[ok], minlength=n * n).reshape(n, n).astype(np.int64)


def confusion_inputs(n, count, seed=606):
    rs = np.random.RandomState(seed + n + count % 977)
    lt = rs.randint(0, n, count).astype(np.int64)
    lp = rs.randint(0, n, count).astype(np.int64)
    ign = rs.rand(count)
    for lo, v in ((0.00, 255), (0.05, -1), (0.10, n), (0.15, 2 ** 40)):
        lt[(ign >= lo) & (ign < lo + 0.05)] = v
    bad = rs.rand(count)
    lp[bad < 0.03] = n                         # predictions out of range, both sides
    lp[(bad >= 0.03) & (bad < 0.06)] = -1
    lp[(bad >= 0.06) & (bad < 0.08)] = 2 ** 40 + 1
    return lt, lp


# ---------------------------------------------------------------------------------------------------------------------
# class feature sums
# ---------------------------------------------------------------------------------------------------------------------
FSUM_CS = (1, 7, 16, MAXC)
FSUM_NPX = (1, 255, 257)
FSUM_BIG = 16 * 768 * 768


def fsum_bar(n_px, abs_sum):
    """per-thread fp32 partial of at most ceil(n_px / (1024 * 256)) terms, then fp64: relative to sum |f| of the class;
    x2 slack"""
    return 2.0 * np.ceil(n_px / 262144.0) * EPS32 * abs_sum


def fsum_inputs(C, n_px, seed=707):
    """features 1e3 + N(0, 1) (an fp32-only accumulation would show); labels 0..2, class 3 absent, class 4 only at the last
    pixel"""
    rg = np.random.default_rng(seed + C + n_px % 1013)
    f = rg.standard_normal((n_px, C), dtype=np.float32)
    f += np.float32(1e3)
    lab = rg.integers(0, 3, n_px, dtype=np.int64)
    lab[-1] = 4
    return f, lab


def fsum_ref(f, lab, c):
    sel = f[lab == c].astype(np.float64)
    return sel.sum(axis=0), np.abs(sel).sum(axis=0), int((lab == c).sum())


# ---------------------------------------------------------------------------------------------------------------------
# OOD measures
# ---------------------------------------------------------------------------------------------------------------------
OOD_OUT8 = (13, -7, 2 ** 31 + 5, 250, 0, 99, 2 ** 40, 17)


def _ood_order_values(rs, n):
    pool = [0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, FLT_MAX, -FLT_MAX]
    v = np.array(pool, np.float32)[rs.randint(0, len(pool), n)]
    den = (rs.standard_normal(n) * 1e-42).astype(np.float32)          # subnormal
    pick = rs.rand(n) < 0.4
    v[pick] = den[pick]
    return v


def ood_labelled(seed=808, n=5000):
    """conf, labels from 12 values of which eight are the out-labels"""
    rs = np.random.RandomState(seed)
    values = np.array(OOD_OUT8 + (1, 2, 3, 2 ** 31 + 6), np.int64)
    lab = values[rs.randint(0, len(values), n)]
    conf = (rs.randint(-40, 40, n) / 16.0 - 0.5 * np.isin(lab, OOD_OUT8)).astype(np.float32)
    return conf, lab


def ood_one_each(seed=809, n=10000):
    """a mask that leaves exactly one positive and one negative"""
    rs = np.random.RandomState(seed)
    conf = rs.standard_normal(n).astype(np.float32)
    lab = rs.randint(0, 14, n).astype(np.int64)
    mask = np.zeros(n, bool)
    mask[np.flatnonzero(lab == 13)[3]] = True
    mask[np.flatnonzero(lab != 13)[-2]] = True
    return conf, lab, mask


def ood_big(seed=810):
    """four different 1024 x 2048 maps, clipped (heavy ties), labels 0..13 with 12, 13 out"""
    rs = np.random.RandomState(seed)
    n = 4 * 1024 * 2048
    lab = rs.randint(0, 14, n).astype(np.int64)
    conf = rs.standard_normal(n).astype(np.float32)
    conf += (lab >= 12) * np.float32(0.8)
    conf = np.round(conf * 64) / 64                                   # a normalised / quantised map: ties everywhere
    conf = np.clip(conf, -1.5, 2.0).astype(np.float32)
    for q in range(4):                                                # the four images differ in offset
        conf[q * (n // 4):(q + 1) * (n // 4)] += np.float32(q / 128.0)
    return conf, lab


def _ood_plain_cases():
    """name -> (pos, neg, recall_level), float32 scores of the positive / negative class"""
    rs = np.random.RandomState(909)
    nrm = lambda n, mu=0.0: (rs.standard_normal(n) + mu).astype(np.float32)     # noqa: E731
    c = {}
    for P, N in ((1, 1), (1, 62), (1, 70000), (70000, 1), (32, 32), (33, 32), (535, 65000), (537, 65000)):
        c["pn_%d_%d" % (P, N)] = (nrm(P, 0.7), nrm(N), 0.95)
    c["all_equal"] = (np.full(40, 0.25, np.float32), np.full(60, 0.25, np.float32), 0.95)
    c["two_values"] = ((rs.rand(300) < 0.7).astype(np.float32), (rs.rand(500) < 0.3).astype(np.float32), 0.95)
    c["sep_high"] = (rs.rand(50).astype(np.float32) + 2, rs.rand(90).astype(np.float32), 0.95)
    c["sep_low"] = (rs.rand(50).astype(np.float32) - 2, rs.rand(90).astype(np.float32), 0.95)
    v = _ood_order_values(rs, 2000)
    c["order"] = (v[:800], v[800:], 0.95)
    c["order_zero_only"] = (np.array([0.0, -0.0, 0.0, -0.0], np.float32), np.array([-0.0, 0.0, -0.0], np.float32), 0.95)
    for P in (20, 301):
        pos = (rs.randint(0, 4 * P, P) / 8.0).astype(np.float32)
        neg = (rs.randint(-P, 3 * P, 500) / 8.0).astype(np.float32)
        for r in (0.0, 0.5, 0.95, 1.0):
            c["recall_%d_%g" % (P, r)] = (pos, neg, r)
    return c


def ood_cases(big=True):
    """every case as (pos, neg, recall); the label / mask cases already reduced to their two score sets the way
    eval_ood_measure does it (scores = -conf)"""
    c = _ood_plain_cases()
    conf, lab = ood_labelled()
    out = np.isin(lab, OOD_OUT8)
    c["labels8"] = (-conf[out], -conf[~out], 0.95)
    conf, lab, mask = ood_one_each()
    out = lab[mask] == 13
    c["one_each"] = (-conf[mask][out], -conf[mask][~out], 0.95)
    if big:
        conf, lab = ood_big()
        out = lab >= 12
        c["big4"] = (-conf[out], -conf[~out], 0.95)
    return c


OOD_NAMES = tuple(_ood_plain_cases().keys()) + ("labels8", "one_each", "big4")
OOD_STORE_INPUTS_UP_TO = 5000                 # the fixture also keeps the inputs of the cases up to this many scores


def ood_aupr_bar(pos):
    """identical terms, fp64 sum in another order: P_distinct eps64, and no looser than 1e-11"""
    return min(len(np.unique(np.asarray(pos, np.float64) + 0.0)) * EPS64, 1e-11)
