"""Case table shared by tests/test_ecdf_refs.py (CPU) and tests/test_gpu_ecdf_score.py (GPU): the numpy definitions of the
per-class ECDF certainty score (dml_ecdf_collect / dml_ecdf_table / dml_ecdf_score; `--ood ecdf`; the recipe kept commented at
DeepLabV3Plus-Pytorch/main_embedding.py:106-113,172-226,249-260 and test_embedding.py:155-163,361-364 of the reference), the seeded
inputs and the error bars.  A plain module in the style of tests/mix_cases.py (no fixtures, no hooks); nothing here looks at a
kernel's output.

What is bitwise defined (include/dmlnet_hip.h), restated below in numpy.float32 so that integer and bit comparisons are possible:
    s(p)   = -(((L_kfirst + L_kfirst+1) + ...) + L_K-1) + 0.0      one float32 rounding per addition, ascending k     dist_sum32
    inv_w  = float32(NB) / float32(clip)
    bin(s) = NB - 1 where s >= clip; 0 where s <= 0; else min(int(float32(s * inv_w)), NB - 1); none for NaN (-1 here)   bin32
    pred   = the first maximal class of the range                                                                        pred_first
    hist[label - k_first][bin(s)] += 1 where k_first <= label < K, label - k_first == pred, s not NaN                     collect_ref
    E_cl[b] = float32(float64(hist[cl][0] + ... + hist[cl][b]) / float64(n_cl)); 1 everywhere for n_cl = 0                ecdf32
    table, mode 0: E > cut ? 1 : E;  mode 2: E;  an empty class: 1;  padding columns: 0                                   table_ref

The two bars, by first-order propagation through the operations the kernels perform; u = EPS32 = 2^-24 is float32's unit
roundoff, so one rounding is a relative error of at most u and "2 ulp" of expf at most 4 u.

  Sigmoid table (mode 1), g = 1 / (1 + exp(-a)), a = slope (E - E_thr) on the bitwise-defined float32 E and E_thr:
    the subtraction and the product round once each, relative to themselves: |da| <= 2 |a| u; expf adds 4 u: the exponential
    carries a relative error of (2 |a| + 4) u, and dg / d(log exp) = -g (1 - g); the addition 1 + exp and the division round once
    each on g: 2 g u.  Below float32's smallest normal number 2^-126 a rounding is absolute, not relative (an exp that overflows
    gives exactly 0 where float64 has 1e-39): that term is added.
        table_bar = 2 x [ g (1 - g) (2 |a| + 4) + 2 g ] u + 2^-126

  Score, conf = (sum_k e_k t_k) / (sum_k e_k), e_k = expf(L_k - max L), t_k = table[bin][k] in [0, 1], Kn terms.  The bin is
  bitwise defined, so the reference looks up the same row and no pixel is "near an edge".
    Each softmax weight w_k = e_k / den: the argument a_k = L_k - max rounds once (|a_k| u absolute on a_k, the same relative on
    e_k) and expf adds 4 u: a relative error d_k <= (|a_k| + 4) u on e_k.  To first order conf moves by sum_k w_k d_k (t_k - conf),
    and |t_k - conf| <= 1: at most sum_k w_k (|a_k| + 4) u.  The largest term is exp(0) = 1 exactly, so den >= 1 and
    w_k |a_k| <= |a_k| exp(a_k) <= 1 / e for each of the other Kn - 1 classes:  ((Kn - 1) / e + 4) u.
    The Kn-term dot product with table values in [0, 1] (products and additions, or fused multiply-adds in their place) carries a
    relative error of at most Kn u on num <= den, the denominator's Kn - 1 additions (Kn - 1) u, the division u: at most 2 Kn u
    relative on conf <= 1.  Both are independent of the inputs:
        score_bar(Kn) = 2 x [ (Kn - 1) / e + 4 + 2 Kn ] u
The factor 2 on each is the slack added.  Looking up a neighbouring bin's row moves a pixel by up to the ECDF's step there, and
swapping two classes' columns by up to 1: millions of bars.

Inputs: tests/mix_cases.dist_logits (negative squared distances of random features to prototypes, mean distance sum 0.85 clip,
every third pixel pushed onto a prototype), so that the bins are spread over [0, clip] and the clip bites; labels that equal the
prediction on about 60 % of the pixels, a random class on 30 %, and 255, -1, K, K + 3 and 0 on the rest.
"""
import numpy as np

import mix_cases as MC
import open_set_cases as OC

EPS32 = OC.EPS32
F32 = np.float32
MAX_CLASSES, MAX_BINS, MAX_CELLS = 32, 2048, 32768        # csrc/ecdf_score.hip: ECDF_MAX_CLASSES / ECDF_MAX_BINS / ECDF_MAX_CELLS
THREADS, MAX_BLOCKS = 1024, 512                           # csrc/ecdf_score.hip: ECDF_THREADS / ECDF_MAX_BLOCKS (dmlnet/_lib.py)
REG_CLASSES = 16                                          # csrc/ecdf_score.hip: ECDF_KREG (the score also has a 20-class form)
KNS = (1, 2, 13, 16, 19, 23, 32)       # 23: above the score's register forms and no multiple of 4, the re-reading form's tail
CLIPS = (400.0, 1000.0)
MODES = {"hard": 0, "sigmoid": 1, "ecdf": 2}
SHAPES = MC.SHAPES


# ---------------------------------------------------------------------------------------------------------------------
# the bitwise definitions
# ---------------------------------------------------------------------------------------------------------------------
def dist_sum32(lg, k_first=0):
    """float32 [B, H, W]: the distance sum of float32 logits [B, K, H, W] in the kernel's order"""
    assert lg.dtype == np.float32
    s = np.zeros((lg.shape[0],) + lg.shape[2:], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(k_first, lg.shape[1]):
            s = s + lg[:, k]
            assert s.dtype == np.float32
        return -s + F32(0.0)


def bin32(s, clip, NB):
    """int64 like s: the bin of float32 distance sums, -1 for NaN"""
    s = np.asarray(s, F32)
    inv_w = F32(NB) / F32(clip)
    assert inv_w.dtype == np.float32
    inside = (s > 0) & (s < F32(clip))
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.where(inside, s, F32(0.0)) * inv_w
    assert prod.dtype == np.float32
    b = np.minimum(prod.astype(np.int64), NB - 1)         # truncation: the values are positive
    b = np.where(s >= F32(clip), NB - 1, b)
    b = np.where(s <= 0, 0, b)
    return np.where(np.isnan(s), -1, b)


def pred_first(lg, k_first=0):
    """int64 [B, H, W], counted from k_first: the first maximal class (`>` against the running best, as the kernels)"""
    best = np.array(lg[:, k_first])
    bi = np.zeros(best.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(k_first + 1, lg.shape[1]):
            up = lg[:, k] > best
            best = np.where(up, lg[:, k], best)
            bi = np.where(up, k - k_first, bi)
    return bi


def collect_ref(lg, labels, k_first, clip, NB, hist=None):
    """int64 [Kn, NB]: dml_ecdf_collect's definition, added onto `hist` when given"""
    K = lg.shape[1]
    out = np.zeros((K - k_first, NB), np.int64) if hist is None else np.array(hist, dtype=np.int64)
    s = dist_sum32(lg, k_first)
    b = bin32(s, clip, NB)
    lab = np.asarray(labels, np.int64).reshape(s.shape)
    ok = (lab >= k_first) & (lab < K) & (lab - k_first == pred_first(lg, k_first)) & (b >= 0)
    np.add.at(out, (lab[ok] - k_first, b[ok]), 1)
    return out


def ecdf32(hist):
    """float32 [Kn, NB]: the binned ECDF of every class, 1 everywhere for an empty class"""
    hist = np.asarray(hist, np.int64)
    cum = np.cumsum(hist, axis=1)
    n = cum[:, -1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        E = (cum.astype(np.float64) / n.astype(np.float64)).astype(F32)
    return np.where(n == 0, F32(1.0), E).astype(F32)


def table_ref(hist, Kp, mode, cut=0.15, slope=50.0, thresholds=None, clip=400.0):
    """(table, bar): float32 [NB, Kp] for the modes 0 and 2 (bitwise, bar 0); float64 and table_bar for mode 1"""
    E = ecdf32(hist)
    Kn, NB = E.shape
    empty = np.asarray(hist).sum(axis=1) == 0
    if mode in (0, 2):
        cert = np.where(E > F32(cut), F32(1.0), E) if mode == 0 else E
        cert = np.where(empty[:, None], F32(1.0), cert).astype(F32)
        out = np.zeros((NB, Kp), F32)
        out[:, :Kn] = cert.T
        return out, np.zeros((NB, Kp))
    tb = bin32(np.asarray(thresholds, F32), clip, NB)
    at = np.where(tb >= 0, E[np.arange(Kn), np.maximum(tb, 0)].astype(np.float64), np.nan)
    a = np.float64(F32(slope)) * (E.astype(np.float64) - at[:, None])
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-a))
    g = np.where(empty[:, None], 1.0, g)
    bar = 2.0 * (g * (1.0 - g) * (2.0 * np.abs(a) + 4.0) + 2.0 * g) * EPS32 + 2.0 ** -126
    out, obar = np.zeros((NB, Kp)), np.zeros((NB, Kp))
    out[:, :Kn], obar[:, :Kn] = g.T, bar.T
    return out, obar


def score_bar(Kn):
    return 2.0 * ((Kn - 1) / np.e + 4.0 + 2.0 * Kn) * EPS32


def score_ref(lg, table, k_first, clip):
    """float64 [B, H, W]: the score of float32 logits against a float32 table [NB, Kp]; NaN where s is NaN (and wherever the
    float64 softmax itself is NaN: an infinite maximum)"""
    NB = table.shape[0]
    Kn = lg.shape[1] - k_first
    b = bin32(dist_sum32(lg, k_first), clip, NB)
    x = lg[:, k_first:].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        rows = table[np.maximum(b, 0)][..., :Kn].astype(np.float64)          # [B, H, W, Kn]
        conf = (e * np.moveaxis(rows, -1, 1)).sum(axis=1) / e.sum(axis=1)
    return np.where(b < 0, np.nan, conf)


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------
def labels_for(lg, k_first, seed):
    """int64 [B, H, W]: the prediction on ~60 % of the pixels, a random class on ~30 %, and 255, -1, K, K + 3, 0 on the rest"""
    K = lg.shape[1]
    rs = np.random.RandomState(seed)
    lab = pred_first(lg, k_first) + k_first
    r = rs.rand(*lab.shape)
    lab = np.where(r > 0.6, rs.randint(0, K, lab.shape), lab)
    odd = np.array([255, -1, K, K + 3, 0], np.int64)
    lab = np.where(r > 0.9, odd[rs.randint(0, odd.size, lab.shape)], lab)
    return lab.astype(np.int64)


def _ccase(shape, Kn, k_first=0, NB=1024, clip=400.0):
    return {"shape": shape, "K": Kn + k_first, "k_first": k_first, "NB": NB, "clip": clip}


def _collect_table():
    c = {}
    for n in (1, 2, 63, 64, 65):                                       # pixels
        c["px%d" % n] = _ccase((1, 1, n), 13)
    # one workgroup pass is THREADS pixels with one pixel per lane and 4 THREADS with four: minus 1, exact, plus 1 (group)
    for n in (THREADS - 1, THREADS, THREADS + 1, 4 * THREADS - 4, 4 * THREADS, 4 * THREADS + 4):
        c["pass%d" % n] = _ccase((1, 1, n), 13, clip=1000.0)
    # workgroups that loop: B = 256 leaves MAX_BLOCKS / 256 = 2 workgroups per image, and each image has three passes
    c["loop_scalar_k2"] = _ccase((256, 1, 2 * THREADS + 3), 2)
    c["loop_vec_k2"] = _ccase((256, 2, 4 * THREADS + 2), 2)
    c["loop_one_image_k2"] = _ccase((1, 1, MAX_BLOCKS * THREADS + 5), 2)    # 513 passes of one image on 512 workgroups
    for Kn in KNS:
        for k_first in (0, 1):
            NB = 2048 if Kn in (13, 16) else 1024                     # 16 x 2048 and 32 x 1024 are the LDS limit itself
            shape = SHAPES["vec"] if (Kn + k_first) % 2 else SHAPES["scalar"]
            c["kn%d_first%d" % (Kn, k_first)] = _ccase(shape, Kn, k_first, NB, 1000.0 if Kn in (2, 19) else 400.0)
    for NB in (1, 2, 1024, 2048):
        for clip in CLIPS:
            c["nb%d_clip%d" % (NB, clip)] = _ccase(SHAPES["batch"], 13, 0, NB, clip)
    c["odd_hw"] = _ccase(SHAPES["odd"], 13, 1, 1024, 400.0)             # H W % 4 != 0
    return c


COLLECT = _collect_table()
OFFSET_CASES = ("kn13_first0", "kn19_first1", "nb1024_clip400")


def collect_inputs(name):
    """(logits float32 [B, K, H, W], labels int64 [B, H, W]) of a COLLECT case"""
    c = COLLECT[name]
    seed = 7100 + sorted(COLLECT).index(name)
    lg = MC.dist_logits(c["K"], c["shape"], c["clip"], c["K"] - c["k_first"], seed)
    return lg, labels_for(lg, c["k_first"], seed + 1)


def edge_sums(clip, NB):
    """float32 distance sums on and around what bin() distinguishes: every power-of-two bin edge and a few others, one ulp
    either side; the clip, one ulp either side; zero, both signs of it, negative values; the infinities and NaN"""
    w = clip / NB                                                      # exact in float32 for the clips and bin counts used here
    edges = sorted({j for j in (1, 2, 3, 5, NB // 3, NB // 2, NB - 2, NB - 1) if 0 < j < NB})
    vals = []
    for j in edges:
        e = F32(j * w)
        vals += [OC.down(e), e, OC.up(e)]
    c = F32(clip)
    vals += [OC.down(c), c, OC.up(c), F32(2.0) * c, F32(0.0), F32(-0.0), F32(1e-30), F32(-1e-30), F32(-3.5), OC.up(F32(0.0)),
             F32(np.inf), F32(-np.inf), F32(np.nan), F32(0.5 * w), F32(clip - 0.5 * w)]
    return np.array(vals, F32)


def edge_inputs(clip, NB):
    """K = 1: the logit is -s exactly, the prediction is class 0 and every label is 0 -> (logits [1, 1, 1, n], labels)"""
    s = edge_sums(clip, NB)
    return (-s).reshape(1, 1, 1, -1), np.zeros((1, 1, s.size), np.int64)


def tie_inputs():
    """K = 4, k_first = 1, six pixels with arg-max ties: the label counts only when it names the FIRST maximal class
    -> (logits, labels, the pixels that count)"""
    lg = np.array([[-5, -1, -1, -9], [-5, -1, -1, -9], [-5, -3, -2, -2], [-5, -3, -2, -2], [0, -4, -4, -4], [0, -4, -4, -4]],
                  F32).T.reshape(1, 4, 1, 6).copy()
    lab = np.array([[[1, 2, 2, 3, 1, 0]]], np.int64)
    return lg, lab, np.array([True, False, True, False, True, False])


def special_logits(K, shape, clip, k_first, seed):
    """a dist_logits frame with a NaN logit (pixel 3), a -inf logit (pixel 4: s = +inf, the last bin), a +inf logit (pixel 5:
    s = -inf, bin 0, and a softmax that is NaN), +inf and -inf together (pixel 6: s NaN) and all mass on one class (pixel 7)"""
    lg = MC.dist_logits(K, shape, clip, K - k_first, seed)
    flat = lg.reshape(lg.shape[0], K, -1)
    flat[:, k_first, 3] = np.nan
    flat[:, K - 1, 4] = -np.inf
    flat[:, K - 1, 5] = np.inf
    flat[:, k_first, 6], flat[:, K - 1, 6] = np.inf, -np.inf
    flat[:, :, 7] = -200.0
    flat[:, K - 1, 7] = 0.0
    return lg


def calib_hist(Kn, NB, seed, empty=(), single=()):
    """int64 [Kn, NB]: a two-bump histogram per class, the classes of `empty` without a sample and those of `single` with one"""
    rs = np.random.RandomState(seed)
    x = (np.arange(NB) + 0.5) / NB
    h = np.zeros((Kn, NB), np.int64)
    for cl in range(Kn):
        m1, m2 = rs.uniform(0.15, 0.4), rs.uniform(0.55, 0.9)
        dens = np.exp(-0.5 * ((x - m1) / 0.04) ** 2) + 0.4 * np.exp(-0.5 * ((x - m2) / 0.12) ** 2)
        h[cl] = rs.poisson(2.0e5 * dens / dens.sum())
    for cl in empty:
        h[cl] = 0
    for cl in single:
        h[cl] = 0
        h[cl, (7 * cl + 3) % NB] = 1
    return h


def random_table(NB, Kn, Kp, seed):
    """float32 [NB, Kp]: a table the score kernel may be given -- monotone certainties in [0, 1] per class, 0 in the padding"""
    rs = np.random.RandomState(seed)
    t = np.zeros((NB, Kp), F32)
    t[:, :Kn] = np.cumsum(rs.rand(NB, Kn) ** 4, axis=0)
    t[:, :Kn] /= t[-1:, :Kn]
    return t.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# score cases
# ---------------------------------------------------------------------------------------------------------------------
def _scase(shape, Kn, k_first=0, NB=1024, clip=400.0, kind="random", mode=0):
    return {"shape": shape, "K": Kn + k_first, "k_first": k_first, "NB": NB, "clip": clip, "kind": kind, "mode": mode}


def _score_table():
    c = {}
    for sname, shape in SHAPES.items():
        c["%s_k13" % sname] = _scase(shape, 13, 0, 2048 if sname == "vec" else 1024, 400.0, "hist")
        c["%s_k19" % sname] = _scase(shape, 19, 0, 1024, 1000.0, "random")
    for Kn in KNS:
        for k_first in (0, 1):
            shape = SHAPES["vec"] if (Kn + k_first) % 2 else SHAPES["scalar"]
            c["kn%d_first%d" % (Kn, k_first)] = _scase(shape, Kn, k_first, 1024, 1000.0 if Kn in (2, 19) else 400.0,
                                                         "hist" if Kn in (13, 16, 32) else "random")
    c["sigmoid_k13"] = _scase(SHAPES["vec"], 13, 1, 1024, 400.0, "hist", mode=1)
    c["ecdf_k13"] = _scase(SHAPES["scalar"], 13, 0, 1024, 400.0, "hist", mode=2)
    c["nb1_k13"] = _scase(SHAPES["batch"], 13, 0, 1, 400.0, "random")
    c["nb2_k17"] = _scase(SHAPES["batch"], 17, 0, 2, 400.0, "random")
    c["special_k13"] = _scase(SHAPES["vec"], 13, 0, 1024, 400.0, "special")
    c["special_k19_first1"] = _scase(SHAPES["batch"], 19, 1, 1024, 1000.0, "special")
    return c


SCORE = _score_table()
SCORE_OFFSET_CASES = ("vec_k13", "vec_k19", "kn16_first1")
_REFS = {}


def score_inputs(name):
    """(logits, table float32 [NB, Kp], conf float64, bar) of a SCORE case; computed once and shared (read-only).  "hist" tables
    are table_ref of a calibration histogram with an empty class (the last) and a one-sample class (the first): mode 0 and 2
    bitwise; for mode 1 the float64 certainties rounded to float32, which is a table like any other to the score kernel."""
    if name not in _REFS:
        c = SCORE[name]
        seed = 7700 + sorted(SCORE).index(name)
        K, k_first, NB, clip = c["K"], c["k_first"], c["NB"], c["clip"]
        Kn, Kp = K - k_first, (K - k_first + 3) // 4 * 4
        if c["kind"] == "special":
            lg = special_logits(K, c["shape"], clip, k_first, seed)
        else:
            lg = MC.dist_logits(K, c["shape"], clip, Kn, seed)
        if c["kind"] == "hist":
            h = calib_hist(Kn, NB, seed + 1, empty=(Kn - 1,) if Kn > 1 else (), single=(0,) if Kn > 2 else ())
            thr = np.linspace(0.2, 0.5, Kn) * clip
            table = table_ref(h, Kp, c["mode"], 0.15, 50.0, thr, clip)[0].astype(F32)
        else:
            table = random_table(NB, Kn, Kp, seed + 1)
        conf = score_ref(lg, table, k_first, clip)
        for arr in (lg, table, conf):
            arr.setflags(write=False)
        _REFS[name] = (lg, table, conf, score_bar(Kn))
    return _REFS[name]
