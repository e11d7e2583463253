"""Case table shared by tests/test_pooled_refs.py (CPU) and tests/test_gpu_pooled_ood.py (GPU): the numpy definition of the pooled
(dataset-level) OOD measures (dml_pooled_ood_update / dml_pooled_ood_finalize, anom_utils.PooledOodMeasures, `--pooled`), the
finalize formulas in Python integers and fractions.Fraction, and the seeded inputs.  A plain module in the style of
tests/ecdf_cases.py (no fixtures, no hooks); nothing here looks at a kernel's output.

What is bitwise defined (include/dmlnet_hip.h), restated in numpy.float32 so that integer comparisons are possible:
    inv_w = float32(NB) / (float32(hi) - float32(lo))
    bin   = NB - 1 where conf >= hi; 0 where conf <= lo; else min(int(float32(float32(conf - lo) * inv_w)), NB - 1); none for NaN    bin32
    state = hist[2][NB] (row 0: label in out_labels) + [n_nan, n_below, n_above, n_masked, n_frames]                                  state_ref
With P_b, N_b the rows, tp_b / fp_b their inclusive prefix sums (a pixel is flagged when its bin <= b), exactly:                      finalize_ref
    AUROC = sum_b P_b (2 (N - fp_b) + N_b) / (2 P N)
    AUPR  = sum_{b: P_b > 0} (P_b / P) tp_b / (tp_b + fp_b)
    T     = sum_b P_b N_b / (P N)                 the tie mass: |AUROC - unquantised AUROC| <= T / 2, binning being monotone
    FPR   = fp / N of the candidate whose recall float64(tp) / float64(P) is nearest the level in float64 (the higher recall on a
            tie): per bin with P_b > 0, taken in descending order, the first (lowest score -bin) with its own fp_b and every other
            with the negatives of the bins strictly below the previous such bin; cut = the candidate's bin
These are oracle/ood_measures_ref.get_measures on the scores -bin; tests/test_pooled_refs.py holds them to it.

The bars.  The kernel's AUROC and T are one correctly rounded 128-bit numerator, two products in the denominator and one division:
4 eps64 relative.  Its AUPR is a float64 sum of terms in [0, 1], each with three roundings (two quotients and a product, 3 eps64
relative, the terms sum to at most 1) plus one rounding per addition of two non-zero values, on a partial sum <= 1.  Summed lane by
lane and then over the lanes, k_i positive bins in lane i and L lanes with any: sum_i (k_i - 1) + (L - 1) = positive bins - 1 such
additions, as in a single chain.  (positive bins + 2) eps64 to first order; the bar is (positive bins + 4) eps64 absolute.
FPR is one division of two exact integers by the same rule on both sides: equal.
"""
from fractions import Fraction

import numpy as np

import open_set_cases as OC

F32 = np.float32
EPS64 = OC.EPS64
MAX_BINS, MAX_OUT, COUNTERS = 8192, 8, 5                  # csrc/pooled_ood.hip: POOLED_MAX_BINS / POOLED_MAX_OUT / POOLED_COUNTERS
SPAN, MAX_BLOCKS = 2048, 256                              # csrc/pooled_ood.hip: POOLED_SPAN / POOLED_MAX_BLOCKS (dmlnet/_lib.py)
NBS = (1, 2, 3, 4095, 4096, 8192)
SIZES = (0, 1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, MAX_BLOCKS * SPAN + 5)      # the last: the grid-stride second pass
RANGES = ((0.0, 1.0), (-37.5, 2.25))
LEVELS = (0.95, 0.5, 0.999)
OUT1 = (13,)


# ---------------------------------------------------------------------------------------------------------------------
# the bitwise definitions
# ---------------------------------------------------------------------------------------------------------------------
def bin32(conf, lo, hi, NB):
    """int64 like conf: the bin of float32 confidences, -1 for NaN"""
    c = np.asarray(conf, F32)
    lo32, hi32 = F32(lo), F32(hi)
    inv_w = F32(NB) / (hi32 - lo32)
    assert inv_w.dtype == np.float32
    inside = (c > lo32) & (c < hi32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(inside, c, lo32) - lo32
        prod = t * inv_w
    assert t.dtype == np.float32 and prod.dtype == np.float32
    b = np.minimum(prod.astype(np.int64), NB - 1)          # truncation: the values are not negative
    b = np.where(c >= hi32, NB - 1, b)
    b = np.where(c <= lo32, 0, b)
    return np.where(np.isnan(c), -1, b)


def state_ref(conf, lab, mask, out_labels, lo, hi, NB, state=None):
    """int64 [2 NB + 5]: dml_pooled_ood_update's definition, added onto `state` when given"""
    out = np.zeros(2 * NB + COUNTERS, np.int64) if state is None else np.array(state, dtype=np.int64)
    c = np.asarray(conf, F32).reshape(-1)
    lab = np.asarray(lab, np.int64).reshape(-1)
    if c.size == 0:
        return out
    keep = np.ones(c.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    b = bin32(c, lo, hi, NB)
    ok = keep & (b >= 0)
    row = np.where(np.isin(lab, np.asarray(out_labels, np.int64)), 0, 1)
    np.add.at(out, row[ok] * NB + b[ok], 1)
    with np.errstate(invalid="ignore"):
        out[2 * NB + 0] += int((keep & (b < 0)).sum())
        out[2 * NB + 1] += int((ok & (c < F32(lo))).sum())
        out[2 * NB + 2] += int((ok & (c > F32(hi))).sum())
    out[2 * NB + 3] += int((~keep).sum())
    out[2 * NB + 4] += 1
    return out


def finalize_ref(state, NB, level):
    """dict of the exact measures of a state: auroc, aupr and tie_mass as Fractions, fpr as the float64 quotient of its two integers,
    cut, P, N, pos_bins; auroc / aupr / tie_mass / fpr are None when P == 0 or N == 0"""
    h = [int(v) for v in np.asarray(state).reshape(-1)[:2 * NB]]
    Pb, Nb = h[:NB], h[NB:]
    P, N = sum(Pb), sum(Nb)
    r = {"P": P, "N": N, "pos_bins": sum(1 for v in Pb if v), "auroc": None, "aupr": None, "tie_mass": None, "fpr": None, "cut": -1}
    if P == 0 or N == 0:
        return r
    tp = fp = 0
    au = tie = 0
    aupr = Fraction(0)
    cands = []                                             # (tp, fp, bin) in ascending bin order
    prev = -1
    for b in range(NB):
        if Pb[b]:
            if prev >= 0:
                cands.append((tp, fp, prev))               # the previous positive bin: the negatives strictly below this one
            prev = b
        tp += Pb[b]
        fp += Nb[b]
        au += Pb[b] * (2 * (N - fp) + Nb[b])
        tie += Pb[b] * Nb[b]
        if Pb[b]:
            aupr += Fraction(Pb[b], P) * Fraction(tp, tp + fp)
    cands.append((P, sum(Nb[:prev + 1]), prev))            # the highest positive bin: full recall, its own fp
    rec = np.array([np.float64(c[0]) / np.float64(P) for c in cands])
    d = np.abs(rec - np.float64(level))
    best = np.flatnonzero(d == d.min())
    k = best[np.argmax(rec[best])]
    r.update(auroc=Fraction(au, 2 * P * N), aupr=aupr, tie_mass=Fraction(tie, P * N), fpr=float(np.float64(cands[k][1]) / np.float64(N)),
             cut=cands[k][2])
    return r


def quantised_scores(conf, lab, mask, out_labels, lo, hi, NB):
    """(pos, neg, pos_raw, neg_raw): the scores -bin of the positives / negatives the way eval_ood_measure reduces a frame, NaN
    and masked pixels left out, and the unquantised scores -conf of the same pixels"""
    c = np.asarray(conf, F32).reshape(-1)
    lab = np.asarray(lab, np.int64).reshape(-1)
    keep = (np.ones(c.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0) & ~np.isnan(c)
    b = bin32(c, lo, hi, NB)[keep]
    out = np.isin(lab[keep], np.asarray(out_labels, np.int64))
    raw = -c[keep].astype(np.float64)
    return -b[out].astype(np.float64), -b[~out].astype(np.float64), raw[out], raw[~out]


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------
def edge_values(lo, hi, NB):
    """float32 confidences on and around what bin() distinguishes: lo and hi, one ulp either side; bin edges and their neighbours;
    both zeros, subnormals, the infinities, NaN, values far outside"""
    lo32, hi32 = F32(lo), F32(hi)
    w = (np.float64(hi32) - np.float64(lo32)) / NB
    vals = [OC.down(lo32), lo32, OC.up(lo32), OC.down(hi32), hi32, OC.up(hi32)]
    for j in sorted({j for j in (1, 2, 3, NB // 3, NB // 2, NB - 2, NB - 1) if 0 < j < NB}):
        e = F32(np.float64(lo32) + j * w)
        vals += [OC.down(e), e, OC.up(e)]
    vals += [F32(0.0), F32(-0.0), F32(1e-45), F32(-1e-45), F32(1e-42), F32(-1e-42), F32(np.inf), F32(-np.inf), F32(np.nan),
             F32(np.float64(lo32) + 0.5 * w), F32(np.float64(hi32) - 0.5 * w), F32(2.0) * hi32 + F32(1.0), lo32 - F32(100.0),
             OC.FLT_MAX, -OC.FLT_MAX]
    return np.array(vals, F32)


def frame(n, lo, hi, seed, out_labels=OUT1, edges_nb=0, mask=False):
    """(conf float32 [n], labels int64 [n], mask uint8 [n] or None): confidences spread over a little more than [lo, hi], the
    positives (about 7 %) drawn lower; the first pixels replaced by edge_values(lo, hi, edges_nb) when edges_nb > 0; labels from
    the out-labels and other ids"""
    rs = np.random.RandomState(seed)
    others = np.array([1, 2, 3, 255, -1, 2 ** 31 + 6, 12], np.int64)
    pos = rs.rand(n) < 0.07
    lab = np.where(pos, np.asarray(out_labels, np.int64)[rs.randint(0, len(out_labels), n)], others[rs.randint(0, others.size, n)])
    u = np.where(pos, rs.beta(2.0, 4.0, n), rs.beta(4.0, 2.0, n))
    conf = (lo + (hi - lo) * (1.04 * u - 0.02)).astype(F32)
    if edges_nb:
        e = edge_values(lo, hi, edges_nb)[:n]
        conf[:e.size] = e
    m = (rs.rand(n) < 0.8).astype(np.uint8) if mask else None
    return conf, lab.astype(np.int64), m


def _fcase(conf, lab, mask, out_labels, lo, hi, NB):
    return {"conf": np.asarray(conf, F32), "lab": np.asarray(lab, np.int64), "mask": mask, "out": tuple(out_labels), "lo": lo, "hi": hi,
            "NB": NB}


def _finalize_table():
    c = {}
    for NB in (1, 2, 3, 17, 256, 4096, 8192):
        conf, lab, _ = frame(6000, 0.0, 1.0, 9100 + NB)
        c["smooth_nb%d" % NB] = _fcase(conf, lab, None, OUT1, 0.0, 1.0, NB)
    conf, lab, m = frame(5000, -37.5, 2.25, 9201, OC.OOD_OUT8, edges_nb=4095, mask=True)
    c["out8_masked_edges"] = _fcase(conf, lab, m, OC.OOD_OUT8, -37.5, 2.25, 4095)
    conf, lab = OC.ood_labelled()
    c["labels8"] = _fcase(conf, lab, None, OC.OOD_OUT8, -3.0, 2.5, 256)
    conf, lab, m = OC.ood_one_each()
    c["one_each"] = _fcase(conf, lab, m.astype(np.uint8), OUT1, -4.0, 4.0, 4096)
    # all positives in one bin, all negatives in another: positives below (flagged first, AUROC 1) and above (AUROC 0)
    lab = np.array([13] * 40 + [1] * 60, np.int64)
    c["sep_pos_low"] = _fcase([0.101] * 40 + [0.7] * 60, lab, None, OUT1, 0.0, 1.0, 256)
    c["sep_pos_high"] = _fcase([0.7] * 40 + [0.101] * 60, lab, None, OUT1, 0.0, 1.0, 256)
    c["one_bin"] = _fcase([0.3331] * 100, lab, None, OUT1, 0.0, 1.0, 3)                  # AUROC 0.5, tie mass 1, FPR 1
    conf, lab, _ = frame(3000, 0.0, 1.0, 9301)
    one = np.flatnonzero(lab == 13)[0]
    c["p1"] = _fcase(conf, np.where(np.arange(3000) == one, 13, 1), None, OUT1, 0.0, 1.0, 4096)
    c["n1"] = _fcase(conf, np.where(np.arange(3000) == one, 1, 13), None, OUT1, 0.0, 1.0, 4096)
    c["p0"] = _fcase(conf, np.ones(3000, np.int64), None, OUT1, 0.0, 1.0, 256)
    c["n0"] = _fcase(conf, np.full(3000, 13, np.int64), None, OUT1, 0.0, 1.0, 256)
    # recall levels that fall between, and exactly half-way between, the recalls that exist
    lab = np.array([13] * 4 + [1] * 8, np.int64)
    c["recall_ties"] = _fcase([0.1, 0.3, 0.5, 0.7, 0.05, 0.2, 0.2, 0.4, 0.6, 0.6, 0.8, 0.9], lab, None, OUT1, 0.0, 1.0, 17)
    return c


FINALIZE = _finalize_table()
_STATES = {}


def finalize_state(name):
    """the accumulated state of a FINALIZE case, in three updates (thirds of the frame); computed once and shared (read-only)"""
    if name not in _STATES:
        c = FINALIZE[name]
        st = None
        for part in np.array_split(np.arange(c["conf"].size), 3):
            st = state_ref(c["conf"][part], c["lab"][part], None if c["mask"] is None else c["mask"][part], c["out"], c["lo"], c["hi"],
                           c["NB"], st)
        st.setflags(write=False)
        _STATES[name] = st
    return _STATES[name]


def big_state(NB=4096, seed=9400, per_class=3.0e11):
    """int64 [2 NB + 5] written directly: about `per_class` counts in each row, spread over the bins as two overlapping bumps, a few
    bins empty: the AUROC numerator is about 10^23, past 64 bits"""
    rs = np.random.RandomState(seed)
    x = (np.arange(NB) + 0.5) / NB
    dp = np.exp(-0.5 * ((x - 0.35) / 0.12) ** 2) * rs.uniform(0.5, 1.5, NB)
    dn = np.exp(-0.5 * ((x - 0.65) / 0.15) ** 2) * rs.uniform(0.5, 1.5, NB)
    dp[rs.rand(NB) < 0.05] = 0.0
    st = np.zeros(2 * NB + COUNTERS, np.int64)
    st[:NB] = np.floor(per_class * dp / dp.sum()).astype(np.int64)
    st[NB:2 * NB] = np.floor(per_class * dn / dn.sum()).astype(np.int64)
    st[2 * NB + 4] = 1500
    return st
