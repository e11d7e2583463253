"""GPU: the open-set scoring and metric kernels at their edges -- dml_argmax_msp, dml_dissum_score, dml_novel_relabel,
dml_confusion_update, dml_class_feature_sum (csrc/scores.hip, csrc/eval_sums.hip) and dml_ood_measures (csrc/ood_measures.hip) through the C
ABI, and the Python wrappers where they hold logic.

Every comparison is against the float64 definitions of tests/open_set_cases.py on the same float32 inputs (proved right on
these inputs, without a GPU, by tests/test_open_set_refs.py) or against oracle/.  Integer outputs are compared exactly;
float outputs against bars derived there from the arithmetic a kernel may do.  Each float check prints
"MEASURE <what> err=<largest error> bar=<bar>" before it asserts (run with -s to see the figures).

Largest error measured on the MI355X next to its bar (the whole file takes about 6 s there):
  MSP                      4.3e-7   of 4.3e-6  (K = 16, 1024 x 2048; 10 % of the bar at worst, expf is well inside 2 ulp)
  dissum, normalised       1.3e-7   of 3.6e-7  (K = 1, 257 pixels: one division and one subtraction, 38 % of 6 eps32)
  dissum, range found      8.4e-5   of 1.5e-3  (K = 13, 65 pixels, scores around 5000)
  class feature sums       4.0e-10  of 4.3e-6  relative to sum |f| (C = 7, 16 x 768 x 768)
  prototype mean           17 %     of its bar (sum's bar / n + eps32 |mean|)
  AUROC                    1.1e-16  of 1e-15   (against scikit-learn's figure in the fixture; 0 against the oracle)
  AUPR                     1.1e-16  of 3.7e-15 (P = 33, N = 32); 5.6e-17 of 5.0e-14 at 8 388 608 scores; shuffled: 0 of 1e-13
  FPR, argmax, relabel, confusion counts, P / N: exact.  Relabel at 2 x 96 x 160: 0 of 30 720 pixels excluded.

Not covered, on purpose: MSP kinds (b)-(d) at 1024 x 2048 (only the distance logits run there); the feature sums at
16 x 768 x 768 with C = 32 (1.2 GB of host features); d == thresh at -1.5 for C = 1 (no dyadic square gives 1.5: -1 and its
neighbours stand in); "one ulp above" is reached by moving the threshold / the maximal logit one ulp below an exact d;
a dissum workgroup without any pixel cannot occur (the grid is ceil(H W / 256)), partially filled ones do.  dml_argmax_msp
and dml_novel_relabel do not check H / W / C, so no error code is asked of them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import open_set_cases as CS
from oracle import dmlnet_ref as O
from oracle import metrics_ref as MR
from oracle import ood_measures_ref as OR

pytestmark = pytest.mark.gpu

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
F64 = np.float64


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ood_cases():
    return CS.ood_cases()


@pytest.fixture(scope="module")
def g11b():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11b_ood_edges.npz"))


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_le(what, err, bar):
    err = float(err)
    print("MEASURE %s err=%.3e bar=%.3e" % (what, err, bar))
    assert err <= bar, "%s: error %.3e above the bar %.3e" % (what, err, bar)


# ---------------------------------------------------------------------------------------------------------------------
# dml_argmax_msp
# ---------------------------------------------------------------------------------------------------------------------
def _run_msp(lib, lg, kind):
    B, K, Hh, Ww = lg.shape
    d = dev(lg)
    preds = torch.full((B, Hh, Ww), -7, dtype=torch.int64, device="cuda")
    msp = torch.full((B, Hh, Ww), float("nan"), dtype=torch.float32, device="cuda")
    chk(lib.dml_argmax_msp(d.data_ptr(), preds.data_ptr(), msp.data_ptr(), B, K, Hh, Ww, st()))
    rp, rm = CS.msp_ref(lg)
    assert np.array_equal(preds.cpu().numpy(), rp)                           # first maximal index, every pixel
    got = msp.cpu().numpy().astype(F64)
    if kind == "gap":
        assert (got == 0.0).all()
    if kind == "uniform":
        check_le("msp uniform K=%d vs 1-1/K" % K, np.abs(got - (1.0 - 1.0 / K)).max(), CS.msp_bar(K))
    check_le("msp %s K=%d %dx%dx%d" % (kind, K, B, Hh, Ww), np.abs(got - rm).max(), CS.msp_bar(K))
    # either output may be null
    p2 = torch.full_like(preds, -7)
    chk(lib.dml_argmax_msp(d.data_ptr(), p2.data_ptr(), None, B, K, Hh, Ww, st()))
    m2 = torch.full_like(msp, float("nan"))
    chk(lib.dml_argmax_msp(d.data_ptr(), None, m2.data_ptr(), B, K, Hh, Ww, st()))
    assert torch.equal(p2, preds) and torch.equal(m2, msp)


@pytest.mark.parametrize("K", CS.MSP_KS)
@pytest.mark.parametrize("kind", CS.MSP_KINDS)
def test_argmax_msp(lib, kind, K):
    """bar 2 (2K + 4) eps32"""
    for shape in CS.MSP_SHAPES:
        _run_msp(lib, CS.msp_logits(kind, K, shape), kind)


def test_argmax_msp_full_image(lib):
    K, shape = CS.MSP_BIG
    _run_msp(lib, CS.msp_logits("dist", K, shape), "dist")


def test_argmax_msp_wrapper(lib):
    import utils
    lg = CS.msp_logits("dist", 19, (3, 5, 7))
    preds, msp = utils.argmax_msp(dev(lg))
    rp, rm = CS.msp_ref(lg)
    assert np.array_equal(preds.cpu().numpy(), rp)
    check_le("msp wrapper", np.abs(msp.cpu().numpy().astype(F64) - rm).max(), CS.msp_bar(19))


# ---------------------------------------------------------------------------------------------------------------------
# dml_dissum_score
# ---------------------------------------------------------------------------------------------------------------------
def _run_dissum(lib, lg, clip, inclusive, what):
    """every image of the batch against the definition evaluated on that image alone"""
    B, K, Hh, Ww = lg.shape
    d = dev(lg)
    score = torch.full((B, Hh, Ww), 7.0, dtype=torch.float32, device="cuda")
    work = torch.full((2 * B,), 7.0, dtype=torch.float32, device="cuda")
    chk(lib.dml_dissum_score(d.data_ptr(), score.data_ptr(), work.data_ptr(), B, K, Hh, Ww, float(clip),
                             1 if inclusive else 0, st()))
    got, w = score.cpu().numpy().astype(F64), work.cpu().numpy().astype(F64)
    for b in range(B):
        ref, s = CS.dissum_ref(lg[b], clip, inclusive)
        with np.errstate(all="ignore"):
            assert np.array_equal(O.dissum_score(lg[b].astype(F64), clip, inclusive), ref, equal_nan=True)
        bar, max_err = CS.dissum_bar(lg[b], clip, inclusive)
        tag = "%s K=%d clip=%g img %d" % (what, K, clip, b)
        # before normalisation: the per-image range the kernel found (x2 slack on the summation bound)
        check_le("dissum min " + tag, abs(w[2 * b] - s.min()), 2 * max_err)
        check_le("dissum max " + tag, abs(w[2 * b + 1] - s.max()), 2 * max_err)
        if s.max() == s.min():
            assert np.isnan(got[b]).all()                                    # constant image: 0 / 0, as NumPy
            continue
        assert not np.isnan(got[b]).any()
        check_le("dissum " + tag, np.abs(got[b] - ref).max(), bar)
    return got


@pytest.mark.parametrize("clip,inclusive", CS.DISSUM_MODES)
@pytest.mark.parametrize("K", CS.DISSUM_KS)
def test_dissum_batch_is_normalised_per_image(lib, K, clip, inclusive):
    """B = 3, ranges 1 : 100 : 10000, negative and positive scores.  Bar 2 (2 max_err / (hi - lo) + 3 eps32) with
    max_err = (K - 1) eps32 max_px sum_k |logit_k|"""
    _run_dissum(lib, CS.dissum_batch(K), clip, inclusive, "batch")


@pytest.mark.parametrize("clip,inclusive", CS.DISSUM_MODES)
@pytest.mark.parametrize("K", CS.DISSUM_KS)
def test_dissum_on_the_clip_and_all_clipped_but_one(lib, K, clip, inclusive):
    """exactly summing logits: scores on the clip and one ulp either side; max_err = 0, so the range is exact and the bar
    is 6 eps32"""
    lg = CS.dissum_on_clip(K)
    bar, max_err = CS.dissum_bar(lg[0], clip, inclusive)
    if K == 1:
        assert max_err == 0.0
    got = _run_dissum(lib, lg, clip, inclusive, "on-clip")
    s = -lg[0].astype(F64).sum(axis=0).ravel()
    assert (got[0].ravel()[s >= clip] == 1.0).all()                          # on and above the clip: the maximum itself
    got = _run_dissum(lib, CS.dissum_all_clip_but_one(K), clip, inclusive, "all-but-one")
    assert (got[0].ravel() == 1.0).sum() == got[0].size - 1 and got[0].ravel()[41] == 0.0


@pytest.mark.parametrize("clip,inclusive", CS.DISSUM_MODES)
@pytest.mark.parametrize("hw", CS.DISSUM_HW)
def test_dissum_partial_waves_and_workgroups(lib, hw, clip, inclusive):
    """H W = 1 is a constant image (NaN); 1024 * 2048 + 1 runs the capped grid with a one-pixel tail"""
    for K in ((13,) if hw > 1000 else (1, 13)):
        _run_dissum(lib, CS.dissum_flat(K, hw), clip, inclusive, "hw=%d" % hw)


def test_dissum_constant_image_is_nan(lib):
    lg = np.full((2, 4, 8, 8), -2.0, np.float32)
    lg[1, :, 3, 3] = -1.0                                                    # image 1 is not constant
    got = _run_dissum(lib, lg, 400.0, True, "constant")
    assert np.isnan(got[0]).all() and got[1].max() == 1.0 and got[1].min() == 0.0


def test_dissum_signed_zero_maximum(lib):
    """every score negative except one pixel whose logits are all +0.0: that zero is the image's maximum.  A kernel that
    negates the zero sum to -0.0 and picks the integer atomic by `v >= 0` leaves the stored maximum at the largest
    negative score (atomicMax(int, INT_MIN) changes nothing) and normalises the whole image wrongly."""
    got = _run_dissum(lib, CS.dissum_signed_zero(False), 1000.0, False, "signed-zero")
    assert got[0].ravel()[5] == 1.0 and got[0].ravel()[0] == 0.0


def test_dissum_signed_zero_in_last_workgroup(lib):
    """the same with the zero in the last workgroup and the minimum at pixel 0 (the minimum's half of the defect depends
    on the order workgroups retire in); also as image 1 of a batch whose image 0 is ordinary"""
    got = _run_dissum(lib, CS.dissum_signed_zero(True), 400.0, True, "signed-zero-last")
    assert got[0].ravel()[-1] == 1.0 and got[0].ravel()[0] == 0.0
    z = CS.dissum_signed_zero(True)
    both = np.concatenate([CS.dissum_flat(4, z.shape[-1]), z])
    got = _run_dissum(lib, both, 400.0, True, "signed-zero-batch")
    assert got[1].ravel()[-1] == 1.0 and got[1].ravel()[0] == 0.0


def test_dissum_wrapper(lib):
    import utils
    lg = CS.dissum_batch(16)
    got = utils.dissum_score(dev(lg), 400.0, True).cpu().numpy().astype(F64)
    for b in range(3):
        check_le("dissum wrapper img %d" % b, np.abs(got[b] - CS.dissum_ref(lg[b], 400.0, True)[0]).max(),
                 CS.dissum_bar(lg[b], 400.0, True)[0])


# ---------------------------------------------------------------------------------------------------------------------
# dml_novel_relabel
# ---------------------------------------------------------------------------------------------------------------------
def _run_relabel(lib, feats, lg, proto, preds, thresh, new_label):
    B, K, Hh, Ww = lg.shape
    f, l, p, out = dev(feats), dev(lg), dev(proto), dev(preds).clone()
    chk(lib.dml_novel_relabel(f.data_ptr(), l.data_ptr(), p.data_ptr(), out.data_ptr(), B, feats.shape[-1], K, Hh, Ww,
                              float(thresh), int(new_label), st()))
    return out.cpu().numpy()


@pytest.mark.parametrize("new_label", CS.RELABEL_LABELS)
@pytest.mark.parametrize("K", CS.RELABEL_KS)
@pytest.mark.parametrize("C", CS.RELABEL_CS)
def test_relabel_exact_boundaries(lib, C, K, new_label):
    """d == thresh and d == max logit are not relabelled, one fp32 ulp above each is; a pixel that already carries
    new_label and one that holds 255 below the threshold keep their value.  Thresholds -1.5, 0 and their fp32 neighbours.
    Everything is exact in fp32: no pixel is excluded."""
    feats, lg, proto, preds, expect = CS.relabel_exact(C, K, new_label)
    for th in expect:
        got = _run_relabel(lib, feats, lg, proto, preds, th, new_label)
        for b in range(2):
            ref, _, _ = CS.relabel_ref(preds[b], lg[b], feats[b], proto, th, new_label)
            assert np.array_equal(O.novel_relabel(preds[b], lg[b].astype(F64), feats[b].astype(F64), proto.astype(F64),
                                                  th, new_label), ref)
            assert np.array_equal(got[b], ref), (th, b, got[b], ref)


@pytest.mark.parametrize("thresh", (-1.5, 0.0))
def test_relabel_random(lib, thresh):
    """2 x 96 x 160, C = K = 16: exact except where the fp64 margin is below the fp32 bound (C + 2) eps32 |d|; at most
    0.1 % of the pixels may be excluded that way"""
    import utils
    feats, lg, proto, preds = CS.relabel_random()
    got = _run_relabel(lib, feats, lg, proto, preds, thresh, 16)
    via = utils.novel_relabel(dev(preds).clone(), dev(lg), dev(feats), proto, thresh, 16).cpu().numpy()
    assert np.array_equal(via, got)
    excluded = 0
    for b in range(preds.shape[0]):
        ref, d, margin = CS.relabel_ref(preds[b], lg[b], feats[b], proto, thresh, 16)
        sure = margin > CS.relabel_err(d, feats.shape[-1])
        excluded += int((~sure).sum())
        assert np.array_equal(got[b][sure], ref[sure])
    print("MEASURE relabel random thresh=%g excluded=%d of %d" % (thresh, excluded, preds.size))
    assert excluded <= CS.EXCLUDE_CAP * preds.size


# ---------------------------------------------------------------------------------------------------------------------
# dml_confusion_update / StreamSegMetrics
# ---------------------------------------------------------------------------------------------------------------------
def _confusion(lib, lt, lp, n, hist=None):
    count = lt.size
    a = dev(lt) if count else torch.zeros(2, dtype=torch.int64, device="cuda")      # count = 0: valid pointers all the same
    b = dev(lp) if count else torch.zeros(2, dtype=torch.int64, device="cuda")
    if hist is None:
        hist = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    chk(lib.dml_confusion_update(a.data_ptr(), b.data_ptr(), hist.data_ptr(), count, n, st()))
    return hist


@pytest.mark.parametrize("n", CS.CONF_NS)
@pytest.mark.parametrize("count", CS.CONF_COUNTS)
def test_confusion_counts(lib, n, count):
    """labels 255 / -1 / n / 2**40 are ignored, predictions outside [0, n) are dropped; exact counts"""
    lt, lp = CS.confusion_inputs(n, count)
    hist = _confusion(lib, lt, lp, n)
    assert np.array_equal(hist.cpu().numpy(), CS.confusion_ref(lt, lp, n))
    # on top of what is there: the update accumulates
    hist = _confusion(lib, lt, lp, n, hist)
    assert np.array_equal(hist.cpu().numpy(), 2 * CS.confusion_ref(lt, lp, n))


@pytest.mark.parametrize("n", CS.CONF_NS)
def test_confusion_every_label_ignored_and_one_cell(lib, n):
    count = 2 * 2048 * 256 + 1
    lp = np.zeros(count, np.int64)
    for v in (255, -1, n, 2 ** 40):
        if 0 <= v < n:
            continue
        assert int(_confusion(lib, np.full(count, v, np.int64), lp, n).abs().sum()) == 0
    t, p = 3 % n, 5 % n                                                      # every pixel in one cell
    hist = _confusion(lib, np.full(count, t, np.int64), np.full(count, p, np.int64), n).cpu().numpy()
    want = np.zeros((n, n), np.int64)
    want[t, p] = count
    assert np.array_equal(hist, want)


def test_confusion_error_codes(lib):
    """argument checks that return before any launch"""
    a = torch.zeros(64, dtype=torch.int64, device="cuda")
    hist = torch.zeros((65, 65), dtype=torch.int64, device="cuda")
    assert lib.dml_confusion_update(a.data_ptr(), a.data_ptr(), hist.data_ptr(), 32, 65, st()) == EINVAL
    assert lib.dml_confusion_update(a.data_ptr(), a.data_ptr(), hist.data_ptr(), 32, 0, st()) == EINVAL
    assert lib.dml_confusion_update(a.data_ptr(), a.data_ptr(), hist.data_ptr(), -1, 19, st()) == EINVAL
    assert lib.dml_confusion_update(None, a.data_ptr(), hist.data_ptr(), 32, 19, st()) == EINVAL
    off = a[1:]
    assert off.data_ptr() % 16 == 8
    assert lib.dml_confusion_update(off.data_ptr(), a.data_ptr(), hist.data_ptr(), 32, 19, st()) == EALIGN
    assert lib.dml_confusion_update(a.data_ptr(), off.data_ptr(), hist.data_ptr(), 32, 19, st()) == EALIGN
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0


@pytest.mark.parametrize("n", CS.CONF_NS)
def test_stream_metrics_accumulates_and_scores(lib, n):
    """50 updates into one matrix against one bincount over the concatenation; get_results against the oracle on the same
    matrix, NaN paths (classes never seen / never predicted) included -- the same float64 expressions, so equal"""
    import metrics
    rs = np.random.RandomState(11 + n)
    m = metrics.StreamSegMetrics(n)
    empty = m.get_results()                                                  # nothing seen: 0 / 0 everywhere
    assert np.isnan(empty["Overall Acc"]) and np.isnan(empty["Mean IoU"])
    lts, lps = [], []
    for it in range(50):
        lt, lp = CS.confusion_inputs(n, int(rs.randint(1, 4000)), seed=1000 + it)
        if n > 2:
            lt[lt == n - 1] = 0                                              # class n - 1 never present ...
            lp[(lp == 1) | (lp == n - 1)] = 0                                # ... nor predicted; class 1 never predicted
        lp[lp >= n] = 0                                                      # the oracle's bincount needs predictions in range
        lp[lp < 0] = 0
        lts.append(lt)
        lps.append(lp)
        t, p = dev(lt), dev(lp)
        if it % 2:                                                           # views 8 bytes off a 16-byte boundary: the wrapper copies
            t, p = dev(np.r_[0, lt])[1:], dev(np.r_[0, lp])[1:]
        m.update(t, p)
    lt, lp = np.concatenate(lts), np.concatenate(lps)
    hist = MR.fast_hist(lt, lp, n)
    assert np.array_equal(m.confusion_matrix.cpu().numpy(), hist)
    got, ref = m.get_results(), MR.results(hist)
    for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
        assert got[k] == ref[k] or (np.isnan(got[k]) and np.isnan(ref[k])), (k, got[k], ref[k])
    assert np.array_equal(np.array([got["Class IoU"][c] for c in range(n)]),
                          np.array([ref["Class IoU"][c] for c in range(n)]), equal_nan=True)
    if n > 2:
        assert np.isnan(got["Class IoU"][n - 1]) and got["Class IoU"][1] == 0.0
    m.reset()
    m.update(dev(np.full(7, 255, np.int64)), dev(np.zeros(7, np.int64)))     # every label ignored
    assert int(m.confusion_matrix.sum()) == 0 and np.isnan(m.get_results()["Mean IoU"])


# ---------------------------------------------------------------------------------------------------------------------
# dml_class_feature_sum / extract_prototype
# ---------------------------------------------------------------------------------------------------------------------
def _fsum(lib, f, lab, c):
    fd, ld = dev(f), dev(lab)
    sums = torch.full((f.shape[1],), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    chk(lib.dml_class_feature_sum(fd.data_ptr(), ld.data_ptr(), f.shape[0], f.shape[1], int(c), sums.data_ptr(),
                                  cnt.data_ptr(), st()))
    return sums.cpu().numpy(), int(cnt.item())


def _check_fsum(lib, f, lab, c, what):
    got, n = _fsum(lib, f, lab, c)
    ref, abs_sum, rn = CS.fsum_ref(f, lab, c)
    assert n == rn                                                           # counts exact
    if rn == 0:
        assert (got == 0.0).all()                                            # absent: exactly 0
        return
    rel = np.abs(got - ref) / abs_sum
    check_le("feature sum %s C=%d n_px=%d class %d (relative to sum|f|)" % (what, f.shape[1], f.shape[0], c), rel.max(),
             CS.fsum_bar(f.shape[0], 1.0))


@pytest.mark.parametrize("n_px", CS.FSUM_NPX)
@pytest.mark.parametrize("Cc", CS.FSUM_CS)
def test_class_feature_sum(lib, Cc, n_px):
    """features 1e3 + N(0, 1); class absent, one pixel only (the last), an ordinary class, every pixel.  Bar
    2 ceil(n_px / 262144) eps32 relative to sum |f| of the class"""
    f, lab = CS.fsum_inputs(Cc, n_px)
    for c in (0, 1, 3, 4):
        _check_fsum(lib, f, lab, c, "mixed")
    got, n = _fsum(lib, f, lab, 4)
    assert n == 1 and np.array_equal(got, f[-1].astype(F64))                  # one term: exact
    _check_fsum(lib, f, np.full(n_px, 6, np.int64), 6, "every pixel")


@pytest.mark.parametrize("Cc", (1, 7, 16))
def test_class_feature_sum_full_batch(lib, Cc):
    """16 x 768 x 768 pixels: the capped grid gives every thread up to 36 terms of fp32 before the fp64 finish"""
    f, lab = CS.fsum_inputs(Cc, CS.FSUM_BIG)
    for c in (1, 3, 4):
        _check_fsum(lib, f, lab, c, "full")


def test_class_feature_sum_error_codes(lib):
    a = torch.zeros(64, dtype=torch.float32, device="cuda")
    l = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert lib.dml_class_feature_sum(a.data_ptr(), l.data_ptr(), 2, CS.MAXC + 1, 0, s.data_ptr(), l.data_ptr(), st()) == EINVAL
    assert lib.dml_class_feature_sum(a.data_ptr(), l.data_ptr(), 0, 16, 0, s.data_ptr(), l.data_ptr(), st()) == EINVAL
    assert lib.dml_class_feature_sum(a.data_ptr(), l.data_ptr(), 2, 0, 0, s.data_ptr(), l.data_ptr(), st()) == EINVAL


def test_extract_prototype_mean_and_five_percent_rule(lib):
    import utils
    f, lab = CS.fsum_inputs(16, 2000)
    lab[:] = 0
    lab[100:200] = 9                                                         # exactly 5 %: `<=` -> None
    lab[-1] = 4
    fd = dev(f).view(1, 40, 50, 16)
    assert utils.extract_prototype(fd, dev(lab).view(40, 50), 9) is None
    assert utils.extract_prototype(fd, dev(lab).view(40, 50), 3) is None      # absent
    assert utils.extract_prototype(fd, dev(lab).view(40, 50), 4) is None      # one pixel
    lab[200] = 9                                                             # one pixel above
    got = utils.extract_prototype(fd, dev(lab).view(40, 50), 9)
    ref, abs_sum, n = CS.fsum_ref(f, lab, 9)
    assert n == 101 and len(got) == 16
    mean = ref / n
    # the sum's bar over n, plus the rounding of the mean to float32
    bar = CS.fsum_bar(2000, abs_sum) / n + CS.EPS32 * np.abs(mean)
    err = np.abs(np.array(got, F64) - mean)
    check_le("prototype mean (worst err / bar)", (err / bar).max(), 1.0)
    every = utils.extract_prototype(fd, dev(np.full(2000, 2, np.int64)), 2)
    mean = f.astype(F64).mean(axis=0)
    bar = CS.fsum_bar(2000, np.abs(f.astype(F64)).sum(axis=0)) / 2000 + CS.EPS32 * np.abs(mean)
    check_le("prototype mean, every pixel (worst err / bar)", (np.abs(np.array(every, F64) - mean) / bar).max(), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# dml_ood_measures / anom_utils
# ---------------------------------------------------------------------------------------------------------------------
def _check_measures(got, pos, neg, recall, what, fixture=None):
    ref = OR.get_measures(pos, neg, recall)
    bar = CS.ood_aupr_bar(pos)
    check_le("auroc " + what, abs(got[0] - ref[0]), 1e-15)
    check_le("aupr " + what, abs(got[1] - ref[1]), bar)
    assert got[2] == ref[2], (what, got[2], ref[2])
    if fixture is not None:                      # scikit-learn's figures: within 2e-16 of the oracle (test_open_set_refs.py)
        check_le("auroc vs fixture " + what, abs(got[0] - fixture[0]), 1e-15)
        check_le("aupr vs fixture " + what, abs(got[1] - fixture[1]), bar + 2e-16)
        assert got[2] == fixture[2], (what, got[2], fixture[2])


@pytest.mark.parametrize("name", CS.OOD_NAMES)
def test_ood_get_measures_edges(lib, name, ood_cases, g11b):
    """P = 1, N = 1, fewer keys than sort waves, ties, signed zeros / subnormals / +-FLT_MAX, recall levels, 8 M scores.
    AUROC 1e-15, AUPR P_distinct eps64 (at most 1e-11), FPR exact -- against the oracle and the reference's own figures"""
    import anom_utils
    pos, neg, recall = ood_cases[name]
    got = anom_utils.get_measures(dev(pos), dev(neg), recall)
    _check_measures(got, pos, neg, recall, name, g11b[name + "_res"])
    if name == "all_equal":
        assert got == (0.5, 40 / 100, 1.0)
    if name == "order_zero_only":
        assert got == (0.5, 4 / 7, 1.0)
    if name == "sep_high":
        assert got[0] == 1.0
    if name == "sep_low":
        assert got[0] == 0.0


def test_ood_eight_out_labels_and_masks(lib, ood_cases, g11b):
    import anom_utils
    conf, lab = CS.ood_labelled()
    got = anom_utils.eval_ood_measure(dev(conf), dev(lab), list(CS.OOD_OUT8))
    pos, neg, r = ood_cases["labels8"]
    assert OR.eval_ood_measure(conf, lab, list(CS.OOD_OUT8)) == OR.get_measures(pos, neg, r)
    _check_measures(got, pos, neg, r, "labels8", g11b["labels8_res"])
    assert anom_utils.eval_ood_measure(dev(conf), dev(lab), [4, 5, 6]) is None            # labels never in the set
    conf, lab, mask = CS.ood_one_each()
    got = anom_utils.eval_ood_measure(dev(conf), dev(lab), [13], mask=dev(mask))
    _check_measures(got, *ood_cases["one_each"], "one_each", g11b["one_each_res"])
    only_pos = mask & (lab == 13)
    assert anom_utils.eval_ood_measure(dev(conf), dev(lab), [13], mask=dev(only_pos)) is None


@pytest.mark.parametrize("P", (20, 301))
def test_ood_recall_levels_differ(lib, P, ood_cases):
    """the four recall levels pick four different cut-offs on the same scores"""
    import anom_utils
    fprs = []
    for r in (0.0, 0.5, 0.95, 1.0):
        pos, neg, recall = ood_cases["recall_%d_%g" % (P, r)]
        fprs.append(anom_utils.get_measures(dev(pos), dev(neg), recall)[2])
    assert fprs[0] == 0.0 and fprs == sorted(fprs) and len(set(fprs)) == 4


def test_ood_four_images_and_shuffle(lib, ood_cases, g11b):
    """8 388 608 scores in image order through eval_ood_measure, then shuffled: identical AUROC / FPR, AUPR within 1e-13"""
    import anom_utils
    conf, lab = CS.ood_big()
    got = anom_utils.eval_ood_measure(dev(conf), dev(lab), [12, 13])
    _check_measures(got, *ood_cases["big4"], "big4 in image order", g11b["big4_res"])
    perm = np.random.RandomState(5).permutation(conf.size)
    got2 = anom_utils.eval_ood_measure(dev(conf[perm]), dev(lab[perm]), [12, 13])
    assert got2[0] == got[0] and got2[2] == got[2]
    check_le("aupr big4 shuffled vs in order", abs(got2[1] - got[1]), 1e-13)


def test_ood_error_codes(lib):
    """argument checks that return before any launch: n_out = 9, n = 2**31, a short or misaligned workspace"""
    n = 1000
    conf = torch.zeros(n, dtype=torch.float32, device="cuda")
    lab = torch.zeros(n, dtype=torch.int64, device="cuda")
    res = torch.full((5,), 7.0, dtype=torch.float64, device="cuda")
    need = lib.dml_ood_workspace_bytes(n)
    assert need > 2 * 8 * n and lib.dml_ood_workspace_bytes(0) == 0
    work = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    ol = (C.c_int64 * 9)(*range(9))

    def call(n_=n, n_out=1, wp=work.data_ptr(), wb=need):
        return lib.dml_ood_measures(conf.data_ptr(), lab.data_ptr(), None, n_, ol, n_out, 0.95, wp, wb, res.data_ptr(), st())

    assert call(n_out=9) == EINVAL and call(n_out=0) == EINVAL and call(n_=0) == EINVAL
    assert call(n_=2 ** 31) == EUNSUPPORTED                                  # before the workspace is looked at
    assert call(wb=need - 1) == EINVAL
    assert call(wp=work.data_ptr() + 128, wb=need + 384) == EINVAL
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 7.0).all()                                  # nothing ran
    chk(call(n_out=8))                                                       # and the same buffers are fine when the arguments are
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert r[3] == n and r[4] == 0 and np.isnan(r[0])                        # label 0 is an out-label: only positives
