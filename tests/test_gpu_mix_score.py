"""GPU: the "EDS + MMSP" anomaly score -- dml_dissum_msp_score (csrc/scores.hip) through the C ABI, through
utils.dissum_msp_score and through the open-set driver's `--ood dissum_msp`.

Every float comparison is against the float64 definition of tests/mix_cases.py on the same float32 inputs (proved to be the
reference's statements, without a GPU, by tests/test_mix_refs.py), on EVERY pixel, to the per-pixel bar derived there; the NaN
pattern must be the definition's exactly.  Each float check prints
"MEASURE <case> err=<largest error> bar=<largest bar> worst err/bar=<largest ratio>" before it asserts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import mix_cases as MC

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
F64 = np.float64
GUARD = 64                       # floats before and after the output: 256 bytes, so the output keeps its alignment


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def run(lib, lg, case, offset=0, k_first=None):
    """dml_dissum_msp_score on a host array -> conf [B, H, W] as numpy.  The output is pre-filled with NaN between two
    guards that must come back untouched, and so is the work buffer's end; `offset` shifts the logits pointer by that many
    floats."""
    B, K, Hh, Ww = lg.shape
    k_first = case["k_first"] if k_first is None else k_first
    lbuf = torch.zeros(lg.size + offset, dtype=torch.float32, device="cuda")
    lbuf[offset:] = torch.from_numpy(np.array(lg).ravel()).cuda()             # a writable copy
    n = B * Hh * Ww
    obuf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    obuf[GUARD:GUARD + n] = float("nan")
    nwork = 4 * B + 2 * n
    work = torch.full((nwork + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.dml_dissum_msp_score(lbuf.data_ptr() + 4 * offset, obuf.data_ptr() + 4 * GUARD, work.data_ptr(), B, K, Hh, Ww,
                                  k_first, case["clip"], case["threshold"], case["slope"],
                                  1 if case["prob"] == "logit" else 0, st())
    assert rc == 0, "dml_dissum_msp_score returned %d" % rc
    torch.cuda.synchronize()
    out = obuf.cpu().numpy()
    assert (out[:GUARD] == 7.0).all() and (out[GUARD + n:] == 7.0).all(), "a guard element of the output was written"
    assert (work[nwork:].cpu().numpy() == 7.0).all(), "the work buffer was written past 4 B + 2 B H W floats"
    return out[GUARD:GUARD + n].reshape(B, Hh, Ww)


def check(what, got, ref):
    """the definition's NaN pattern exactly, the finite pixels to the bar"""
    want, bar = ref["conf"], ref["bar"]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: %d pixels NaN, the definition has %d" % (what, np.isnan(got).sum(), nan.sum())
    if nan.all():
        print("MEASURE %s NaN on every pixel, as the definition" % what)
        return
    err = np.abs(got.astype(F64) - want)[~nan]
    ratio = err / bar[~nan]
    print("MEASURE %s err=%.3e bar=%.3e worst err/bar=%.3e" % (what, err.max(), bar[~nan].max(), ratio.max()))
    bad = np.flatnonzero(np.nan_to_num(np.abs(got.astype(F64) - want), nan=0.0) > np.nan_to_num(bar, nan=0.0))
    assert bad.size == 0, "%s: %d pixels above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_score_against_float64(lib, name):
    case = MC.CASES[name]
    lg, ref = MC.reference(name)
    got = run(lib, lg, case)
    check(name, got, ref)
    assert np.isnan(ref["conf"]).all() == (name in MC.NAN_CASES)
    # two runs are bitwise equal
    assert np.array_equal(bits(got), bits(run(lib, lg, case)))
    # image b of the batch equals the same image run alone, bitwise
    if lg.shape[0] > 1:
        for b in range(lg.shape[0]):
            alone = run(lib, lg[b:b + 1], case)
            assert np.array_equal(bits(alone[0]), bits(got[b])), "image %d differs from its solo run" % b
    if case["slope"] == 0.0:                                             # conf = (d + q) / 2
        mean = 0.5 * (ref["d"] + ref["q"])
        assert np.abs(got.astype(F64) - mean).max() <= ref["bar"].max()
    if case["slope"] == 200.0:                                           # float32's exp overflows: the result is finite, conf = q
        over = case["slope"] * (ref["d"] - case["threshold"]) > 89.0
        assert over.any() and np.isfinite(got).all()


@pytest.mark.parametrize("name", ("kfirst_softmax", "kfirst_logit", "kfirst_vec_softmax", "kfirst_vec_logit"))
def test_first_class_skips_the_background_without_a_copy(lib, name):
    """k_first = 1 on 14 classes: the same bits as the call on a contiguous copy of [:, 1:]"""
    case = MC.CASES[name]
    lg, ref = MC.reference(name)
    got = run(lib, lg, case)
    check(name + " in place", got, ref)
    copy = run(lib, np.ascontiguousarray(lg[:, 1:]), case, k_first=0)
    assert np.array_equal(bits(got), bits(copy))
    # and the background plane takes no part: another one changes nothing
    other = np.array(lg)
    other[:, 0] = 1e30
    assert np.array_equal(bits(got), bits(run(lib, other, case)))


@pytest.mark.parametrize("name", MC.OFFSET_CASES)
def test_logits_pointer_offset_by_one_float(lib, name):
    """a logits pointer that is not 16-byte aligned takes the one-float-per-lane path, whatever H W is"""
    case = MC.CASES[name]
    lg, ref = MC.reference(name)
    got = run(lib, lg, case, offset=1)
    check(name + " offset", got, ref)
    # every pixel's arithmetic is the same on both paths and the ranges do not depend on the order
    assert np.array_equal(bits(got), bits(run(lib, lg, case)))


def test_error_codes(lib):
    """argument checks that return before any launch; the limits themselves are accepted"""
    a = torch.full((8192,), -7.0, dtype=torch.float32, device="cuda")
    o = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    w = torch.full((4096,), 7.0, dtype=torch.float32, device="cuda")
    A, O, Wk = a.data_ptr(), o.data_ptr(), w.data_ptr()

    def call(lg=A, conf=O, work=Wk, B=1, K=13, Hh=4, Ww=4, k_first=0, prob_logit=0):
        return lib.dml_dissum_msp_score(lg, conf, work, B, K, Hh, Ww, k_first, 400.0, 0.2, 50.0, prob_logit, st())

    assert call(lg=None) == EINVAL and call(conf=None) == EINVAL and call(work=None) == EINVAL
    assert call(B=0) == EINVAL and call(K=0) == EINVAL and call(Hh=0) == EINVAL and call(Ww=0) == EINVAL
    assert call(B=-1) == EINVAL and call(K=-1) == EINVAL and call(Hh=-1) == EINVAL and call(Ww=-1) == EINVAL
    assert call(k_first=-1) == EINVAL and call(k_first=13) == EINVAL and call(k_first=14) == EINVAL
    assert call(K=MC.MAX_CLASSES + 1) == EUNSUPPORTED and call(K=40, k_first=7) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED
    assert call(B=2, Hh=2 ** 20, Ww=2 ** 20) == EUNSUPPORTED and call(B=1, Hh=2 ** 20 + 1, Ww=2 ** 20) == EUNSUPPORTED
    assert call(B=65535, Hh=2 ** 30, Ww=2 ** 30) == EUNSUPPORTED             # B H W beyond int64's comfort
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all() and (w.cpu().numpy() == 7.0).all() and (a.cpu().numpy() == -7.0).all()
    # the limits themselves are accepted: 32 classes, 32 classes behind k_first, and 65535 images of one pixel
    assert call(K=MC.MAX_CLASSES, Hh=2, Ww=2, prob_logit=1) == 0
    assert call(K=40, k_first=8, Hh=2, Ww=2, prob_logit=1) == 0
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all()                                   # a constant image: NaN, and nothing beyond it
    assert (w[4 + 8:].cpu().numpy() == 7.0).all()
    nb = 65535
    lg = torch.randn(nb * 2, dtype=torch.float32, device="cuda")
    conf = torch.full((nb + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    work = torch.empty(6 * nb, dtype=torch.float32, device="cuda")
    assert call(lg=lg.data_ptr(), conf=conf.data_ptr(), work=work.data_ptr(), B=nb, K=2, Hh=1, Ww=1) == 0
    torch.cuda.synchronize()
    out = conf.cpu().numpy()
    assert np.isnan(out[:nb]).all() and (out[nb:] == 7.0).all()              # one pixel per image: NaN everywhere


def test_utils_wrapper(lib):
    import utils
    for name in ("batch_k13_softmax_400", "vec_k19_logit_1000", "kfirst_softmax", "steep_logit"):
        case = MC.CASES[name]
        lg, ref = MC.reference(name)
        t = torch.from_numpy(np.array(lg)).cuda()
        got = utils.dissum_msp_score(t, clip=case["clip"], threshold=case["threshold"], slope=case["slope"],
                                     prob=case["prob"], first_class=case["k_first"])
        assert got.shape == ref["conf"].shape and got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(bits(got.cpu().numpy()), bits(run(lib, lg, case)))
    # the defaults are the anomaly driver's: clip 400, Coefficient_map(dis_sum, 0.2), lamda = 50, the softmax, every class
    lg, ref = MC.reference("vec_k13_softmax_400")
    t = torch.from_numpy(np.array(lg)).cuda()
    assert np.array_equal(bits(utils.dissum_msp_score(t).cpu().numpy()), bits(run(lib, lg, MC.CASES["vec_k13_softmax_400"])))
    # the DeepLab recipe is reachable
    deeplab = utils.dissum_msp_score(t, clip=1000.0, threshold=0.3, prob="logit")
    want = MC.score_ref(lg, 1000.0, 0.3, 50.0, "logit")
    check("deeplab recipe", deeplab.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        utils.dissum_msp_score(torch.zeros(1, 13, 4, 4))                     # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        utils.dissum_msp_score(torch.zeros(13, 4, 4, device="cuda"))         # not 4-D
    with pytest.raises(ValueError):
        utils.dissum_msp_score(torch.zeros(1, 1, 13, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        utils.dissum_msp_score(t, prob="entropy")
    from dmlnet._lib import DmlError
    with pytest.raises(DmlError):
        utils.dissum_msp_score(t, first_class=13)
    with pytest.raises(DmlError):
        utils.dissum_msp_score(torch.zeros(1, 33, 4, 4, device="cuda"))


def test_driver_confidence_branch():
    import eval_ood_traditional as T
    import utils
    lg, ref = MC.reference("kfirst_vec_softmax")
    scores = torch.from_numpy(np.array(lg)).cuda()
    for exclude_back in (False, True):
        want = utils.dissum_msp_score(scores, clip=400.0, threshold=0.2, slope=50.0, first_class=1 if exclude_back else 0)[0]
        conf = T.confidence(scores, "dissum_msp", exclude_back)
        assert conf.is_cuda and conf.shape == want.shape and torch.equal(conf, want)
    check("driver --exclude_back", T.confidence(scores, "dissum_msp", True)[None].cpu().numpy(), ref)
    # the other branches are what they were on the same tensor
    for exclude_back in (False, True):
        tmp = scores[:, 1:].contiguous() if exclude_back else scores
        assert torch.equal(T.confidence(scores, "dissum", exclude_back), utils.dissum_score(tmp, clip=400.0, inclusive=True)[0])
        assert torch.equal(T.confidence(scores, "msp", exclude_back), utils.argmax_msp(tmp)[1][0])
        assert torch.equal(T.confidence(scores, "maxlogit", exclude_back), tmp.max(dim=1)[0][0])
        assert torch.equal(T.confidence(scores, "background", exclude_back), tmp[0, 0])
    # the gate's settings reach the kernel from where main() leaves them
    saved = dict(T.MIX)
    try:
        T.MIX.update(threshold=0.3, slope=20.0)
        want = utils.dissum_msp_score(scores, clip=400.0, threshold=0.3, slope=20.0)[0]
        assert torch.equal(T.confidence(scores, "dissum_msp"), want)
    finally:
        T.MIX.update(saved)


def test_open_set_evaluation_driver_dissum_msp():
    """eval_ood_traditional.py --ood dissum_msp end to end at a small frame size"""
    drv = os.path.join(H.PKG, "eval_ood_traditional.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--ood", "dissum_msp", "--num_images", "1", "--height", "360",
                        "--width", "640", "--dtype", "bf16"], capture_output=True, text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean auroc = " in r.stdout and "Mean IoU:" in r.stdout
    auroc = float(r.stdout.split("mean auroc = ")[1].split()[0])
    assert 0.0 <= auroc <= 1.0
