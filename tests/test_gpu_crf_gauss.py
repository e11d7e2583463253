"""GPU: the Gaussian dense-CRF confidence -- dml_crf_gauss (csrc/crf_gauss.hip) through the C ABI, through
utils.dense_crf_gauss and through the open-set driver's `--ood crf-gauss`.

Every float comparison is against the float64 definition of tests/crf_cases.py on the same float32 inputs, on EVERY pixel:
|conf - conf64| <= 1e-5, and `map` equal wherever the two largest float64 marginals are at least 1e-4 apart
(tests/test_crf_refs.py shows, without a GPU, that a float32 numpy run of the definition stays within 1/8 of that bar and that
at most 1 % of the pixels of any case are such near-ties).  Each check prints "MEASURE <case> err=... bar=..." before it
asserts.  conf, map and the workspace's end sit between guard elements that must come back untouched.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_cases as CC
import helpers as H

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
F64 = np.float64
GUARD = 64                       # elements before and after each output


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def run(lib, lg, case, offset=0, k_first=None, compat=None, iters=None, want_map=True):
    """dml_crf_gauss on a host array -> (conf [B, H, W] float32, map [B, H, W] int64) as numpy.  `offset` shifts the
    logits pointer by that many floats."""
    B, K, Hh, Ww = lg.shape
    k_first = case["k_first"] if k_first is None else k_first
    compat = case["compat"] if compat is None else compat
    iters = case["iters"] if iters is None else iters
    lbuf = torch.zeros(lg.size + offset, dtype=torch.float32, device="cuda")
    lbuf[offset:] = torch.from_numpy(np.array(lg).ravel()).cuda()
    n = B * Hh * Ww
    cbuf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    cbuf[GUARD:GUARD + n] = float("nan")
    mbuf = torch.full((n + 2 * GUARD,), -7, dtype=torch.int64, device="cuda")
    nbytes = lib.dml_crf_gauss_workspace_bytes(B, K - k_first, Hh, Ww)
    assert nbytes == 4 * (3 * B * (K - k_first) * Hh * Ww + Hh + Ww + 256)
    work = torch.full((nbytes + 4 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.dml_crf_gauss(lbuf.data_ptr() + 4 * offset, cbuf.data_ptr() + 4 * GUARD,
                           mbuf.data_ptr() + 8 * GUARD if want_map else None, work.data_ptr(), B, K, Hh, Ww, k_first,
                           case["sx"], case["sy"], compat, iters, case["clip"], st())
    assert rc == 0, "dml_crf_gauss returned %d" % rc
    torch.cuda.synchronize()
    conf, lab = cbuf.cpu().numpy(), mbuf.cpu().numpy()
    assert (conf[:GUARD] == 7.0).all() and (conf[GUARD + n:] == 7.0).all(), "a guard element of conf was written"
    assert (lab[:GUARD] == -7).all() and (lab[GUARD + n:] == -7).all(), "a guard element of map was written"
    assert (work[nbytes:].cpu().numpy() == 0x5A).all(), "the workspace was written past dml_crf_gauss_workspace_bytes"
    if not want_map:
        assert (lab == -7).all()
    return conf[GUARD:GUARD + n].reshape(B, Hh, Ww), lab[GUARD:GUARD + n].reshape(B, Hh, Ww)


def check(what, got, ref):
    conf, lab = got
    assert np.isfinite(conf).all(), "%s: %d pixels not finite" % (what, (~np.isfinite(conf)).sum())
    err = np.abs(conf.astype(F64) - ref["conf"])
    off = (lab != ref["map"]) & ~ref["tie"]
    print("MEASURE %s err=%.3e bar=%.3e ties=%d of %d labels off outside ties=%d"
          % (what, err.max(), CC.GPU_BAR, ref["tie"].sum(), ref["tie"].size, off.sum()))
    bad = np.flatnonzero(err > CC.GPU_BAR)
    assert bad.size == 0, "%s: %d pixels above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], conf.ravel()[bad[:6]], ref["conf"].ravel()[bad[:6]])
    assert off.sum() == 0, "%s: %d labels differ outside the tie set" % (what, off.sum())
    assert lab.min() >= 0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_against_float64(lib, name):
    case = CC.CASES[name]
    lg, ref = CC.reference(name)
    got = run(lib, lg, case)
    check(name, got, ref)
    assert got[1].max() < case["shape"][1] - case["k_first"]
    if name in CC.BATCH_CASES:
        # image b of the batch equals the same image run alone, bitwise
        for b in range(lg.shape[0]):
            alone = run(lib, lg[b:b + 1], case)
            assert np.array_equal(bits(alone[0][0]), bits(got[0][b])), "image %d differs from its solo run" % b
            assert np.array_equal(alone[1][0], got[1][b])


def test_first_class_skips_the_background_without_a_copy(lib):
    """k_first = 1 on 14 classes: the same bits as the call on a contiguous copy of [:, 1:]"""
    case = CC.CASES["kfirst_it100"]
    lg, ref = CC.reference("kfirst_it100")
    got = run(lib, lg, case)
    copy = run(lib, np.ascontiguousarray(lg[:, 1:]), case, k_first=0)
    assert np.array_equal(bits(got[0]), bits(copy[0])) and np.array_equal(got[1], copy[1])
    other = np.array(lg)
    other[:, 0] = 1e30                                     # the background plane takes no part
    again = run(lib, other, case)
    assert np.array_equal(bits(got[0]), bits(again[0])) and np.array_equal(got[1], again[1])


def test_compat_zero_equals_no_iterations(lib):
    case = CC.CASES["plain_it5"]
    lg, _ = CC.reference("plain_it5")
    zero = run(lib, lg, case, compat=0.0)
    none = run(lib, lg, case, iters=0)
    assert np.array_equal(bits(zero[0]), bits(none[0])) and np.array_equal(zero[1], none[1])
    # iters = 0 is the maximum of the re-normalised clipped softmax
    p = np.clip(CC.softmax0(lg[0].astype(F64)), CC.CLIP, 1.0)
    want = (p / p.sum(axis=0)).max(axis=0)
    err = np.abs(none[0][0].astype(F64) - want).max()
    print("MEASURE plain iters=0 err=%.3e bar=%.3e" % (err, CC.GPU_BAR))
    assert err <= CC.GPU_BAR


def test_logits_pointer_offset_by_one_float(lib):
    case = CC.CASES["plain_it5"]
    lg, ref = CC.reference("plain_it5")
    got = run(lib, lg, case, offset=1)
    check("plain_it5 offset", got, ref)
    base = run(lib, lg, case)
    assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(got[1], base[1])


def test_two_runs_are_bitwise_identical_and_map_is_optional(lib):
    case = CC.CASES["plain_it100"]
    lg, _ = CC.reference("plain_it100")
    a, b = run(lib, lg, case), run(lib, lg, case)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    c = run(lib, lg, case, want_map=False)
    assert np.array_equal(bits(a[0]), bits(c[0]))


def test_vector_and_scalar_row_paths_agree(lib):
    """W % 4 == 0 takes 16-byte accesses in the row launch; a workspace moved by 4 bytes takes one float per lane"""
    case = CC.CASES["kfirst_it100"]
    lg, ref = CC.reference("kfirst_it100")
    B, K, Hh, Ww = lg.shape
    t = torch.from_numpy(np.array(lg)).cuda()
    nbytes = lib.dml_crf_gauss_workspace_bytes(B, K - 1, Hh, Ww)
    out = []
    for shift in (0, 4):
        conf = torch.empty(B * Hh * Ww, dtype=torch.float32, device="cuda")
        work = torch.full((nbytes + 4 + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        assert lib.dml_crf_gauss(t.data_ptr(), conf.data_ptr(), None, work.data_ptr() + shift, B, K, Hh, Ww, 1, 3.0, 3.0,
                                 3.0, 5, CC.CLIP, st()) == 0
        torch.cuda.synchronize()
        assert (work[shift + nbytes:].cpu().numpy() == 0x5A).all() and (work[:shift].cpu().numpy() == 0x5A).all()
        out.append(conf.cpu().numpy())
    assert np.array_equal(bits(out[0]), bits(out[1]))


def test_error_codes(lib):
    """argument checks that return before any launch; the limits themselves are accepted"""
    a = torch.full((32 * 64,), -7.0, dtype=torch.float32, device="cuda")
    o = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    m = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
    w = torch.full((1 << 16,), 7.0, dtype=torch.float32, device="cuda")
    A, O, M, Wk = a.data_ptr(), o.data_ptr(), m.data_ptr(), w.data_ptr()

    def call(lg=A, conf=O, lab=M, work=Wk, B=1, K=13, Hh=4, Ww=4, k_first=0, sx=3.0, sy=3.0, compat=3.0, iters=2, clip=1e-5):
        return lib.dml_crf_gauss(lg, conf, lab, work, B, K, Hh, Ww, k_first, sx, sy, compat, iters, clip, st())

    assert call(lg=None) == EINVAL and call(conf=None) == EINVAL and call(work=None) == EINVAL
    assert call(B=0) == EINVAL and call(K=0) == EINVAL and call(Hh=0) == EINVAL and call(Ww=0) == EINVAL
    assert call(B=-1) == EINVAL and call(K=-1) == EINVAL and call(Hh=-1) == EINVAL and call(Ww=-1) == EINVAL
    assert call(k_first=-1) == EINVAL and call(k_first=13) == EINVAL and call(k_first=14) == EINVAL
    assert call(iters=-1) == EINVAL
    assert call(sx=0.0) == EINVAL and call(sy=0.0) == EINVAL and call(sx=-1.0) == EINVAL and call(sy=float("nan")) == EINVAL
    assert call(clip=0.0) == EINVAL and call(clip=1.0) == EINVAL and call(clip=float("nan")) == EINVAL
    assert call(K=CC.MAX_CLASSES + 1) == EUNSUPPORTED and call(K=40, k_first=7) == EUNSUPPORTED
    assert call(sx=8.5) == EUNSUPPORTED and call(sy=8.5) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED
    assert call(B=2, Hh=2 ** 20, Ww=2 ** 20) == EUNSUPPORTED and call(B=1, Hh=2 ** 20 + 1, Ww=2 ** 20) == EUNSUPPORTED
    assert lib.dml_crf_gauss_workspace_bytes(1, 33, 4, 4) == EUNSUPPORTED
    assert lib.dml_crf_gauss_workspace_bytes(1, 13, 0, 4) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all() and (m.cpu().numpy() == -7).all()
    assert (w.cpu().numpy() == 7.0).all() and (a.cpu().numpy() == -7.0).all()
    # the limits themselves are accepted: 32 classes, 32 classes behind k_first, sigma 8, a NULL map
    assert call(K=CC.MAX_CLASSES, Hh=2, Ww=2) == 0
    assert call(K=40, k_first=8, Hh=2, Ww=2, sx=8.0, sy=8.0, lab=None) == 0
    torch.cuda.synchronize()
    out = o.cpu().numpy()
    assert np.abs(out[:4] - 1.0 / 32).max() < 1e-6 and np.isnan(out[4:]).all()       # constant logits: a uniform marginal
    assert (m.cpu().numpy()[:4] == 0).all() and (m.cpu().numpy()[4:] == -7).all()     # ... whose lowest index wins
    nfl = lib.dml_crf_gauss_workspace_bytes(1, 32, 2, 2) // 4
    assert (w[nfl:].cpu().numpy() == 7.0).all()


def test_utils_wrapper(lib):
    import utils
    for name in ("tiles_over_it5", "kfirst_it100", "aniso_it5"):
        case = CC.CASES[name]
        lg, ref = CC.reference(name)
        t = torch.from_numpy(np.array(lg)).cuda()
        sxy = case["sx"] if case["sx"] == case["sy"] else (case["sx"], case["sy"])
        conf, lab = utils.dense_crf_gauss(t, sxy=sxy, compat=case["compat"], iters=case["iters"],
                                          first_class=case["k_first"], return_map=True)
        assert conf.shape == ref["conf"].shape and conf.dtype == torch.float32 and conf.is_cuda
        assert lab.shape == ref["map"].shape and lab.dtype == torch.int64
        want = run(lib, lg, case)
        assert np.array_equal(bits(conf.cpu().numpy()), bits(want[0])) and np.array_equal(lab.cpu().numpy(), want[1])
        only = utils.dense_crf_gauss(t, sxy=sxy, compat=case["compat"], iters=case["iters"], first_class=case["k_first"])
        assert torch.is_tensor(only) and torch.equal(only, conf)
    # the defaults are the reference's: sxy 3, compat 3, 100 steps, every class
    lg, ref = CC.reference("plain_it100")
    t = torch.from_numpy(np.array(lg)).cuda()
    assert CC.CASES["plain_it100"]["compat"] == 3.0 and CC.CASES["plain_it100"]["sx"] == 3.0
    assert np.array_equal(bits(utils.dense_crf_gauss(t).cpu().numpy()), bits(run(lib, lg, CC.CASES["plain_it100"])[0]))
    with pytest.raises(RuntimeError):
        utils.dense_crf_gauss(torch.zeros(1, 13, 4, 4))                      # a CPU tensor: no fallback
    with pytest.raises(TypeError):
        utils.dense_crf_gauss(torch.zeros(1, 13, 4, 4, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError):
        utils.dense_crf_gauss(torch.zeros(13, 4, 4, device="cuda"))          # not 4-D
    from dmlnet._lib import DmlError
    with pytest.raises(DmlError):
        utils.dense_crf_gauss(t, first_class=13)
    with pytest.raises(DmlError):
        utils.dense_crf_gauss(torch.zeros(1, 33, 4, 4, device="cuda"))
    with pytest.raises(DmlError):
        utils.dense_crf_gauss(t, sxy=9.0)


def test_driver_confidence_branch():
    import eval_ood_traditional as T
    import utils
    lg, ref = CC.reference("kfirst_it100")
    scores = torch.from_numpy(np.array(lg)).cuda()
    for exclude_back in (False, True):
        want = utils.dense_crf_gauss(scores, sxy=3.0, compat=3.0, iters=100, first_class=1 if exclude_back else 0)[0]
        conf = T.confidence(scores, "crf-gauss", exclude_back)
        assert conf.is_cuda and conf.shape == want.shape and torch.equal(conf, want)
    got = T.confidence(scores, "crf-gauss", True)[None].cpu().numpy()
    err = np.abs(got.astype(F64) - ref["conf"]).max()
    print("MEASURE driver --exclude_back err=%.3e bar=%.3e" % (err, CC.GPU_BAR))
    assert err <= CC.GPU_BAR
    # the settings reach the kernel from where main() leaves them
    saved = dict(T.CRF)
    try:
        T.CRF.update(sxy=2.0, compat=1.5, iters=3)
        want = utils.dense_crf_gauss(scores, sxy=2.0, compat=1.5, iters=3)[0]
        assert torch.equal(T.confidence(scores, "crf-gauss"), want)
    finally:
        T.CRF.update(saved)


def test_open_set_evaluation_driver_crf_gauss():
    """eval_ood_traditional.py --synthetic --ood crf-gauss --crf_iters 3 end to end at a small frame size, in a child process"""
    drv = os.path.join(H.PKG, "eval_ood_traditional.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--ood", "crf-gauss", "--crf_iters", "3", "--num_images", "1",
                        "--height", "360", "--width", "640", "--dtype", "bf16"], capture_output=True, text=True, cwd=H.PKG,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean auroc = " in r.stdout and "Mean IoU:" in r.stdout
    line = r.stdout.split("mean auroc = ")[1].splitlines()[0]
    auroc = float(line.split()[0])
    aupr = float(line.split("mean aupr = ")[1].split()[0])
    fpr = float(line.split("mean fpr = ")[1].split()[0])
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in (auroc, aupr, fpr)), line
