"""GPU: the kNN cosine-similarity anomaly score -- dml_knn_cosine_score (csrc/knn_score.hip) through the C ABI, through
utils.knn_cosine_score and through the open-set driver's `--ood knn`.

Every comparison is against the float64 definition of tests/knn_cases.py on the same float32 inputs (proved to be the
reference's statements, without a GPU, by tests/test_knn_refs.py), on EVERY pixel, to the per-pixel bar
256 * 2^-24 * T(p) derived there; the C = 1 case must match exactly.  Each float check prints
"MEASURE <what> err=<largest error> bar=<largest bar>" before it asserts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import knn_cases as KC

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


def run(lib, feats, neighbor_size, offset=0):
    """dml_knn_cosine_score on a host array -> score [B, H, W] as numpy.  The output is pre-filled with NaN between two
    guards that must come back untouched; `offset` shifts the features pointer by that many floats."""
    B, C, Hh, Ww = feats.shape
    fbuf = torch.zeros(feats.size + offset, dtype=torch.float32, device="cuda")
    fbuf[offset:] = torch.from_numpy(np.array(feats).ravel()).cuda()          # a writable copy
    n = B * Hh * Ww
    obuf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    obuf[GUARD:GUARD + n] = float("nan")
    rc = lib.dml_knn_cosine_score(fbuf.data_ptr() + 4 * offset, obuf.data_ptr() + 4 * GUARD, B, C, Hh, Ww, neighbor_size,
                                  st())
    assert rc == 0, "dml_knn_cosine_score returned %d" % rc
    torch.cuda.synchronize()
    out = obuf.cpu().numpy()
    assert (out[:GUARD] == 7.0).all() and (out[GUARD + n:] == 7.0).all(), "a guard element was written"
    got = out[GUARD:GUARD + n].reshape(B, Hh, Ww)
    assert np.isfinite(got).all(), "%d outputs not written or not finite" % (~np.isfinite(got)).sum()
    return got


def check(what, got, score, T):
    err, bar = np.abs(got.astype(F64) - score), KC.bar(T)
    worst = (err / np.maximum(bar, 1e-300)).max()
    print("MEASURE %s err=%.3e bar=%.3e worst err/bar=%.3e" % (what, err.max(), bar.max(), worst))
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, "%s: %d pixels above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], got.ravel()[bad[:6]], score.ravel()[bad[:6]])


@pytest.mark.parametrize("name", sorted(KC.CASES))
def test_score_against_float64(lib, name):
    feats, score, T = KC.reference(name)
    ns = KC.CASES[name][1]
    got = run(lib, feats, ns)
    check(name, got, score, T)
    if name in ("one_pixel", "ns1"):
        assert not got.any()                                         # exactly 0: no neighbour / empty loops
    norms = np.sqrt((feats.astype(F64) ** 2).sum(axis=1))
    assert not got[norms == 0.0].any()                               # a zero vector scores exactly 0
    if name == "c1":
        assert np.array_equal(got.astype(F64), score)                # integers, exactly
    # two runs are bitwise equal
    again = run(lib, feats, ns)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # image b of the batch equals the same image run alone, bitwise
    if feats.shape[0] > 1:
        for b in range(feats.shape[0]):
            alone = run(lib, feats[b:b + 1], ns)
            assert np.array_equal(alone[0].view(np.uint32), got[b].view(np.uint32)), "image %d differs from its solo run" % b


@pytest.mark.parametrize("name", KC.OFFSET_CASES)
def test_features_pointer_offset_by_one_float(lib, name):
    """a features pointer that is not 16-byte aligned takes the one-float-per-lane path, whatever W is"""
    feats, score, T = KC.reference(name)
    ns = KC.CASES[name][1]
    got = run(lib, feats, ns, offset=1)
    check(name + " offset", got, score, T)
    # each output is a fixed-order sum over its own neighbourhood: the load path does not change a bit
    assert np.array_equal(got.view(np.uint32), run(lib, feats, ns).view(np.uint32))


def test_error_codes(lib):
    """argument checks that return before any launch"""
    a = torch.full((4096,), 7.0, dtype=torch.float32, device="cuda")
    o = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    A, O = a.data_ptr(), o.data_ptr()

    def call(f=A, s=O, B=1, C=13, Hh=4, Ww=4, ns=9):
        return lib.dml_knn_cosine_score(f, s, B, C, Hh, Ww, ns, st())

    assert call(f=None) == EINVAL and call(s=None) == EINVAL
    assert call(B=0) == EINVAL and call(C=0) == EINVAL and call(Hh=0) == EINVAL and call(Ww=0) == EINVAL
    assert call(B=-1) == EINVAL and call(C=-1) == EINVAL and call(Hh=-1) == EINVAL and call(Ww=-1) == EINVAL
    assert call(ns=0) == EINVAL and call(ns=-3) == EINVAL
    assert call(C=KC.MAXC + 1) == EUNSUPPORTED and call(ns=KC.MAX_NEIGHBOR_SIZE + 1) == EUNSUPPORTED
    assert call(B=65536) == EUNSUPPORTED
    assert call(B=2, Hh=2 ** 20, Ww=2 ** 20) == EUNSUPPORTED and call(B=1, Hh=2 ** 20 + 1, Ww=2 ** 20) == EUNSUPPORTED
    assert call(B=65535, Hh=2 ** 30, Ww=2 ** 30) == EUNSUPPORTED             # B H W beyond int64's comfort
    torch.cuda.synchronize()
    assert np.isnan(o.cpu().numpy()).all() and (a.cpu().numpy() == 7.0).all()        # nothing ran
    # the limits themselves are accepted
    assert call(C=KC.MAXC, Hh=2, Ww=2) == 0 and call(ns=KC.MAX_NEIGHBOR_SIZE, Hh=2, Ww=2) == 0
    torch.cuda.synchronize()
    assert np.isfinite(o[:4].cpu().numpy()).all() and np.isnan(o[4:].cpu().numpy()).all()


def test_utils_wrapper(lib):
    import utils
    for name in ("seams", "vec_ns4", "c32_big"):
        feats, score, T = KC.reference(name)
        ns = KC.CASES[name][1]
        t = torch.from_numpy(np.array(feats)).cuda()
        got = utils.knn_cosine_score(t, ns) if ns != 9 else utils.knn_cosine_score(t)
        assert got.shape == score.shape and got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy().view(np.uint32), run(lib, feats, ns).view(np.uint32))
    with pytest.raises(RuntimeError):
        utils.knn_cosine_score(torch.zeros(1, 13, 4, 4))                     # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        utils.knn_cosine_score(torch.zeros(13, 4, 4, device="cuda"))         # not 4-D
    with pytest.raises(ValueError):
        utils.knn_cosine_score(torch.zeros(1, 1, 13, 4, 4, device="cuda"))
    from dmlnet._lib import DmlError
    with pytest.raises(DmlError):
        utils.knn_cosine_score(torch.zeros(1, 13, 4, 4, device="cuda"), neighbor_size=18)


def test_driver_confidence_branch():
    import eval_ood_traditional as T
    import utils
    feats = KC.reference("vec_seams")[0]
    f = torch.from_numpy(np.array(feats)).cuda()
    scores = torch.randn(1, 14, feats.shape[2], feats.shape[3], device="cuda")
    want = utils.knn_cosine_score(f)[0]
    for exclude_back in (False, True):                               # --exclude_back does not touch this score
        conf = T.confidence(scores, "knn", exclude_back, feats=f)
        assert conf.is_cuda and conf.shape == want.shape and torch.equal(conf, want)
    with pytest.raises(ValueError):
        T.confidence(scores, "knn")
    # the other branches do not need the features
    assert torch.equal(T.confidence(scores, "background", feats=f), scores[0, 0])


def test_open_set_evaluation_driver_knn():
    """eval_ood_traditional.py --ood knn end to end at a small frame size"""
    drv = os.path.join(H.PKG, "eval_ood_traditional.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--ood", "knn", "--num_images", "1", "--height", "360", "--width",
                        "640", "--dtype", "bf16"], capture_output=True, text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean auroc = " in r.stdout and "Mean IoU:" in r.stdout
    auroc = float(r.stdout.split("mean auroc = ")[1].split()[0])
    assert 0.0 <= auroc <= 1.0
