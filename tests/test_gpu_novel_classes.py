"""GPU: several few-shot novel classes in one open-world pass -- dml_open_world_post, dml_novel_relabel_multi and
dml_class_feature_sums (csrc/scores.hip, csrc/eval_sums.hip) through the C ABI and through utils.

Every comparison is against the float64 definitions of tests/novel_cases.py and tests/open_set_cases.py on the same
float32 inputs (proved to be the reference's rules, without a GPU, by tests/test_novel_refs.py).  Predictions are compared
exactly on every pixel whose fp64 decision margin is above the fp32 bound (the share left out is capped at
open_set_cases.EXCLUDE_CAP; the exact rows leave nothing out); MSP, score and feature sums against the bars the existing
kernels are held to.  Each float check prints "MEASURE <what> err=<largest error> bar=<bar>" before it asserts.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import novel_cases as NC
import open_set_cases as CS

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
F64 = np.float64


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def check_le(what, err, bar):
    err = float(err)
    print("MEASURE %s err=%.3e bar=%.3e" % (what, err, bar))
    assert err <= bar, "%s: error %.3e above the bar %.3e" % (what, err, bar)


def run_post(lib, lg, feats, protos, labels, thresh, vs_known, clip=1000.0, inclusive=False, want_msp=True,
             want_score=True):
    """dml_open_world_post on host arrays -> preds, msp, score, work as numpy (None where not asked for)"""
    B, K, Hh, Ww = lg.shape
    N = 0 if protos is None else len(protos)
    C = feats.shape[-1] if feats is not None else 1
    l, f = dev(lg), (dev(feats) if N else None)
    p, nl = (dev(protos) if N else None), (dev(np.asarray(labels, np.int64)) if N else None)
    preds = torch.full((B, Hh, Ww), -7, dtype=torch.int64, device="cuda")
    msp = torch.full((B, Hh, Ww), float("nan"), dtype=torch.float32, device="cuda") if want_msp else None
    score = torch.full((B, Hh, Ww), 7.0, dtype=torch.float32, device="cuda") if want_score else None
    work = torch.full((2 * B,), 7.0, dtype=torch.float32, device="cuda") if want_score else None
    rc = lib.dml_open_world_post(l.data_ptr(), ptr(f), ptr(p), ptr(nl), preds.data_ptr(), ptr(msp), ptr(score), ptr(work),
                                 B, C, K, Hh, Ww, N, float(thresh), 1 if vs_known else 0, float(clip),
                                 1 if inclusive else 0, st())
    assert rc == 0, "dml_open_world_post returned %d" % rc
    return tuple(None if t is None else t.cpu().numpy() for t in (preds, msp, score, work))


def check_preds(what, got, ref, exact=False):
    sure = np.ones(ref["sure"].shape, bool) if exact else ref["sure"]
    excluded = int((~sure).sum())
    print("MEASURE %s excluded=%d of %d" % (what, excluded, sure.size))
    assert excluded <= CS.EXCLUDE_CAP * sure.size
    bad = np.flatnonzero((got != ref["preds"]) & sure)
    assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:8]], ref["preds"].ravel()[bad[:8]])


def check_msp(what, msp, lg):
    _, rm = CS.msp_ref(lg)
    check_le("msp " + what, np.abs(msp.astype(F64) - rm).max(), CS.msp_bar(lg.shape[1]))


def check_score(what, score, work, lg, clip, inclusive):
    """the checks of the dml_dissum_score test: range found, NaN for a constant image, normalised score"""
    got, w = score.astype(F64), work.astype(F64)
    for b in range(lg.shape[0]):
        ref, s = CS.dissum_ref(lg[b], clip, inclusive)
        bar, max_err = CS.dissum_bar(lg[b], clip, inclusive)
        tag = "%s img %d" % (what, b)
        check_le("dissum min " + tag, abs(w[2 * b] - s.min()), 2 * max_err)
        check_le("dissum max " + tag, abs(w[2 * b + 1] - s.max()), 2 * max_err)
        if s.max() == s.min():
            assert np.isnan(got[b]).all()
            continue
        assert not np.isnan(got[b]).any()
        check_le("dissum " + tag, np.abs(got[b] - ref).max(), bar)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# dml_open_world_post
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NC.RANDOM_NS)
def test_post_random_batch(lib, N):
    """2 x 96 x 160, C = K = 16 (the register path): predictions outside the margin, MSP and score to their bars, through
    the C ABI and through utils"""
    import utils
    feats, lg, protos, labels = NC.random_batch(N)
    for vs_known in (True, False):
        ref = NC.post_ref(lg, feats, protos, labels, -1.5, vs_known)
        preds, msp, score, work = run_post(lib, lg, feats, protos, labels, -1.5, vs_known)
        what = "random N=%d vs_known=%d" % (N, vs_known)
        check_preds(what, preds, ref)
        check_msp(what, msp, lg)
        check_score(what, score, work, lg, 1000.0, False)
        p2, m2, s2 = utils.open_world_post(dev(lg), dev(feats), protos, labels, vs_known=vs_known)
        assert np.array_equal(p2.cpu().numpy(), preds) and np.array_equal(m2.cpu().numpy(), msp)
        assert np.array_equal(s2.cpu().numpy(), score)
    # a tensor of prototypes, the other clip rule, no score wanted
    p3, m3, s3 = utils.open_world_post(dev(lg), dev(feats), dev(protos), labels, clip=400.0, inclusive=True, want_msp=False)
    assert m3 is None and np.array_equal(p3.cpu().numpy(), run_post(lib, lg, feats, protos, labels, -1.5, True)[0])
    check_le("score clip 400 N=%d" % N, np.abs(s3[0].cpu().numpy().astype(F64) - CS.dissum_ref(lg[0], 400.0, True)[0]).max(),
             CS.dissum_bar(lg[0], 400.0, True)[0])


@pytest.mark.parametrize("K", (16, 19))
@pytest.mark.parametrize("C", (3, 16, NC.CS.MAXC))
def test_post_exact_row(lib, C, K):
    """dyadic distances, exact in fp32: a two-way tie for the top, d* on the threshold and one ulp either side, d* on the
    max logit, a prototype that wins only with vs_known = 0; image 1 reversed.  No pixel is left out.  The row has 8 pixels
    (16-byte path) and, cut to 7, goes through the one-pixel-per-lane path."""
    feats, lg, protos, labels, what = NC.exact_row(C, K)
    for n in (8, 7):
        f, l = np.ascontiguousarray(feats[:, :, :n]), np.ascontiguousarray(lg[:, :, :, :n])
        for th in NC.EXACT_THRESHOLDS:
            for vs_known in (True, False):
                ref = NC.post_ref(l, f, protos, labels, th, vs_known)
                preds = run_post(lib, l, f, protos, labels, th, vs_known, want_msp=False, want_score=False)[0]
                assert np.array_equal(preds, ref["preds"]), (n, float(th), vs_known, preds, ref["preds"])
    preds = run_post(lib, lg, feats, protos, labels, -1.5, True, want_msp=False, want_score=False)[0]
    assert preds[0, 0, what["tie"]] == np.argmax(lg[0, :, 0, what["tie"]])           # the tie keeps its known class


@pytest.mark.parametrize("K", CS.RELABEL_KS)
@pytest.mark.parametrize("C", CS.RELABEL_CS)
def test_post_one_prototype_exact_boundaries(lib, C, K):
    """the exact row of dml_novel_relabel's test with N = 1: the same pixels are relabelled, on top of the argmax"""
    feats, lg, proto, _, expect = CS.relabel_exact(C, K, 16)
    base = np.argmax(lg, axis=1)
    for th, idx in expect.items():
        preds = run_post(lib, lg, feats, proto[None], [16], th, True, want_msp=False, want_score=False)[0]
        want = base.copy()
        want[0, 0, idx] = 16
        want[1, 0, [lg.shape[-1] - 1 - i for i in idx]] = 16
        assert np.array_equal(preds, want), (th, preds, want)


def test_post_odd_shapes(lib):
    """H W not a multiple of 4 (one pixel per lane), C in 1 / 13 / 32, K in 1 / 13 / 19 / 32, N in 0 / 1 / 3"""
    for shape in NC.ODD_SHAPES:
        for C in NC.ODD_CS:
            for K in NC.ODD_KS:
                for N in NC.ODD_NS:
                    feats, lg, protos, labels = NC.random_batch(N, C, K, shape)
                    vs_known = (C + K + N) % 2 == 0
                    ref = NC.post_ref(lg, feats, protos, labels, -1.5, vs_known)
                    preds, msp, score, work = run_post(lib, lg, feats, protos, labels, -1.5, vs_known)
                    bad = (preds != ref["preds"]) & ref["sure"]
                    assert not bad.any(), (shape, C, K, N)
                    assert np.abs(msp.astype(F64) - CS.msp_ref(lg)[1]).max() <= CS.msp_bar(K)
                    check_score("odd %s C=%d K=%d N=%d" % (shape, C, K, N), score, work, lg, 1000.0, False)


def test_post_generic_vector_path(lib):
    """H W % 4 == 0 without C = K = 16: 16-byte logit loads, runtime C and K; more than one workgroup per image"""
    for C, K, N in ((12, 19, 3), (32, 33, 8), (16, 13, 2), (13, 16, 2), (1, 16, 1)):
        feats, lg, protos, labels = NC.random_batch(N, C, K, (2, 36, 44))
        ref = NC.post_ref(lg, feats, protos, labels, -1.5, True)
        preds, msp, score, work = run_post(lib, lg, feats, protos, labels, -1.5, True)
        check_preds("generic C=%d K=%d N=%d" % (C, K, N), preds, ref)
        check_msp("generic C=%d K=%d" % (C, K), msp, lg)
        check_score("generic C=%d K=%d" % (C, K), score, work, lg, 1000.0, False)


def _three_calls(lg, feats, proto, thresh):
    import utils
    l, f = dev(lg), dev(feats)
    preds, msp = utils.argmax_msp(l)
    score = utils.dissum_score(l, clip=1000.0, inclusive=False)
    preds = utils.novel_relabel(preds, l, f, proto, thresh, 16)
    return preds.cpu().numpy(), msp.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("shape", CS.MSP_SHAPES)
def test_post_one_prototype_is_the_three_calls(lib, shape):
    """N = 1: argmax_msp + dissum_score + novel_relabel on the same inputs.  The sums run in the same order, so MSP and
    score are held to their bars twice over (each against fp64) and predictions are equal outside the margin."""
    for K in (13, 16):
        feats, lg, protos, labels = NC.random_batch(1, 16, K, shape)
        ref = NC.post_ref(lg, feats, protos, [16], -1.5, True)
        preds, msp, score, _ = run_post(lib, lg, feats, protos, [16], -1.5, True)
        p3, m3, s3 = _three_calls(lg, feats, protos[0], -1.5)
        assert np.array_equal(preds[ref["sure"]], p3[ref["sure"]])
        assert np.abs(msp.astype(F64) - m3).max() <= 2 * CS.msp_bar(K)
        if shape != (1, 1, 1):
            for b in range(shape[0]):
                assert np.abs(score[b].astype(F64) - s3[b]).max() <= 2 * CS.dissum_bar(lg[b], 1000.0, False)[0]


def test_post_full_image_is_the_three_calls(lib):
    """1 x 1024 x 2048, K = C = 16 (MSP_BIG): the capped grid walks several pixel groups per lane"""
    K, shape = CS.MSP_BIG
    lg = CS.msp_logits("dist", K, shape)
    rs = np.random.RandomState(77)
    proto = rs.standard_normal(16).astype(np.float32)
    feats = rs.standard_normal(shape + (16,)).astype(np.float32)
    feats *= rs.uniform(0.05, 0.6, shape + (1,)).astype(np.float32)
    feats += proto
    ref = NC.post_ref(lg, feats, proto[None], [16], -1.5, True)
    assert 0.2 < ref["hit"].mean() < 0.8
    preds, msp, score, work = run_post(lib, lg, feats, proto[None], [16], -1.5, True)
    check_preds("full image", preds, ref)
    check_msp("full image", msp, lg)
    p3, _, _ = _three_calls(lg, feats, proto, -1.5)
    assert np.array_equal(preds[ref["sure"]], p3[ref["sure"]])
    check_score("full image", score, work, lg, 1000.0, False)


@pytest.mark.parametrize("clip,inclusive", CS.DISSUM_MODES)
def test_post_dissum_edges(lib, clip, inclusive):
    """the signed-zero and on-clip cases of dml_dissum_score's test, with the same expectations"""
    def scores(lg):
        _, _, score, work = run_post(lib, lg, None, None, None, -1.5, True, clip, inclusive)
        return check_score("edges clip=%g" % clip, score, work, lg, clip, inclusive)

    got = scores(CS.dissum_signed_zero(False))
    assert got[0].ravel()[5] == 1.0 and got[0].ravel()[0] == 0.0
    z = CS.dissum_signed_zero(True)
    got = scores(z)
    assert got[0].ravel()[-1] == 1.0 and got[0].ravel()[0] == 0.0
    got = scores(np.concatenate([CS.dissum_flat(4, z.shape[-1]), z]))
    assert got[1].ravel()[-1] == 1.0 and got[1].ravel()[0] == 0.0
    for K in CS.DISSUM_KS:
        lg = CS.dissum_on_clip(K)
        got = scores(lg)
        s = -lg[0].astype(F64).sum(axis=0).ravel()
        assert (got[0].ravel()[s >= clip] == 1.0).all()
        got = scores(CS.dissum_all_clip_but_one(K))
        assert (got[0].ravel() == 1.0).sum() == got[0].size - 1 and got[0].ravel()[41] == 0.0
    const = np.full((2, 4, 8, 8), -2.0, np.float32)
    const[1, :, 3, 3] = -1.0
    got = scores(const)
    assert np.isnan(got[0]).all() and got[1].max() == 1.0 and got[1].min() == 0.0


def test_post_null_outputs_leave_the_others_unchanged(lib):
    feats, lg, protos, labels = NC.random_batch(3, 16, 16, (2, 12, 20))
    for case in ((feats, lg, protos, labels), NC.random_batch(2, 13, 19, (3, 5, 7))):
        f, l, p, nl = case
        full = run_post(lib, l, f, p, nl, -1.5, True)
        no_msp = run_post(lib, l, f, p, nl, -1.5, True, want_msp=False)
        no_score = run_post(lib, l, f, p, nl, -1.5, True, want_score=False)
        neither = run_post(lib, l, f, p, nl, -1.5, True, want_msp=False, want_score=False)
        assert no_msp[1] is None and no_score[2] is None
        for other in (no_msp, no_score, neither):
            assert np.array_equal(other[0], full[0])
        assert np.array_equal(no_msp[2], full[2]) and np.array_equal(no_msp[3], full[3])
        assert np.array_equal(no_score[1], full[1])


def test_post_error_codes(lib):
    """argument checks that return before any launch"""
    a = torch.zeros(4096, dtype=torch.float32, device="cuda")
    i8 = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    A, I = a.data_ptr(), i8.data_ptr()

    def call(lg=A, f=A, p=A, nl=I, preds=I, msp=A, score=A, work=A, B=1, C=16, K=16, Hh=2, Ww=2, N=1):
        return lib.dml_open_world_post(lg, f, p, nl, preds, msp, score, work, B, C, K, Hh, Ww, N, -1.5, 1, 1000.0, 0, st())

    assert call(C=0) == EINVAL and call(K=0) == EINVAL and call(N=-1) == EINVAL
    assert call(C=CS.MAXC + 1) == EUNSUPPORTED and call(K=34) == EUNSUPPORTED and call(N=NC.MAXN + 1) == EUNSUPPORTED
    assert call(lg=None) == EINVAL and call(preds=None) == EINVAL and call(work=None) == EINVAL
    assert call(f=None) == EINVAL and call(p=None) == EINVAL and call(nl=None) == EINVAL
    assert call(Hh=0) == EINVAL and call(Ww=0) == EINVAL and call(B=0) == EINVAL
    assert call(B=65536) == EUNSUPPORTED and call(B=2, Hh=2 ** 20, Ww=2 ** 20) == EUNSUPPORTED

    def multi(f=A, lg=A, p=A, nl=I, preds=I, C=16, K=16, N=1):
        return lib.dml_novel_relabel_multi(f, lg, p, nl, preds, 1, C, K, 2, 2, N, -1.5, 1, st())

    assert multi(C=33) == EUNSUPPORTED and multi(N=9) == EUNSUPPORTED and multi(K=0) == EINVAL
    assert multi(f=None) == EINVAL and multi(preds=None) == EINVAL
    torch.cuda.synchronize()
    assert (i8.cpu().numpy() == -7).all() and (a.cpu().numpy() == 0.0).all()        # nothing ran
    # N = 0 without features and prototypes is a plain argmax
    assert call(f=None, p=None, nl=None, msp=None, score=None, work=None, N=0) == 0
    torch.cuda.synchronize()
    assert (i8[:4].cpu().numpy() == 0).all() and (i8[4:].cpu().numpy() == -7).all()


def test_novel_relabel_multi_in_place(lib):
    """given predictions (some 255, some already a novel label): only relabelled pixels change"""
    import utils
    for N, C, K, shape in ((3, 16, 16, (2, 96, 160)), (2, 13, 19, (3, 5, 7)), (8, 32, 16, (1, 20, 20))):
        feats, lg, protos, labels = NC.random_batch(N, C, K, shape)
        rs = np.random.RandomState(N)
        given = rs.randint(0, K, shape).astype(np.int64)
        given[rs.rand(*shape) < 0.05] = 255
        given[rs.rand(*shape) < 0.05] = labels[0]
        for vs_known in (True, False):
            ref = NC.post_ref(lg, feats, protos, labels, -1.5, vs_known)
            want = np.where(ref["hit"], ref["preds"], given)
            t = dev(given).clone()
            out = utils.novel_relabel_multi(t, dev(lg), dev(feats), protos, labels, -1.5, vs_known)
            assert out.data_ptr() == t.data_ptr()
            got = out.cpu().numpy()
            assert np.array_equal(got[ref["sure"]], want[ref["sure"]])
            assert (~ref["sure"]).sum() <= CS.EXCLUDE_CAP * ref["sure"].size
    # one prototype against the known classes: dml_novel_relabel
    feats, lg, proto, preds = CS.relabel_random()
    a = utils.novel_relabel(dev(preds).clone(), dev(lg), dev(feats), proto, -1.5, 16).cpu().numpy()
    b = utils.novel_relabel_multi(dev(preds).clone(), dev(lg), dev(feats), proto[None], [16], -1.5, True).cpu().numpy()
    sure = NC.post_ref(lg, feats, proto[None], [16], -1.5, True)["sure"]
    assert np.array_equal(a[sure], b[sure])


# ---------------------------------------------------------------------------------------------------------------------
# dml_class_feature_sums / extract_prototypes
# ---------------------------------------------------------------------------------------------------------------------
def _fsums(lib, f, lab, ids):
    fd, ld, cd = dev(f), dev(lab), dev(np.asarray(ids, np.int64))
    M, Cc = len(ids), f.shape[1]
    sums = torch.full((M, Cc), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((M,), 7, dtype=torch.int64, device="cuda")
    rc = lib.dml_class_feature_sums(fd.data_ptr(), ld.data_ptr(), f.shape[0], Cc, cd.data_ptr(), M, sums.data_ptr(),
                                    cnt.data_ptr(), st())
    assert rc == 0, rc
    return sums.cpu().numpy(), cnt.cpu().numpy()


def _check_fsums(lib, f, lab, ids, what):
    got, n = _fsums(lib, f, lab, ids)
    for m, c in enumerate(ids):
        ref, abs_sum, rn = CS.fsum_ref(f, lab, c)
        assert n[m] == rn                                                    # counts exact
        if rn == 0:
            assert (got[m] == 0.0).all()                                     # a class with no pixel: exactly 0
            continue
        check_le("feature sums %s C=%d n_px=%d class %d (relative to sum|f|)" % (what, f.shape[1], f.shape[0], c),
                 (np.abs(got[m] - ref) / abs_sum).max(), CS.fsum_bar(f.shape[0], 1.0))
    return got, n


@pytest.mark.parametrize("n_px", CS.FSUM_NPX + (70001,))
@pytest.mark.parametrize("Cc", CS.FSUM_CS + (13,))
def test_class_feature_sums(lib, Cc, n_px):
    """the inputs and the bar of dml_class_feature_sum's test (2 ceil(n_px / 262144) eps32 relative to sum |f| of the
    class): several classes at once, one of them absent, one on a single pixel; M = 1 against the existing entry point;
    M = 8"""
    f, lab = CS.fsum_inputs(Cc, n_px)
    got, n = _check_fsums(lib, f, lab, [0, 1, 3, 4], "mixed")
    assert n[3] == 1 and np.array_equal(got[3], f[-1].astype(F64))            # one term: exact
    _check_fsums(lib, f, lab, [4, 2, 9, 1, 0, 3, 77, -1], "M=8")
    fd, ld = dev(f), dev(lab)
    for c in (1, 3):
        one, n1 = _check_fsums(lib, f, lab, [c], "M=1")
        sums = torch.full((Cc,), 7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        assert lib.dml_class_feature_sum(fd.data_ptr(), ld.data_ptr(), n_px, Cc, c, sums.data_ptr(), cnt.data_ptr(), st()) == 0
        assert int(cnt.item()) == n1[0]
        abs_sum = CS.fsum_ref(f, lab, c)[1]
        if n1[0]:
            check_le("M=1 vs dml_class_feature_sum C=%d n_px=%d" % (Cc, n_px),
                     (np.abs(one[0] - sums.cpu().numpy()) / abs_sum).max(), 2 * CS.fsum_bar(n_px, 1.0))
    _check_fsums(lib, f, np.full(n_px, 6, np.int64), [5, 6], "every pixel")


def test_class_feature_sums_many_terms_per_thread(lib):
    """4 x 768 x 768 pixels, C = 16: the capped grid gives every thread up to 9 fp32 terms before the fp64 finish"""
    f, lab = CS.fsum_inputs(16, 4 * 768 * 768)
    _check_fsums(lib, f, lab, [1, 3, 4, 0, 2], "capped grid")


def test_class_feature_sums_error_codes(lib):
    a = torch.zeros(64, dtype=torch.float32, device="cuda")
    l = torch.zeros(8, dtype=torch.int64, device="cuda")
    s = torch.zeros(8 * 32, dtype=torch.float64, device="cuda")

    def call(f=a.data_ptr(), n_px=2, Cc=16, ids=l.data_ptr(), M=1):
        return lib.dml_class_feature_sums(f, l.data_ptr(), n_px, Cc, ids, M, s.data_ptr(), l.data_ptr(), st())

    assert call(Cc=CS.MAXC + 1) == EINVAL and call(Cc=0) == EINVAL and call(n_px=0) == EINVAL
    assert call(M=0) == EINVAL and call(M=9) == EINVAL and call(f=None) == EINVAL and call(ids=None) == EINVAL


def test_extract_prototypes(lib):
    """the 5 % rule per class, one dictionary for all classes, duplicates refused with DML_EINVAL's error"""
    import utils
    from dmlnet._lib import DmlError
    f, lab = CS.fsum_inputs(16, 2000)
    lab[:] = 0
    lab[100:200] = 9                                                         # exactly 5 %: `<=` -> None
    lab[300:401] = 11                                                        # one pixel above
    lab[-1] = 4
    fd, ld = dev(f).view(1, 40, 50, 16), dev(lab).view(40, 50)
    got = utils.extract_prototypes(fd, ld, [9, 3, 4, 11, 0])
    assert list(got) == [9, 3, 4, 11, 0]
    assert got[9] is None and got[3] is None and got[4] is None
    for c in (11, 0):
        ref, abs_sum, n = CS.fsum_ref(f, lab, c)
        mean = ref / n
        bar = CS.fsum_bar(2000, abs_sum) / n + CS.EPS32 * np.abs(mean)       # the sum's bar over n + the rounding to float32
        check_le("prototype mean class %d (worst err / bar)" % c, (np.abs(np.array(got[c], F64) - mean) / bar).max(), 1.0)
        single = utils.extract_prototype(fd, ld, c)
        check_le("vs extract_prototype class %d (worst err / bar)" % c,
                 (np.abs(np.array(got[c], F64) - np.array(single, F64)) / (2 * bar)).max(), 1.0)
    with pytest.raises(DmlError, match=r"invalid argument \(code -1\)"):
        utils.extract_prototypes(fd, ld, [9, 11, 9])


# ---------------------------------------------------------------------------------------------------------------------
# end to end: model -> shots -> JSON -> prototypes -> one pass
# ---------------------------------------------------------------------------------------------------------------------
def test_shots_to_predictions_end_to_end(lib, tmp_path):
    import network
    import utils
    m = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
    m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=1))
    m.cuda().eval()
    ids = (13, 14, 15)
    shots = {c: [] for c in ids}
    frames = []
    with torch.no_grad():
        for i in range(2):
            img = H.synth_tensor(40 + i, "novel.img", (1, 3, 128, 256)).cuda()
            # blocky label map: 32 x 32 blocks cycling through 12 .. 15, each a quarter of the frame
            yy, xx = np.meshgrid(np.arange(128) // 32, np.arange(256) // 32, indexing="ij")
            lab = dev((12 + (yy + xx + i) % 4).astype(np.int64))[None]
            lg, _, ft = m(img)
            lg, ft = lg.float().contiguous(), ft.float().contiguous()
            for c, shot in utils.extract_prototypes(ft, lab, ids).items():
                assert shot is not None and len(shot) == 16
                shots[c].append(shot)
            # each shot is the masked mean of the features it came from
            fh, lh = ft.cpu().numpy().reshape(-1, 16), lab.cpu().numpy().reshape(-1)
            for c in ids:
                ref, abs_sum, n = CS.fsum_ref(fh, lh, c)
                bar = CS.fsum_bar(fh.shape[0], abs_sum) / n + CS.EPS32 * np.abs(ref / n)
                assert (np.abs(np.array(shots[c][-1], F64) - ref / n) <= bar).all()
            frames.append((lg, ft))
    protos = []
    for c in ids:
        path = tmp_path / ("prototype_%d.json" % c)
        path.write_text(json.dumps(shots[c]))
        protos.append(utils.mean_prototype(json.loads(path.read_text())))
    protos = np.stack(protos)
    labels = [16, 17, 18]
    hits = 0
    for lg, ft in frames:
        lgh, fth = lg.cpu().numpy(), ft.cpu().numpy()
        p32 = protos.astype(np.float32)                                      # what the wrapper hands to the kernel
        dstar = NC.post_ref(lgh, fth, p32, labels, -np.inf, False)
        # a threshold that half of the pixels pass, whatever scale the random-init features have
        d = np.stack([-((fth.astype(F64) - p.astype(F64)) ** 2).sum(-1) for p in p32], -1).max(-1)
        thresh = float(np.float32(np.median(d)))
        for vs_known in (False, True):
            ref = NC.post_ref(lgh, fth, p32, labels, thresh, vs_known)
            preds, msp, score = utils.open_world_post(lg, ft, protos, labels, thresh=thresh, vs_known=vs_known)
            check_preds("end to end vs_known=%d" % vs_known, preds.cpu().numpy(), ref)
            check_msp("end to end", msp.cpu().numpy(), lgh)
            assert np.isfinite(score.cpu().numpy()).all()
            hits += int(ref["hit"].sum())
        assert dstar["hit"].any()
    assert hits > 0


# ---------------------------------------------------------------------------------------------------------------------
# the driver: shots written, read back, 19 classes; one and two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _driver(args, ranks=1):
    drv = os.path.join(H.PKG, "eval_open_world.py")
    cmd = [sys.executable, drv]
    env = dict(os.environ)
    if ranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), drv]
        env.update(DML_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd + ["--synthetic", "--height", "256", "--width", "512", "--num_images", "4", "--dtype", "f32"] + args,
                       env=env, capture_output=True, text=True, cwd=H.PKG, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _table(text):
    """the scalar scores and the per-class lines of the driver's output"""
    scores, classes = {}, {}
    for ln in text.splitlines():
        for key in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
            if ln.startswith(key + ":"):
                scores[key] = float(ln.split(":")[1])
        parts = ln.split(":")
        if ln.startswith("  ") and len(parts) == 2 and parts[0].strip().isdigit():
            classes[int(parts[0])] = float(parts[1])
    return scores, classes


def test_driver_extracts_shots_and_evaluates_nineteen_classes(tmp_path):
    """eval_open_world.py end to end on four synthetic 256 x 512 frames: --extract_prototypes writes one file per class
    with one shot per frame in which the class covers more than 5 % (counted here from the driver's seeded label maps),
    the same files on two ranks; the same command reads them back and prints a 19-class table, the same on two ranks."""
    ids = (13, 14, 15)
    want = {c: 0 for c in ids}
    for i in range(4):                                                       # the driver's synthetic target of frame i
        g = torch.Generator().manual_seed(4321 + i)
        torch.randn(1, 3, 256, 512, generator=g)
        coarse = torch.randint(0, 17, (1, 4, 8), generator=g)
        for c in ids:
            want[c] += int((coarse == c).float().mean().item() > 0.05)
    assert all(want[c] >= 1 for c in ids), want
    files = {}
    for ranks in (1, 2):
        out = tmp_path / ("shots%d" % ranks)
        _driver(["--extract_prototypes"] + [str(c) for c in ids] + ["--shots_out", str(out)], ranks)
        assert sorted(os.listdir(out)) == ["prototype_%d.json" % c for c in ids]
        files[ranks] = {c: json.loads((out / ("prototype_%d.json" % c)).read_text()) for c in ids}
        for c in ids:
            assert len(files[ranks][c]) == want[c] and all(len(shot) == 16 for shot in files[ranks][c])
    assert files[1] == files[2]                                              # frame order, whatever the number of ranks
    protos = [str(tmp_path / "shots1" / ("prototype_%d.json" % c)) for c in ids]
    s1, c1 = _table(_driver(["--prototype_json"] + protos))
    assert len(s1) == 4 and sorted(c1) == list(range(19))
    s2, c2 = _table(_driver(["--prototype_json"] + protos, 2))
    assert sorted(c2) == list(range(19))
    for k in s1:
        assert abs(s1[k] - s2[k]) <= 1e-6, (k, s1[k], s2[k])
