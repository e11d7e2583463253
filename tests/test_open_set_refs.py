"""CPU: the references tests/test_gpu_open_set_scores.py compares the kernels with are themselves right on the edge
inputs of tests/open_set_cases.py -- so that a failure there means the kernel.

* oracle/ood_measures_ref.get_measures == live scikit-learn (2e-16) and == tests/golden/g11b_ood_edges.npz, minted from
  the reference's anom_utils.get_measures (FPR exactly), on every OOD case;
* oracle dissum_score / novel_relabel == the float64 formulas of the case table on the boundary cases;
* the random inputs leave at most 0.1 % of their pixels with a decision margin below the fp32 error bound.
"""
import os
import warnings

import numpy as np
import pytest

import helpers as H  # noqa: F401  (path setup)
import open_set_cases as CS
from oracle import dmlnet_ref as O
from oracle import metrics_ref as MR
from oracle import ood_measures_ref as OR

G11B = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11b_ood_edges.npz")


@pytest.fixture(scope="module")
def ood_cases():
    return CS.ood_cases()


@pytest.fixture(scope="module")
def g11b():
    return np.load(G11B)


def test_g11b_holds_every_case_and_only_data(g11b):
    names = set(k.rsplit("_", 1)[0] for k in g11b.files)
    assert names == set(CS.OOD_NAMES)
    for k in g11b.files:
        assert g11b[k].dtype in (np.float32, np.float64) and k.rsplit("_", 1)[1] in ("res", "pos", "neg")
    assert os.path.getsize(G11B) < 400 * 1024


@pytest.mark.parametrize("name", CS.OOD_NAMES)
def test_ood_oracle_matches_fixture_and_table_regenerates_inputs(name, ood_cases, g11b):
    pos, neg, recall = ood_cases[name]
    assert pos.dtype == np.float32 and neg.dtype == np.float32
    assert np.isfinite(pos).all() and np.isfinite(neg).all()                 # scikit-learn refuses NaN / inf
    if name + "_pos" in g11b.files:                                          # bit-equal inputs (signed zeros included)
        assert np.array_equal(pos.view(np.uint32), g11b[name + "_pos"].view(np.uint32))
        assert np.array_equal(neg.view(np.uint32), g11b[name + "_neg"].view(np.uint32))
    else:
        assert len(pos) + len(neg) > CS.OOD_STORE_INPUTS_UP_TO
    a, p, f = OR.get_measures(pos, neg, recall)
    ref = g11b[name + "_res"]
    assert abs(a - ref[0]) <= 2e-16, (a, ref[0])
    assert abs(p - ref[1]) <= 2e-16, (p, ref[1])
    assert f == ref[2], (f, ref[2])


@pytest.mark.parametrize("name", CS.OOD_NAMES)
def test_ood_oracle_matches_live_sklearn(name, ood_cases):
    sk = pytest.importorskip("sklearn.metrics")
    pos, neg, recall = ood_cases[name]
    y = np.r_[np.ones(len(pos), np.int32), np.zeros(len(neg), np.int32)]
    s = np.r_[pos, neg]
    a, p, _ = OR.get_measures(pos, neg, recall)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ra, rp = sk.roc_auc_score(y, s), sk.average_precision_score(y, s)
    assert abs(a - ra) <= 2e-16, (a, ra)
    assert abs(p - rp) <= 2e-16, (p, rp)


def test_ood_known_values(ood_cases):
    """what the definitions give without any implementation"""
    a, p, f = OR.get_measures(*ood_cases["all_equal"])
    assert (a, p, f) == (0.5, 40 / 100, 1.0)
    assert OR.get_measures(*ood_cases["sep_high"])[0] == 1.0 and OR.get_measures(*ood_cases["sep_low"])[0] == 0.0
    a, p, f = OR.get_measures(*ood_cases["order_zero_only"])                  # +0.0 and -0.0 tie
    assert (a, p, f) == (0.5, 4 / 7, 1.0)
    assert OR.get_measures(*ood_cases["pn_1_1"])[0] in (0.0, 1.0)
    pos, neg, _ = ood_cases["order"]                                          # the order case holds every kind of value
    v = np.r_[pos, neg]
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    assert ((v != 0) & (np.abs(v) < tiny)).sum() > 500 and (v == CS.FLT_MAX).any() and (v == -CS.FLT_MAX).any()
    assert (v == np.float32(1e-45)).any() and (v == np.float32(-1e-45)).any()


def test_ood_label_and_mask_cases_reduce_as_eval_ood_measure(ood_cases):
    conf, lab = CS.ood_labelled()
    assert set(CS.OOD_OUT8) <= set(lab.tolist()) and min(CS.OOD_OUT8) < 0 and max(CS.OOD_OUT8) > 2 ** 31
    pos, neg, r = ood_cases["labels8"]
    assert OR.eval_ood_measure(conf, lab, list(CS.OOD_OUT8)) == OR.get_measures(pos, neg, r)
    assert OR.eval_ood_measure(conf, lab, [4, 5, 6]) is None
    conf, lab, mask = CS.ood_one_each()
    assert mask.sum() == 2 and (lab[mask] == 13).sum() == 1
    assert OR.eval_ood_measure(conf, lab, [13], mask=mask) == OR.get_measures(*ood_cases["one_each"])


# ---- dissum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip,inclusive", CS.DISSUM_MODES)
@pytest.mark.parametrize("K", CS.DISSUM_KS)
def test_dissum_oracle_equals_formula_on_boundaries(K, clip, inclusive):
    imgs = [CS.dissum_on_clip(K)[0], CS.dissum_all_clip_but_one(K)[0], CS.dissum_signed_zero(False)[0],
            CS.dissum_signed_zero(True)[0]] + list(CS.dissum_batch(K)) + [CS.dissum_flat(K, 257)[0]]
    for lg in imgs:
        ref, s = CS.dissum_ref(lg, clip, inclusive)
        got = O.dissum_score(lg.astype(np.float64), clip, inclusive)
        assert np.array_equal(got, ref)
        assert s.max() <= clip and np.nanmin(ref) == 0.0 and np.nanmax(ref) == 1.0
        bar, _ = CS.dissum_bar(lg, clip, inclusive)
        assert bar < 1e-3                                                    # the derived bar is a real bar on every case


def test_dissum_boundary_inputs_are_what_they_claim():
    lg = CS.dissum_on_clip(16)[0]
    s = -lg.astype(np.float64).sum(axis=0).ravel()                            # exact: one non-zero logit per pixel
    for c in (400.0, 1000.0):
        assert {float(CS.down(c)), c, float(CS.up(c))} <= set(s.tolist())
    for clip, inclusive in CS.DISSUM_MODES:
        _, sc = CS.dissum_ref(lg, clip, inclusive)
        assert (sc.ravel()[s >= clip] == clip).all() and (sc.ravel()[s < clip] == s[s < clip]).all()
    _, sc = CS.dissum_ref(CS.dissum_all_clip_but_one(13)[0], 400.0, True)
    assert (sc == 400.0).sum() == sc.size - 1
    for last in (False, True):
        lg = CS.dissum_signed_zero(last)[0]
        s = -lg.astype(np.float64).sum(axis=0).ravel()
        z = np.flatnonzero(s == 0)
        assert len(z) == 1 and (np.delete(s, z) < 0).all() and s.argmin() == 0 and s.min() == -128.0
        assert z[0] == (len(s) - 1 if last else 5)
        assert np.array_equal(-lg.sum(axis=0, dtype=np.float32).ravel().astype(np.float64), s)   # exact in fp32 too
    b = CS.dissum_batch(16)
    rng = [np.ptp(CS.dissum_ref(im, 1e30, False)[1]) for im in b]
    assert rng[1] > 50 * rng[0] and rng[2] > 50 * rng[1]                      # per-image ranges ~100x apart
    assert (CS.dissum_ref(b[0], 1000.0, False)[1] < 0).any() and (CS.dissum_ref(b[0], 1000.0, False)[1] > 0).any()
    ref, _ = CS.dissum_ref(np.full((4, 1, 64), -2.0, np.float32), 400.0, True)
    assert np.isnan(ref).all()                                                # constant image: 0 / 0


# ---- relabel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS.RELABEL_CS)
@pytest.mark.parametrize("K", CS.RELABEL_KS)
def test_relabel_oracle_equals_formula_on_exact_cases(C, K):
    for new_label in CS.RELABEL_LABELS:
        feats, lg, proto, preds, expect = CS.relabel_exact(C, K, new_label)
        n = preds.shape[-1]
        assert float(np.float32(-1.5)) in expect and 0.0 in expect and expect[0.0] == []
        for th, idx in expect.items():
            for b in range(2):
                ref, d, _ = CS.relabel_ref(preds[b], lg[b], feats[b], proto, th, new_label)
                got = O.novel_relabel(preds[b], lg[b].astype(np.float64), feats[b].astype(np.float64),
                                      proto.astype(np.float64), th, new_label)
                assert np.array_equal(got, ref)
                want = preds[b].copy().ravel()
                want[[i if b == 0 else n - 1 - i for i in idx]] = new_label
                assert np.array_equal(ref.ravel(), want)
                # exact in fp32: the fp32 evaluation of d equals the fp64 one bit for bit
                d32 = -((feats[b] - proto) ** 2).sum(axis=-1, dtype=np.float32)
                assert np.array_equal(d32.astype(np.float64), d)
        dt = -1.5 if C >= 3 else -1.0
        assert 0 not in expect[dt] and 0 in expect[float(CS.down(dt))]        # d == thresh / one ulp above it
        assert 1 not in expect[-5.0] and 2 in expect[-5.0] and 5 not in expect[-5.0]   # d == max logit / one ulp either side
        assert 3 in expect[-5.0] and 4 not in expect[-1.5] and 4 in expect[-5.0]   # already new_label; 255 survives below thresh


def test_relabel_random_input_stays_within_the_exclusion_cap():
    feats, lg, proto, preds = CS.relabel_random()
    for th in (-1.5, 0.0):
        undecidable = changed = 0
        for b in range(preds.shape[0]):
            ref, d, margin = CS.relabel_ref(preds[b], lg[b], feats[b], proto, th, 16)
            undecidable += int((margin <= CS.relabel_err(d, feats.shape[-1])).sum())
            changed += int((ref != preds[b]).sum())
        assert undecidable <= CS.EXCLUDE_CAP * preds.size, undecidable
        if th < 0:
            assert 0.05 * preds.size < changed < 0.95 * preds.size           # both outcomes are well represented


# ---- argmax / MSP ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CS.MSP_KS)
def test_msp_reference_on_known_values(K):
    for shape in CS.MSP_SHAPES:
        p, m = CS.msp_ref(CS.msp_logits("gap", K, shape))
        assert (m == 0.0).all()
        p, m = CS.msp_ref(CS.msp_logits("uniform", K, shape))
        assert (p == 0).all() and np.abs(m - (1.0 - 1.0 / K)).max() <= 2 * CS.EPS64
        lg = CS.msp_logits("ties", K, shape)
        p, m = CS.msp_ref(lg)
        mx = lg.max(axis=1)
        first = np.array([[next(k for k in range(K) if lg[b, k].ravel()[i] == mx[b].ravel()[i])
                           for i in range(mx[b].size)] for b in range(shape[0])]).reshape(p.shape)
        assert np.array_equal(p, first)
        if K > 2 and mx[0].size > 1:
            assert (p == K - 2).any() and (p == 0).any()
        lg = CS.msp_logits("dist", K, shape)
        import torch
        ref = O.msp_score(torch.from_numpy(lg).double()).numpy()
        assert np.abs(CS.msp_ref(lg)[1] - ref).max() <= 4 * CS.EPS64
        if shape[0] > 1:
            assert not np.array_equal(lg[0], lg[1])                          # different data per image
    assert CS.msp_bar(K) == 2 * (2 * K + 4) * 2.0 ** -24


# ---- confusion / feature sums ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CS.CONF_NS)
def test_confusion_reference_equals_oracle_where_predictions_are_classes(n):
    lt, lp = CS.confusion_inputs(n, 5000)
    assert {255, -1, n, 2 ** 40} <= set(lt.tolist()) and {n, -1, 2 ** 40 + 1} <= set(lp.tolist())
    ok = (lp >= 0) & (lp < n)
    assert np.array_equal(CS.confusion_ref(lt, lp, n), MR.fast_hist(lt[ok], lp[ok], n))
    assert CS.confusion_ref(lt, lp, n).sum() == ((lt >= 0) & (lt < n) & ok).sum()


def test_feature_sum_reference_and_bar():
    f, lab = CS.fsum_inputs(7, 257)
    s, a, n = CS.fsum_ref(f, lab, 4)
    assert n == 1 and np.array_equal(s, f[-1].astype(np.float64))
    assert CS.fsum_ref(f, lab, 3)[2] == 0 and (CS.fsum_ref(f, lab, 3)[0] == 0).all()
    s, a, n = CS.fsum_ref(f, lab, 1)
    assert np.allclose(s / n, 1e3, atol=1.0)
    # the bar separates an fp64-finished sum from an fp32-only accumulation of the offset features at full size
    npx = CS.FSUM_BIG
    one_class = npx / 3 * 1e3
    fp32_only = one_class * CS.EPS32 * np.sqrt(npx / 3)                       # random-walk estimate of a running fp32 sum
    assert CS.fsum_bar(npx, one_class) < fp32_only
