"""CPU: the open-set threshold sweep without a GPU -- the cube-to-matrix identity of include/dmlnet_hip.h against the per-threshold
route as the reference writes it, the score formulas of metrics.OpenSetSweepMetrics against restatements of the reference's, the
ABI plumbing of dml_open_set_sweep, every argument check that returns before a launch, the driver's flag, and the refusal of CPU
tensors.

The reference lines restated below.  anomaly/eval_ood_traditional.py: :227-229 seg_label_unknown = 1 where the label is not 13,
0 where it is; :537-549 pred[conf < thre] = 13; :600-605 unknown_pred = 0 where conf < threshold, 1 where conf >= threshold,
intersectionAndUnion(unknown_pred, seg_label_unknown, 2); :646 iou = intersection / (union + 1e-10).  anomaly/utils.py:136-156
intersectionAndUnion: both maps + 1, prediction zeroed where the label is 0, area_intersection = histogram of the prediction where it
equals the label, area_union = area_pred + area_lab - area_intersection.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers as H
import open_sweep_cases as OC

EINVAL, EALIGN = -1, -2


def intersection_and_union(im_pred, im_lab, num_class):
    """anomaly/utils.py:136-156 of the reference, restated"""
    im_pred = np.asarray(im_pred).copy() + 1
    im_lab = np.asarray(im_lab).copy() + 1
    im_pred = im_pred * (im_lab > 0)
    inter = im_pred * (im_pred == im_lab)
    area_inter, _ = np.histogram(inter, bins=num_class, range=(1, num_class))
    area_pred, _ = np.histogram(im_pred, bins=num_class, range=(1, num_class))
    area_lab, _ = np.histogram(im_lab, bins=num_class, range=(1, num_class))
    return area_inter, area_pred + area_lab - area_inter


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_cube_identity_equals_the_per_threshold_route(name):
    c = OC.CASES[name]
    conf, pred, label, t = OC.inputs(name)
    cube = OC.reference(name)
    assert cube.sum() == ((OC.remap(label, c["out"], c["u"]) >= 0) & (OC.remap(label, c["out"], c["u"]) < c["nc"])
                          & (pred >= 0) & (pred < c["nc"])).sum()
    from metrics.open_set import cube_to_matrix
    for i in range(len(t)):
        want = OC.matrix_brute(conf, pred, label, t[i], c["out"], c["nc"], c["u"])
        assert np.array_equal(OC.matrix_from_cube(cube, i, c["u"]), want), (name, i)
        assert np.array_equal(cube_to_matrix(cube, i, c["u"]), want), (name, i)      # the package's own derivation


def test_edge_confidences_fall_into_the_bins_the_header_names():
    t = OC.thresholds_for(3)
    conf = np.array([np.nan, np.inf, -np.inf, t[1], np.nextafter(t[1], np.float32(0)), np.nextafter(t[1], np.float32(1))], np.float32)
    pred = np.zeros(6, np.int64)
    label = np.zeros(6, np.int64)
    cube = OC.cube_ref(conf, pred, label, t, (), 2, 1)
    assert cube[0, 0].tolist() == [2, 1, 2, 1]          # NaN, -inf | just below t1 | t1 itself (inclusive), just above | +inf
    assert OC.open_pred_ref(conf, pred + 0, t[1], 1).tolist() == [1, 0, 1, 0, 1, 0]


def _metrics_with_cube(name):
    """an OpenSetSweepMetrics whose device cube is replaced by the case's reference cube on the host"""
    import metrics
    c = OC.CASES[name]
    m = metrics.OpenSetSweepMetrics(c["nc"], OC.thresholds_for(c["T"]), c["u"], c["out"])
    m._host_cube = lambda: np.array(OC.reference(name))
    return m


@pytest.mark.parametrize("name", ["n300007", "T9_k14_last", "T12_k33_middle", "T1_k2_first", "no_unknown", "all_unknown", "pred_oob"])
def test_scores_equal_the_reference_formulas(name):
    c = OC.CASES[name]
    conf, pred, label, t = OC.inputs(name)
    nc, u = c["nc"], c["u"]
    m = _metrics_with_cube(name)
    res = m.get_results()
    assert len(res) == len(t)
    lab = OC.remap(label, c["out"], u)
    ok = (lab >= 0) & (lab < nc) & (pred >= 0) & (pred < nc)
    for i, r in enumerate(res):
        assert r["Threshold"] == float(t[i])
        assert np.array_equal(m.confusion(i), OC.matrix_brute(conf, pred, label, t[i], c["out"], nc, u))
        want = OC.results_ref(OC.matrix_brute(conf, pred, label, t[i], c["out"], nc, u), u)
        for k, v in want.items():
            assert r[k] == v or (np.isnan(r[k]) and np.isnan(v)), (name, i, k, r[k], v)
        # the reference's binary maps (1 = known, 0 = unknown) of the open-set prediction and of the label, over the scored pixels
        p_t = OC.open_pred_ref(conf, pred, t[i], u)[ok]
        inter, union = intersection_and_union((p_t != u).astype(np.int64), (lab[ok] != u).astype(np.int64), 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = inter.astype(np.float64) / union.astype(np.float64)
        for key, cls in (("Unknown IoU", 0), ("Known IoU", 1)):
            assert r[key] == iou[cls] or (np.isnan(r[key]) and np.isnan(iou[cls])), (name, i, key, r[key], iou[cls])
    # a prediction that never names the unknown class: the binary prediction is the reference's `conf >= threshold` itself
    if name == "no_unknown":
        keep = ok & (pred != u)
        cube = OC.cube_ref(conf[keep], pred[keep], label[keep], t, c["out"], nc, u)
        for i in range(len(t)):
            with np.errstate(invalid="ignore"):
                unknown_pred = (conf[keep] >= t[i]).astype(np.int64)
            inter, union = intersection_and_union(unknown_pred, (lab[keep] != u).astype(np.int64), 2)
            got = OC.results_ref(OC.matrix_from_cube(cube, i, u), u)
            with np.errstate(divide="ignore", invalid="ignore"):
                assert got["Known IoU"] == inter[1] / np.float64(union[1])
                assert got["Unknown IoU"] == inter[0] / np.float64(union[0]) or union[0] == 0


def test_closed_mean_iou_equals_stream_metrics():
    import metrics
    name = "n300007"
    c = OC.CASES[name]
    conf, pred, label, t = OC.inputs(name)
    lab = OC.remap(label, c["out"], c["u"])
    ok = (lab >= 0) & (lab < c["nc"]) & (pred >= 0) & (pred < c["nc"])
    s = metrics.StreamSegMetrics(c["nc"])
    s._host = np.bincount(c["nc"] * lab[ok] + pred[ok], minlength=c["nc"] ** 2).reshape(c["nc"], c["nc"]).astype(np.float64)
    want = s.get_results()["Mean IoU"]
    res = _metrics_with_cube(name).get_results()
    assert all(r["Closed Mean IoU"] == want for r in res) and 0.0 < want < 1.0
    # with every threshold passed the open-set matrix is the closed-set one
    conf1 = np.ones_like(conf)
    cube = OC.cube_ref(conf1, pred, label, t, c["out"], c["nc"], c["u"])
    assert np.array_equal(OC.matrix_from_cube(cube, len(t) - 1, c["u"]), s._host.astype(np.int64))


def test_results_of_an_empty_meter_and_to_str():
    import metrics
    m = metrics.OpenSetSweepMetrics(14, (0.1, 0.5, 0.9), 13, (13,))
    assert m.cube is None and m.confusion(2).shape == (14, 14) and m.confusion(0).sum() == 0
    m.reset()
    m.all_reduce()                                                     # no process group: a no-op
    assert m.cube is None
    with pytest.raises(IndexError):
        m.confusion(3)
    txt = metrics.OpenSetSweepMetrics.to_str(_metrics_with_cube("T3").get_results())
    assert len([ln for ln in txt.splitlines() if ln.startswith("threshold ")]) == 3 and "Unknown IoU" in txt
    for bad in ((), tuple(0.01 * k for k in range(13)), (0.5, 0.5), (0.5, 0.4), (float("nan"),), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            metrics.OpenSetSweepMetrics(14, bad, 13)
    for nc, u, out in ((1, 0, ()), (34, 0, ()), (14, 14, ()), (14, -1, ()), (14, 13, tuple(range(9)))):
        with pytest.raises(ValueError):
            metrics.OpenSetSweepMetrics(nc, (0.5,), u, out)


def test_symbol_is_declared_bound_and_in_the_plan_table():
    from dmlnet import _lib
    assert "dml_open_set_sweep" in _lib.EXPORTS
    hdr = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    assert re.search(r"^int\s+dml_open_set_sweep\s*\(", hdr, flags=re.M)
    lib = _lib.load()
    assert lib.dml_abi_version() == 6
    fid = lib.dml_plan_fn_id(b"dml_open_set_sweep")
    assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(lib.dml_open_set_sweep.argtypes) - 1 == 13
    assert (_lib.OPEN_SWEEP_SPAN, _lib.OPEN_SWEEP_MAX_BLOCKS) == (OC.SPAN, OC.MAX_BLOCKS)
    src = open(os.path.join(H.PKG, "csrc", "open_sweep.hip")).read()
    assert "SWEEP_THREADS = 256, SWEEP_PX = 8" in src and "SWEEP_MAX_BLOCKS = 512" in src and OC.SPAN == 256 * 8


def test_argument_checks_return_before_any_launch():
    """every pointer below is a made-up, aligned address: each call must be refused by the host-side checks"""
    from dmlnet import _lib
    lib = _lib.load()
    A = 0x10000                                                        # never dereferenced
    good_t = (C.c_float * 12)(*[0.05 * (k + 1) for k in range(12)])
    out9 = (C.c_int64 * 9)(*range(100, 109))

    def call(conf=A, pred=A, label=A, n=100, t=good_t, T=9, out=out9, n_out=1, nc=14, u=13, cube=A, open_pred=None, w=0):
        return lib.dml_open_set_sweep(conf, pred, label, n, t, T, out, n_out, nc, u, cube, open_pred, w, None)

    def ts(*v):
        return (C.c_float * len(v))(*v)

    assert call(conf=None) == EINVAL and call(pred=None) == EINVAL and call(label=None) == EINVAL and call(cube=None) == EINVAL
    assert call(t=None) == EINVAL and call(n=-1) == EINVAL
    assert call(T=0) == EINVAL and call(T=13) == EINVAL and call(T=-1) == EINVAL
    assert call(t=ts(0.5, 0.4), T=2) == EINVAL                         # unsorted
    assert call(t=ts(0.1, 0.5, 0.5), T=3) == EINVAL                    # equal
    nan = float("nan")
    assert call(t=ts(nan), T=1) == EINVAL and call(t=ts(0.1, nan), T=2) == EINVAL and call(t=ts(nan, 0.5), T=2) == EINVAL
    assert call(nc=1) == EINVAL and call(nc=34, u=33) == EINVAL and call(nc=0, u=0) == EINVAL
    assert call(u=14) == EINVAL and call(u=-1) == EINVAL
    assert call(n_out=9) == EINVAL and call(n_out=-1) == EINVAL and call(out=None, n_out=1) == EINVAL
    assert call(open_pred=A, w=9) == EINVAL and call(open_pred=A, w=-1) == EINVAL and call(open_pred=A, T=3, w=3) == EINVAL
    assert call(cube=None, open_pred=None, label=None) == EINVAL       # nothing to compute
    # the promised alignment: 4 bytes for conf, 8 for the int64 arrays
    assert call(conf=A + 2) == EALIGN and call(pred=A + 4) == EALIGN and call(label=A + 4) == EALIGN
    assert call(cube=A + 4) == EALIGN and call(open_pred=A + 4) == EALIGN
    # n == 0 passes the checks, launches nothing and returns 0 -- also at the limits themselves
    assert call(n=0) == 0 and call(n=0, T=12, nc=33, u=32, n_out=8) == 0 and call(n=0, T=1, nc=2, u=0, n_out=0, out=None) == 0
    assert call(n=0, conf=A + 4, pred=A + 8, label=A + 8, cube=A + 8, open_pred=A + 8, w=8) == 0
    assert call(n=0, cube=None, label=None, open_pred=A) == 0          # the prediction alone
    assert call(n=0, T=13) == EINVAL                                   # the checks come first


def test_driver_flag():
    import eval_ood_traditional as T
    p = T.build_parser()
    assert p.parse_args([]).open_set_thresholds is None
    o = p.parse_args(["--open_set_thresholds", "0.1", "0.5", "0.9"])
    assert o.open_set_thresholds == [0.1, 0.5, 0.9] and o.ood == "dissum"
    o = p.parse_args(["--synthetic", "--open_set_thresholds", "0.25", "--ood", "msp", "--num_images", "1"])
    assert o.open_set_thresholds == [0.25] and o.ood == "msp" and o.num_images == 1 and o.synthetic
    help_text = " ".join(p.format_help().split())
    assert "--open_set_thresholds" in help_text and "0.1 ... 0.9" in help_text
    import inspect
    sig = inspect.signature(T.evaluate)
    assert list(sig.parameters)[-1] == "open_set_thresholds" and sig.parameters["open_set_thresholds"].default is None


def test_no_cpu_fallback():
    import metrics
    import utils
    m = metrics.OpenSetSweepMetrics(14, (0.5,), 13, (13,))
    lab, conf = torch.zeros(8, dtype=torch.int64), torch.zeros(8)
    with pytest.raises(TypeError, match="no CPU fallback"):
        m.update(lab, lab, conf)
    assert m.cube is None
    with pytest.raises(RuntimeError, match="HIP path only"):
        utils.open_set_predict(conf, lab, 0.5, 13)
