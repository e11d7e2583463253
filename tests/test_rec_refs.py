"""CPU: the float64 definition of the reconstruction-consistency score (tests/rec_cases.py) is what the reference's own
statements compute, the bar of tests/test_gpu_rec_score.py follows from their float32 run, the gate cases put pixels on
both sides, and the entry points, the wrappers and the driver's flags exist.  No kernel is launched here."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import helpers as H
import rec_cases as RC

F64 = np.float64


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_definition_is_the_references_statements_in_float64(name):
    f1, f2 = RC.inputs(name)
    cos, zero = RC.reference(name)
    want = RC.torch_cosine(f1, f2, RC.CASES[name]["out"], torch.float64)
    err = np.abs(cos - want).max()
    print("MEASURE %s float64 statements vs definition: %.3e" % (name, err))
    assert cos.shape == (RC.CASES[name]["B"],) + tuple(RC.CASES[name]["out"])
    assert err <= 1e-12
    assert np.isfinite(cos).all() and np.abs(cos).max() <= 1.0 + 1e-12
    # exactly zero vectors give exactly 0, in the definition and in torch
    assert (cos[zero] == 0.0).all() and (want[zero] == 0.0).all()


@pytest.mark.parametrize("name", sorted(RC.CONF_CASES))
def test_confidence_definition_is_the_references_statements_in_float64(name):
    c = RC.CONF_CASES[name]
    scores, cos = RC.conf_inputs(name)
    ref = RC.conf_reference(name)
    conf, msp = RC.torch_confidence(scores, cos, c["threshold"], c["prob"], c["first_class"], torch.float64)
    assert np.abs(msp - ref["msp"]).max() <= 1e-13
    assert np.abs(conf - ref["conf"]).max() <= 1e-13
    assert ref["conf"].shape == (c["B"],) + RC.CONF_HW


def _float32_deviations():
    dev = {}
    for name in sorted(RC.CASES):
        f1, f2 = RC.inputs(name)
        got = RC.torch_cosine(f1, f2, RC.CASES[name]["out"], torch.float32)
        assert got.dtype == np.float32
        dev[name] = float(np.abs(got.astype(F64) - RC.reference(name)[0]).max())
    for name in sorted(RC.CONF_CASES):
        c = RC.CONF_CASES[name]
        scores, cos = RC.conf_inputs(name)
        ref = RC.conf_reference(name)
        conf, _ = RC.torch_confidence(scores, cos, c["threshold"], c["prob"], c["first_class"], torch.float32)
        keep = ~ref["near"]
        dev["conf:" + name] = float(np.abs(conf.astype(F64) - ref["conf"])[keep].max())
    return dev


def test_gpu_bar_is_ten_times_the_float32_deviation_of_the_statements():
    """GPU_BAR = 10 x the largest deviation of the reference's statements in float32 from the float64 definition over both
    case lists.  The constant next to the cases is this machine's figure rounded up to two digits; a float32 run on
    another CPU may sum in another order, so the constant is held to the rule within a quarter, never below it."""
    dev = _float32_deviations()
    for k, v in dev.items():
        print("MEASURE float32 deviation %-28s %.3e" % (k, v))
    worst = max(dev.values())
    rule = 10.0 * worst
    print("MEASURE rule 10 x %.3e = %.3e, GPU_BAR = %.3e" % (worst, rule, RC.GPU_BAR))
    assert rule <= 1e-4, "ill-conditioned cases: change the cases, not the bar"
    assert rule <= RC.GPU_BAR <= 1.25 * rule


def test_bf16_cases_hold_bf16_values_and_same_gives_one():
    for name, c in RC.CASES.items():
        f1, f2 = RC.inputs(name)
        if c["dtype"] == "bf16":
            for a in f1 + f2:
                assert np.array_equal(RC.bf16_round(a), a), name
        assert len(f1) == len(c["scales"]) <= RC.MAX_SCALES and (c["ld"] is None or all(l >= c["C"] for l in c["ld"]))
    cos, zero = RC.reference("same_c4096")
    assert not zero.any() and np.abs(cos - 1.0).max() <= 1e-12
    # signed inputs, non-trivial similarities
    cos, _ = RC.reference("five_c4096_f32")
    assert 0.5 < cos.min() < cos.max() < 0.95
    f1, _ = RC.inputs("five_c4096_f32")
    assert (f1[0] < 0).mean() > 0.4


def test_cases_cover_what_they_claim():
    c = RC.CASES
    assert c["five_c4096_f32"]["scales"] == RC.FIVE and c["five_c4096_f32"]["out"] == (9, 12)
    assert any(h > 9 and w > 12 for h, w in RC.FIVE) and any(h < 9 and w < 12 for h, w in RC.FIVE)
    assert any(l > 4096 for l in c["five_c4096_f32"]["ld"]) and any(l > 4096 for l in c["five_c4096_bf16"]["ld"])
    assert len(RC.EIGHT) == 8 and (1, 1) in RC.EIGHT and c["eight_scales_b2"]["B"] == 2
    assert c["one_by_one_out"]["out"] == (1, 1) and c["c13_scalar"]["C"] == 13 and c["c4100_f32"]["C"] == 4100
    assert c["c13_scalar"]["ld"] is None and c["c13_tail"]["ld"] == (16, 16)          # 13 % 4: one channel per load / vector + tail
    assert c["wide_two_strips"]["out"][1] > 32                                       # more than two 16-pixel strips per row
    for name in ("zero_block", "zero_block_bf16"):
        cos, zero = RC.reference(name)
        print("MEASURE %s exactly-zero pixels: %d of %d" % (name, zero.sum(), zero.size))
        assert 4 <= zero.sum() < zero.size // 2
        assert np.abs(cos[~zero]).min() > 1e-3                                       # the others are ordinary pixels
    k = {n: (v["K"], v["first_class"], v["prob"]) for n, v in RC.CONF_CASES.items()}
    assert (13, 0, "logit") in k.values() and (13, 1, "logit") in k.values() and (13, 0, "softmax") in k.values()
    assert (13, 1, "softmax") in k.values()
    widths = {v["K"] - v["first_class"] for v in RC.CONF_CASES.values()}
    assert {1, 12, 13, 32} <= widths and max(widths) == RC.MAX_CLASSES
    assert RC.CONF_HW == (37, 50) and RC.CONF_COS_HW == (9, 12) and RC.CONF_HW[0] % 4 and RC.CONF_HW[1] % 4
    assert RC.CONF_CASES["k13_softmax_999"]["threshold"] == 0.999


@pytest.mark.parametrize("name", sorted(RC.CONF_CASES))
def test_gate_cases_put_pixels_on_both_sides(name):
    c = RC.CONF_CASES[name]
    ref = RC.conf_reference(name)
    near, opened = ref["near"].mean(), ref["gate"].mean()
    print("MEASURE %s gate open %.3f, within the bar of the threshold %.5f" % (name, opened, near))
    assert near <= RC.GATE_MAX_FRACTION
    if c["prob"] == "softmax" and c["K"] - c["first_class"] > 1:
        assert 0.10 <= opened <= 0.90
    if name == "k13_logit_closed":
        assert opened == 0.0 and np.array_equal(ref["conf"], ref["rec"])              # the reference's literal statement
    if name in ("k13_logit", "k13_logit_back", "k33_back_logit", "k1_logit"):
        assert 0.10 <= opened <= 0.90
    if name == "k2_back_softmax":
        assert opened == 1.0 and (ref["conf"] == 1.0).all()                           # the softmax of one class


def test_entry_points_and_bindings():
    from dmlnet import _lib
    header = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    assert "dml_rec_cosine" in _lib.EXPORTS and "dml_rec_confidence" in _lib.EXPORTS
    assert "int dml_rec_cosine(" in header and "int dml_rec_confidence(" in header and "#define DML_REC_MAX_SCALES 8" in header
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib = _lib.load()
    assert lib.dml_abi_version() == 6 and _lib.REC_MAX_SCALES == 8 == RC.MAX_SCALES
    assert lib.dml_rec_cosine.argtypes == [p, p, p, p, p, i, i, i, i, p, i, i, p] and lib.dml_rec_cosine.restype is i
    assert lib.dml_rec_confidence.argtypes == [p, p, p, i, i, i, i, i, i, i, f, i, p] and lib.dml_rec_confidence.restype is i
    # both refuse before any HIP call
    assert lib.dml_rec_cosine(None, None, None, None, None, 1, 1, 8, 0, None, 4, 4, None) == -1
    ptrs, nul = (p * 2)(64, 64), (p * 2)(64, None)
    ints = (i * 2)(4, 4)
    out = ctypes.c_void_p(64)
    assert lib.dml_rec_cosine(ptrs, nul, ints, ints, (i * 2)(8, 8), 2, 1, 8, 0, out, 4, 4, None) == -1      # a NULL source
    assert lib.dml_rec_cosine(ptrs, ptrs, ints, ints, (i * 2)(8, 8), 0, 1, 8, 0, out, 4, 4, None) == -1     # n outside 1 .. 8
    assert lib.dml_rec_cosine(ptrs, ptrs, ints, ints, (i * 2)(8, 8), 9, 1, 8, 0, out, 4, 4, None) == -1
    assert lib.dml_rec_cosine(ptrs, ptrs, ints, ints, (i * 2)(8, 8), 2, 1, 8, 2, out, 4, 4, None) == -1     # unknown element type
    assert lib.dml_rec_cosine(ptrs, ptrs, ints, ints, (i * 2)(8, 8), 2, 1, 8, 0, out, 0, 4, None) == -1     # non-positive sizes
    assert lib.dml_rec_cosine(ptrs, ptrs, (i * 2)(4, 0), ints, (i * 2)(8, 8), 2, 1, 8, 0, out, 4, 4, None) == -1
    assert lib.dml_rec_cosine(ptrs, ptrs, ints, ints, (i * 2)(8, 7), 2, 1, 8, 0, out, 4, 4, None) == -1     # ld < C
    assert lib.dml_rec_confidence(None, None, None, 1, 13, 8, 8, 2, 2, 0, 0.999, 1, None) == -1
    assert lib.dml_rec_confidence(out, out, out, 1, 40, 8, 8, 2, 2, 0, 0.999, 1, None) == -1                # K - first_class > 32
    assert lib.dml_rec_confidence(out, out, out, 1, 13, 8, 8, 2, 2, 13, 0.999, 1, None) == -1


def test_driver_flags_and_wrappers():
    import eval_ood_rec as R
    import eval_ood_traditional as T
    o = R.build_parser().parse_args([])
    assert (o.ood, o.rec_threshold, o.rec_prob) == ("rec", 0.999, "logit") == ("rec", R.REC["threshold"], R.REC["prob"])
    o = R.build_parser().parse_args(["--ood", "msp", "--exclude_back", "--rec_threshold", "0.9", "--rec_prob", "softmax",
                                     "--cfg", "c.yaml", "--gpu", "1", "DATASET.rec_dataset", "/tmp/rec", "VAL.checkpoint", "e.pth"])
    assert (o.ood, o.exclude_back, o.rec_threshold, o.rec_prob, o.cfg, o.gpu) == ("msp", True, 0.9, "softmax", "c.yaml", 1)
    assert o.opts == ["DATASET.rec_dataset", "/tmp/rec", "VAL.checkpoint", "e.pth"]
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(["--ood", "crf"])
    for flag in ("--synthetic", "--num_images", "--height", "--width", "--dtype", "--workers"):
        assert flag in R.build_parser().format_help()
    assert R.CFG_DEFAULTS["DATASET.rec_dataset"] == "./data" and "DATASET.rec_dataset" not in T.CFG_DEFAULTS
    assert {k: v for k, v in R.CFG_DEFAULTS.items() if k != "DATASET.rec_dataset"} == T.CFG_DEFAULTS
    assert R.load_cfg("", [])["DATASET.rec_dataset"] == "./data"
    cfg = R.load_cfg("", ["DATASET.rec_dataset", "/tmp/rec", "DATASET.num_class", "13"])
    assert cfg["DATASET.rec_dataset"] == "/tmp/rec" and cfg["DATASET.num_class"] == 13

    import models
    import utils
    assert list(inspect.signature(utils.rec_cosine_score).parameters) == ["feats1", "feats2", "out_hw"]
    sig = inspect.signature(utils.rec_confidence)
    assert list(sig.parameters) == ["scores", "cos", "threshold", "prob", "first_class"]
    assert [sig.parameters[k].default for k in ("threshold", "prob", "first_class")] == [0.999, "logit", 0]
    assert "never opens" in utils.rec_confidence.__doc__
    with pytest.raises(RuntimeError, match="HIP path only"):
        utils.rec_cosine_score([torch.zeros(1, 2, 2, 8)], [torch.zeros(1, 2, 2, 8)], (2, 2))
    with pytest.raises(RuntimeError, match="HIP path only"):
        utils.rec_confidence(torch.zeros(1, 13, 8, 8), torch.zeros(1, 2, 2))
    assert list(inspect.signature(models.evaluate_multiscale_rec).parameters) == ["segmentation_module", "img_resized_list",
                                                                                 "img_resized_list_rec", "segSize"]
    from dmlnet.engine_ppm import PPMEngine
    sig = inspect.signature(PPMEngine.infer_multiscale)
    assert sig.parameters["keep_cat"].default is False and sig.parameters["want_scores"].default is True
    from datasets.streethazards import StreetHazardsReader
    assert inspect.signature(StreetHazardsReader.__init__).parameters["rec_dataset"].default is None
