"""CPU: the float64 definition of tests/mix_cases.py is the reference's "EDS + MMSP" recipe, the bar holds for a float32
evaluation of the reference's own statements, the seeded inputs keep the properties the GPU test relies on, and the new
entry point, wrapper and driver flags exist.  No kernel is launched here.

The reference lines restated below.  anomaly/eval_ood_traditional.py: :101-102 Normalizatoin, :104-106 Coefficient_map with
lamda = 50, :302-305 the clipped, normalised distance sum, :434-435 the normalised maximum softmax, :447-448 the gate at 0.2 and
the mix (which :450 then overwrites with `conf = dis_sum`).  test_embedding.py: :349-350 the distance sum clipped with `>`
at 1000, :365-369 the same mix with the gate at 0.3 and the maximum logit (:367).  Where the reference writes `.squeeze()`
the restatement drops only the batch axis: the frames here include rows and single pixels, which a full squeeze would
flatten.  `>= clip` and `> clip` give the same value at the clip, so one restatement serves both drivers.
"""
import os

import numpy as np
import pytest
import torch

import helpers as H
import mix_cases as MC

FINITE = [n for n in MC.CASES if n not in MC.NAN_CASES]


def Normalizatoin(x):                                                                               # :101-102
    return (x - np.min(x)) / (np.max(x) - np.min(x))


def Coefficient_map(x, thre, lamda):                                                                # :104-106
    return 1 / (1 + np.exp(lamda * (x - thre)))


def _literal(lg, case):
    """the reference's statements on float32 logits [B, K, H, W], image by image -> float32 [B, H, W]"""
    out = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(lg.shape[0]):
            tmp_scores = torch.from_numpy(np.array(lg[b:b + 1, case["k_first"]:]))                  # a writable copy
            assert tmp_scores.dtype == torch.float32
            dis_sum = torch.sum(tmp_scores, dim=1)                                                  # :302
            dis_sum = -dis_sum.squeeze(0).cpu().numpy()                                             # :303
            dis_sum[dis_sum >= case["clip"]] = case["clip"]                                         # :304
            dis_sum = Normalizatoin(dis_sum)                                                        # :305
            if case["prob"] == "softmax":
                prob_map = np.max(torch.nn.functional.softmax(tmp_scores, dim=1).squeeze(0).cpu().numpy(), axis=0)  # :434
            else:
                prob_map = tmp_scores.squeeze(0).detach().max(dim=0)[0].cpu().numpy()               # test_embedding.py:367
            prob_map = Normalizatoin(prob_map)                                                      # :435
            Coefficient = Coefficient_map(dis_sum, case["threshold"], case["slope"])                # :447
            conf = Coefficient * dis_sum + (1 - Coefficient) * prob_map                             # :448
            assert conf.dtype == np.float32
            out.append(conf)
    return np.stack(out)


def test_case_table_covers_the_issue():
    for sname in MC.SHAPES:
        for K in MC.KS:
            for prob in MC.PROBS:
                for clip in (400, 1000):
                    assert "%s_k%d_%s_%d" % (sname, K, prob, clip) in MC.CASES
    assert MC.SHAPES == {"px1": (1, 1, 1), "px2": (1, 1, 2), "odd": (1, 3, 5), "batch": (2, 33, 129),
                         "scalar": (1, 70, 131), "vec": (1, 40, 132)}
    assert MC.KS == (2, 13, 16, 19, 32) and max(MC.KS) == MC.MAX_CLASSES
    assert any(K <= MC.REG_CLASSES for K in MC.KS) and any(K > MC.REG_CLASSES for K in MC.KS)
    assert MC.CASES["kfirst_softmax"]["K"] == 14 and MC.CASES["kfirst_softmax"]["k_first"] == 1
    assert MC.CASES["steep_softmax"]["slope"] == 200.0 and MC.CASES["flat_logit"]["slope"] == 0.0
    assert MC.CASES["zero_row_softmax"]["shape"] == (1, 1, 3079)
    assert set(MC.OFFSET_CASES) <= set(FINITE) and len(MC.CLIP_CASES) >= 60
    # the frames that make pass 1's lanes loop: more lanes' worth of pixels than the grid has
    for name, px_per_lane in (("loop_scalar_softmax", 1), ("loop_vec_softmax", 4), ("loop_reread_logit", 1)):
        c = MC.CASES[name]
        (_, Hh, Ww), reg = c["shape"], c["K"] - c["k_first"] <= MC.REG_CLASSES
        assert (Hh * Ww % 4 == 0) == (px_per_lane == 4) and Hh * Ww > MC.PASS1_GRID[reg] * 256 * px_per_lane


@pytest.mark.parametrize("name", FINITE)
def test_float32_statements_stay_within_the_bar(name):
    """the definition is the reference's statements: their float32 evaluation lies inside bar(p) on every pixel"""
    lg, ref = MC.reference(name)
    lit = _literal(lg, MC.CASES[name]).astype(np.float64)
    assert np.isfinite(lit).all() and np.isfinite(ref["conf"]).all() and np.isfinite(ref["bar"]).all()
    err = np.abs(lit - ref["conf"])
    print("MEASURE literal f32 %s err=%.3e bar=%.3e worst err/bar=%.3e"
          % (name, err.max(), ref["bar"].max(), (err / ref["bar"]).max()))
    assert (err <= ref["bar"]).all()
    # the two weights the other way round are no such evaluation
    if MC.CASES[name]["slope"] > 0 and name.split("_")[0] in MC.STAT_SHAPES:
        swapped = (1.0 - ref["c"]) * ref["d"] + ref["c"] * ref["q"]
        assert (np.abs(swapped - ref["conf"]) > ref["bar"]).mean() > 0.5


@pytest.mark.parametrize("name", MC.NAN_CASES)
def test_nan_cases_are_nan_on_every_pixel(name):
    lg, ref = MC.reference(name)
    assert np.isnan(ref["conf"]).all()
    assert np.isnan(_literal(lg, MC.CASES[name])).all()              # and numpy evaluates the statements to the same


@pytest.mark.parametrize("name", FINITE)
def test_inputs_keep_their_properties(name):
    c = MC.CASES[name]
    lg, ref = MC.reference(name)
    B, Hh, Ww = c["shape"]
    assert lg.shape == (B, c["K"], Hh, Ww) and lg.dtype == np.float32 and np.isfinite(lg).all()
    assert 1 <= c["K"] - c["k_first"] <= MC.MAX_CLASSES
    assert ref["bar"].max() <= 1e-3, "the bar of %s is too wide to tell anything: %.3e" % (name, ref["bar"].max())
    assert ref["bar"].min() >= 8 * MC.EPS32
    if name not in MC.CLIP_CASES:
        return
    share = ref["clipped"].mean()
    assert 0.05 <= share <= 0.60, "clipped share %.3f" % share
    assert np.abs(ref["conf"] - ref["d"]).mean() >= 0.05             # a kernel that returned plain dissum fails
    if c["slope"] > 0:
        assert (ref["c"] < 0.5).mean() >= 0.10 and (ref["c"] > 0.5).mean() >= 0.10


def test_special_cases_are_what_they_claim():
    # the steep gate overflows float32's exp on some pixels and stays finite in float64
    for name in ("steep_softmax", "steep_logit"):
        c = MC.CASES[name]
        _, ref = MC.reference(name)
        arg = c["slope"] * (ref["d"] - c["threshold"])
        assert (arg > 89.0).mean() >= 0.10 and np.abs(ref["conf"] - ref["q"])[arg > 89.0].max() <= 1e-30
    # a zero slope is the plain mean of the two maps
    for name in ("flat_softmax", "flat_logit"):
        _, ref = MC.reference(name)
        assert np.abs(ref["conf"] - 0.5 * (ref["d"] + ref["q"])).max() <= 1e-15
    # the row: the minimum at pixel 0, the maximum, a zero sum, at the last pixel; nothing is clipped
    for name in ("zero_row_softmax", "zero_row_logit"):
        lg, ref = MC.reference(name)
        assert ref["s"][0, 0, 0] == ref["s"].min() == -128.0 and ref["s"][0, 0, -1] == ref["s"].max() == 0.0
        assert not ref["clipped"].any() and not lg[0, :, 0, -1].any()
    # the two-pixel frames put one pixel at each end of both ranges
    for name in FINITE:
        if name.startswith("px2_"):
            _, ref = MC.reference(name)
            assert sorted(ref["d"].ravel()) == [0.0, 1.0] and sorted(ref["q"].ravel()) == [0.0, 1.0]
    # the two images of a batch have different ranges
    _, ref = MC.reference("batch_k13_softmax_400")
    assert ref["s"][0].min() != ref["s"][1].min()


def test_entry_point_is_exported_and_bound():
    from dmlnet import _lib
    assert "dml_dissum_msp_score" in _lib.EXPORTS
    header = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    assert "int dml_dissum_msp_score(" in header
    lib = _lib.load()
    assert lib.dml_abi_version() == 6
    fid = lib.dml_plan_fn_id(b"dml_dissum_msp_score")
    assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(lib.dml_dissum_msp_score.argtypes) - 1 == 12
    # argument checks return before any HIP call
    assert lib.dml_dissum_msp_score(None, None, None, 1, 13, 4, 4, 0, 400.0, 0.2, 50.0, 0, None) == -1


def test_driver_parser_accepts_the_new_score():
    import eval_ood_traditional as T
    opts = T.build_parser().parse_args(["--ood", "dissum_msp", "--mix_threshold", "0.3", "--mix_slope", "20"])
    assert opts.ood == "dissum_msp" and opts.mix_threshold == 0.3 and opts.mix_slope == 20.0
    opts = T.build_parser().parse_args(["--ood", "dissum_msp"])
    assert opts.mix_threshold == 0.2 and opts.mix_slope == 50.0      # Coefficient_map(dis_sum, 0.2), lamda = 50
    assert T.build_parser().parse_args([]).ood == "dissum"           # the default stays


def test_python_surface():
    import inspect
    import utils
    sig = inspect.signature(utils.dissum_msp_score)
    assert list(sig.parameters) == ["logits", "clip", "threshold", "slope", "prob", "first_class"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [400.0, 0.2, 50.0, "softmax", 0]
    with pytest.raises(RuntimeError):
        utils.dissum_msp_score(torch.zeros(1, 13, 4, 4))             # a CPU tensor: no fallback
    assert "test_embedding.py:366-369" in utils.dissum_msp_score.__doc__
