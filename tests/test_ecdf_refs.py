"""CPU: the definitions of tests/ecdf_cases.py are what they claim -- the binned ECDF brackets the exact-sample ECDF and equals it
on bin centres, the two certainties are the reference's two `Certainty` bodies, the deterministic EM of utils.fit_gmm_thresholds
climbs, stops at a fixed point and recovers a known mixture -- and the entry points, the wrapper and the driver's flags exist.  No
kernel is launched here.

The reference lines restated below.  DeepLabV3Plus-Pytorch/main_embedding.py: :106-113 Certainty (hard: `res[res>0.15] = 1`),
:209-219 the mixture and `thre = min_mean - 1 * np.sqrt(min_cov)`, :214 `ECDF(data_list[cl])` (statsmodels: the share of the sample
<= x).  test_embedding.py: :155-162 Certainty (sigmoid, coefficient = 50 around ecdf(thre1)).
"""
import os
import re

import numpy as np
import pytest
import torch

import ecdf_cases as EC
import helpers as H

F32 = np.float32


def exact_ecdf(sample, x):
    """statsmodels' ECDF(sample)(x): the share of the sample that is <= x"""
    srt = np.sort(sample)
    return np.searchsorted(srt, x, side="right") / srt.size


def Certainty_hard(r):                                                                              # main_embedding.py:106-113
    res = np.array(r)
    res[res > 0.15] = 1
    return res


def Certainty_sigmoid(r, r_thre):                                                                   # test_embedding.py:155-162
    threshold = r_thre
    coefficient = 50
    return 1 / (1 + np.exp(-coefficient * (r - threshold)))


def _hist_of(sample, clip, NB):
    b = EC.bin32(sample.astype(F32), clip, NB)
    return np.bincount(b, minlength=NB).astype(np.int64)[None]


@pytest.mark.parametrize("clip,NB", [(400.0, 1024), (1000.0, 1024), (400.0, 2048), (400.0, 2), (1000.0, 1)])
def test_binned_ecdf_brackets_the_exact_one(clip, NB):
    """bin() is monotone, so {sample <= x} is inside {bin(sample) <= bin(x)}: E[bin(x)] >= #{s <= x} / n, and the surplus is at
    most the mass of bin(x) itself"""
    rs = np.random.RandomState(31 + NB)
    sample = np.concatenate([rs.gamma(4.0, clip / 10.0, 5000), rs.uniform(-5.0, 1.3 * clip, 300)]).astype(F32)
    s = np.sort(sample)
    assert (np.diff(EC.bin32(s, clip, NB)) >= 0).all(), "bin() is not monotone"
    hist = _hist_of(sample, clip, NB)
    E = EC.ecdf32(hist)[0].astype(np.float64)
    x = np.concatenate([sample[:2000], EC.edge_sums(clip, NB)[~np.isnan(EC.edge_sums(clip, NB))]]).astype(F32)
    bx = EC.bin32(x, clip, NB)
    exact = exact_ecdf(sample, x)
    mass = hist[0][bx] / sample.size
    assert (E[bx] >= exact - 2.0 ** -24).all()                        # the float32 rounding of E
    assert (E[bx] <= exact + mass + 2.0 ** -24).all()
    assert E[-1] == 1.0 and (np.diff(E) >= 0).all()


def test_binned_ecdf_equals_the_exact_one_on_bin_centres():
    clip, NB = 400.0, 1024
    rs = np.random.RandomState(5)
    centres = ((rs.randint(0, NB, 4000) + 0.5) * (clip / NB)).astype(F32)
    hist = _hist_of(centres, clip, NB)
    E = EC.ecdf32(hist)[0]
    x = ((np.arange(NB) + 0.5) * (clip / NB)).astype(F32)
    assert np.array_equal(EC.bin32(x, clip, NB), np.arange(NB))
    assert np.array_equal(E, exact_ecdf(centres, x).astype(F32))


def test_certainties_restate_the_reference():
    h = EC.calib_hist(5, 1024, 77, empty=(4,), single=(0,))
    E = EC.ecdf32(h)
    hard = EC.table_ref(h, 8, 0, cut=0.15)[0]
    for cl in range(4):
        assert np.array_equal(hard[:, cl], Certainty_hard(E[cl]))
    assert (hard[:, 4] == 1.0).all() and (hard[:, 5:] == 0.0).all()          # the empty class passes through; padding
    assert np.array_equal(EC.table_ref(h, 8, 2)[0][:, :4], E[:4].T)
    thr = np.array([120.0, 80.0, 200.0, 33.3, 50.0], F32)
    sig, bar = EC.table_ref(h, 8, 1, slope=50.0, thresholds=thr, clip=400.0)
    for cl in range(4):
        r_thre = E[cl][EC.bin32(thr[cl], 400.0, 1024)]
        want = Certainty_sigmoid(E[cl].astype(np.float64), np.float64(r_thre))
        assert np.abs(sig[:, cl] - want).max() <= 1e-15
        # a float32 evaluation of the reference's statement stays inside the bar
        f32 = Certainty_sigmoid(E[cl], r_thre)
        assert f32.dtype == np.float32 and (np.abs(f32.astype(np.float64) - want) <= bar[:, cl]).all()
    assert (sig[:, 4] == 1.0).all()


def test_the_last_bins_clamp_and_the_clip_rule_bite():
    """the constructed sums hold values that single-line mutants of bin() move: a product that rounds up to NB below the clip
    (the clamp), s == clip (>= against >), zero of both signs and negative sums"""
    s = EC.edge_sums(1000.0, 1024)
    inv_w = F32(1024) / F32(1000.0)
    below = s[(s < F32(1000.0)) & (s > 0)]
    assert ((below * inv_w).astype(np.int64) == 1024).any(), "no sum below the clip reaches NB without the clamp"
    b = EC.bin32(s, 1000.0, 1024)
    assert b[s == F32(1000.0)][0] == 1023 and (b[np.isnan(s)] == -1).all() and (b[s <= 0] == 0).all()
    assert b[np.isposinf(s)][0] == 1023 and b[np.isneginf(s)][0] == 0
    # an edge is the first value of its bin: one ulp below it sits in the bin before
    e = F32(5 * 1000.0 / 1024)
    assert EC.bin32(np.array([EC.OC.down(e), e]), 1000.0, 1024).tolist() == [4, 5]
    # the K = 1 frame carries exactly these sums, and a zero sum is +0.0 whatever the logit's sign
    lg, lab = EC.edge_inputs(1000.0, 1024)
    got = EC.dist_sum32(lg)[0, 0]
    assert np.array_equal(got[~np.isnan(s)], s[~np.isnan(s)]) and np.isnan(got[np.isnan(s)]).all()
    assert (s == 0).sum() >= 2 and not np.signbit(got[s == 0]).any()


def test_collect_definition_on_a_hand_made_frame():
    lg, lab, counts = EC.tie_inputs()
    h = EC.collect_ref(lg, lab, 1, 400.0, 8)
    assert h.sum() == counts.sum() == 3
    s = EC.dist_sum32(lg, 1)[0, 0]
    for p in np.flatnonzero(counts):
        assert h[lab[0, 0, p] - 1, EC.bin32(s[p], 400.0, 8)] >= 1
    # accumulation
    assert np.array_equal(EC.collect_ref(lg, lab, 1, 400.0, 8, hist=h), 2 * h)


def test_case_tables_cover_the_issue():
    for n in (1, 2, 63, 64, 65):
        assert "px%d" % n in EC.COLLECT
    for Kn in (1, 2, 13, 16, 19, 23, 32):
        for k_first in (0, 1):
            assert "kn%d_first%d" % (Kn, k_first) in EC.COLLECT and "kn%d_first%d" % (Kn, k_first) in EC.SCORE
    for c in EC.COLLECT.values():
        assert (c["K"] - c["k_first"]) * c["NB"] <= EC.MAX_CELLS
    assert any((c["K"] - c["k_first"]) * c["NB"] == EC.MAX_CELLS for c in EC.COLLECT.values())
    assert {c["NB"] for c in EC.COLLECT.values()} >= {1, 2, 1024, 2048}
    for sname in EC.SHAPES:
        assert sname + "_k13" in EC.SCORE and sname + "_k19" in EC.SCORE
    # the looping cases do loop: more passes per image than workgroups per image
    for name in ("loop_scalar_k2", "loop_vec_k2", "loop_one_image_k2"):
        B, Hh, Ww = EC.COLLECT[name]["shape"]
        per = Hh * Ww // 4 if (Hh * Ww) % 4 == 0 else Hh * Ww
        assert -(-per // EC.THREADS) > max(1, EC.MAX_BLOCKS // B)


# ---------------------------------------------------------------------------------------------------------------------
# the mixture fit
# ---------------------------------------------------------------------------------------------------------------------
# the known mixture: N = 400,000 draws, 60 % from N(90, 6^2) and 40 % from N(230, 40^2), on the 1024 bins of [0, 400]
MIX_N, MIX_PI, MIX_MU, MIX_SD = 400000, (0.6, 0.4), (90.0, 230.0), (6.0, 40.0)


def _mixture_hist():
    rs = np.random.RandomState(2024)
    n1 = rs.binomial(MIX_N, MIX_PI[0])
    x = np.concatenate([rs.normal(MIX_MU[0], MIX_SD[0], n1), rs.normal(MIX_MU[1], MIX_SD[1], MIX_N - n1)])
    return _hist_of(x, 400.0, 1024)[0], n1


def test_em_climbs_and_stops_at_a_fixed_point():
    from utils.scores import _em_two_gaussians
    hist, _ = _mixture_hist()
    w = 400.0 / 1024
    x = (np.arange(1024) + 0.5) * w
    floor = w * w / 12.0 + 1e-6
    pi, mu, var, trace = _em_two_gaussians(x, hist.astype(np.float64), floor)
    assert 2 <= len(trace) <= 500
    assert (np.diff(trace) >= -1e-12 * np.abs(trace[:-1])).all(), "the log-likelihood fell"
    assert len(trace) == 500 or trace[-1] - trace[-2] < 1e-9 * abs(trace[-2])
    # the M-step equations at the returned parameters: one more E- and M-step moves them by no more than the last step could have
    c = hist.astype(np.float64)
    logp = np.log(pi)[:, None] - 0.5 * np.log(2 * np.pi * var)[:, None] - (x[None] - mu[:, None]) ** 2 / (2 * var[:, None])
    lse = np.logaddexp(logp[0], logp[1])
    assert abs((c * lse).sum() - trace[-1]) <= 1e-9 * abs(trace[-1])
    r = np.exp(logp - lse) * c
    nj = r.sum(axis=1)
    mu2 = (r * x).sum(axis=1) / nj
    var2 = np.maximum((r * (x - mu2[:, None]) ** 2).sum(axis=1) / nj, floor)
    # a relative log-likelihood gain below 1e-9 bounds the step: the likelihood is locally quadratic, so parameters move by about
    # sqrt(gain); 1e-3 relative to each component's standard deviation is that with room
    assert (np.abs(mu2 - mu) <= 1e-3 * np.sqrt(var)).all() and (np.abs(var2 - var) <= 2e-3 * var).all()
    assert (np.abs(nj / c.sum() - pi) <= 1e-3).all()
    # deterministic
    again = _em_two_gaussians(x, hist.astype(np.float64), floor)
    assert np.array_equal(again[1], mu) and np.array_equal(again[2], var) and again[3] == trace


def test_em_recovers_the_narrow_component():
    import utils
    hist, n1 = _mixture_hist()
    thr = utils.fit_gmm_thresholds(np.stack([hist, np.zeros_like(hist)]), 400.0)
    w = 400.0 / 1024
    # standard errors of the narrow component's mean and standard deviation from n1 draws: sd / sqrt(n1) and sd / sqrt(2 n1); the
    # threshold is mean - sd, so 5 standard errors of each plus half a bin width (the sample is only known to its bins)
    se = MIX_SD[0] / np.sqrt(n1) + MIX_SD[0] / np.sqrt(2.0 * n1)
    want = MIX_MU[0] - MIX_SD[0]
    print("MEASURE gmm threshold %.4f, mixture %.4f, bound %.4f" % (thr[0], want, 5 * se + 0.5 * w))
    assert abs(thr[0] - want) <= 5.0 * se + 0.5 * w
    assert thr[1] == 0.0                                               # an empty class


def test_fit_thresholds_small_classes():
    import utils
    h = np.zeros((4, 16), np.int64)
    h[1, 5] = 9                                                        # one occupied bin: its centre
    h[2, 3], h[2, 11] = 4, 1                                           # two occupied bins: the fit runs
    h[3, 2], h[3, 3] = 1, 10                                           # the weighted median is the last occupied bin
    thr = utils.fit_gmm_thresholds(h, 400.0)
    assert thr[0] == 0.0 and thr[1] == 5.5 * 25.0 and np.isfinite(thr).all()
    assert np.array_equal(thr, utils.fit_gmm_thresholds(h, 400.0))


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_planned():
    from dmlnet import _lib
    hdr = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("dml_ecdf_collect", 10), ("dml_ecdf_table", 10), ("dml_ecdf_score", 11)):
        assert name in _lib.EXPORTS and re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M)
        fid = lib.dml_plan_fn_id(name.encode())
        assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(getattr(lib, name).argtypes) - 1 == nargs
    assert lib.dml_abi_version() == 6
    assert (_lib.ECDF_THREADS, _lib.ECDF_MAX_BLOCKS) == (EC.THREADS, EC.MAX_BLOCKS)
    assert (_lib.ECDF_MAX_CLASSES, _lib.ECDF_MAX_BINS, _lib.ECDF_MAX_CELLS) == (EC.MAX_CLASSES, EC.MAX_BINS, EC.MAX_CELLS)
    src = open(os.path.join(H.PKG, "csrc", "ecdf_score.hip")).read()
    assert "ECDF_THREADS = %d" % EC.THREADS in src and "ECDF_MAX_BLOCKS = %d" % EC.MAX_BLOCKS in src
    assert "ECDF_KREG = %d" % EC.REG_CLASSES in src


def test_argument_checks_return_before_any_launch():
    """every code that needs no device memory: the checks run on the host, before the first HIP call"""
    from dmlnet import _lib
    lib = _lib.load()
    P, T16 = 4096, 4096                                                # stand-ins for device addresses: never dereferenced

    def collect(lg=P, lab=P, hist=P, B=1, K=13, Hh=4, Ww=4, k_first=0, clip=400.0, NB=1024):
        return lib.dml_ecdf_collect(lg, lab, hist, B, K, Hh, Ww, k_first, clip, NB, None)

    def table(hist=P, tab=T16, thr=None, Kn=13, Kp=16, NB=1024, clip=400.0, mode=0):
        return lib.dml_ecdf_table(hist, tab, thr, Kn, Kp, NB, clip, mode, 0.15, 50.0, None)

    def score(lg=P, tab=T16, conf=P, B=1, K=13, Hh=4, Ww=4, k_first=0, Kp=16, clip=400.0, NB=1024):
        return lib.dml_ecdf_score(lg, tab, conf, B, K, Hh, Ww, k_first, Kp, clip, NB, None)

    for f in (collect, score):
        for kw in ({"lg": None}, {"B": 0}, {"K": 0}, {"Hh": 0}, {"Ww": -1}, {"k_first": -1}, {"k_first": 13}, {"clip": 0.0},
                   {"clip": -1.0}, {"clip": float("inf")}, {"clip": float("nan")}, {"NB": 0}):
            assert f(**kw) == -1, kw
        wide = {"Kp": 40} if f is score else {}
        for kw in ({"K": 33}, {"K": 40, "k_first": 7}, {"NB": 2049}, {"B": 65536}, {"B": 2, "Hh": 2 ** 20, "Ww": 2 ** 20},
                   {"B": 65535, "Hh": 2 ** 30, "Ww": 2 ** 30}):
            assert f(**kw, **wide) == -3, kw
        assert f(lg=P + 2) == -2
    assert collect(lab=None) == -1 and collect(hist=None) == -1
    assert collect(K=17, NB=2048) == -3 and collect(K=32, NB=1025) == -3          # the LDS limit
    assert collect(lab=P + 4) == -2 and collect(hist=P + 4) == -2
    assert score(tab=None) == -1 and score(conf=None) == -1 and score(Kp=15) == -1 and score(Kp=12) == -1
    assert score(conf=P + 1) == -2 and score(tab=T16 + 4) == -2 and score(tab=T16 + 8) == -2
    for kw in ({"hist": None}, {"tab": None}, {"Kn": 0}, {"NB": 0}, {"clip": 0.0}, {"clip": float("nan")}, {"Kp": 14}, {"Kp": 12},
               {"mode": 3}, {"mode": -1}, {"mode": 1}):
        assert table(**kw) == -1, kw
    assert table(Kn=33, Kp=36) == -3 and table(NB=2049) == -3
    assert table(hist=P + 4) == -2 and table(tab=T16 + 4) == -2 and table(mode=1, thr=P + 2) == -2


def test_driver_flags_and_the_missing_calibration():
    import eval_ood_traditional as T
    opts = T.build_parser().parse_args(["--ood", "ecdf", "--ecdf_mode", "sigmoid", "--ecdf_cut", "0.2", "--ecdf_slope", "20",
                                        "--ecdf_bins", "512", "--ecdf_clip", "1000", "--ecdf_calib", "3", "--ecdf_load", "a.npz",
                                        "--ecdf_save", "b.npz"])
    assert (opts.ood, opts.ecdf_mode, opts.ecdf_cut, opts.ecdf_slope, opts.ecdf_bins, opts.ecdf_clip, opts.ecdf_calib,
            opts.ecdf_load, opts.ecdf_save) == ("ecdf", "sigmoid", 0.2, 20.0, 512, 1000.0, 3, "a.npz", "b.npz")
    opts = T.build_parser().parse_args(["--ood", "ecdf"])
    assert (opts.ecdf_mode, opts.ecdf_cut, opts.ecdf_slope, opts.ecdf_bins, opts.ecdf_clip, opts.ecdf_calib, opts.ecdf_load,
            opts.ecdf_save) == ("hard", 0.15, 50.0, 1024, 400.0, None, "", "")
    with pytest.raises(SystemExit) as e:
        T.check_ecdf_source(opts)
    assert "--ecdf_calib" in str(e.value) and "--ecdf_load" in str(e.value)
    T.check_ecdf_source(T.build_parser().parse_args(["--ood", "ecdf", "--ecdf_load", "a.npz"]))
    T.check_ecdf_source(T.build_parser().parse_args(["--ood", "ecdf", "--ecdf_calib", "0"]))
    with pytest.raises(SystemExit):
        T.check_ecdf_source(T.build_parser().parse_args(["--synthetic", "--ood", "ecdf", "--ecdf_calib", "0"]))
    T.check_ecdf_source(T.build_parser().parse_args(["--ood", "dissum"]))
    assert T.CFG_DEFAULTS["DATASET.list_calib"] == "./data/training.odgt"
    # the calibration travels in the module's settings, as the gates of dissum_msp and crf-gauss do: the two signatures that
    # tests/test_knn_refs.py and tests/test_open_sweep_refs.py pin are what they were
    import inspect
    assert list(inspect.signature(T.confidence).parameters) == ["scores", "ood", "exclude_back", "feats"]
    assert list(inspect.signature(T.evaluate).parameters)[-1] == "open_set_thresholds"
    assert T.ECDF["calibrator"] is None
    with pytest.raises(ValueError):
        T.confidence(torch.zeros(1, 13, 4, 4), "ecdf")                 # no calibration
    import utils
    cal = utils.EcdfCalibrator(13, 400.0, first_class=1)
    with T.use_calibrator(cal) as held:
        assert held is cal and T.ECDF["calibrator"] is cal
        with pytest.raises(ValueError):
            T.confidence(torch.zeros(1, 13, 4, 4), "ecdf", False)      # calibrated without the background, asked with it
        with pytest.raises(TypeError):
            T.confidence(torch.zeros(1, 13, 4, 4), "ecdf", True)       # a CPU tensor: no fallback
    assert T.ECDF["calibrator"] is None                                # put back, also when the block raises
    with pytest.raises(KeyError):
        with T.use_calibrator(cal):
            raise KeyError("out")
    assert T.ECDF["calibrator"] is None


def test_calibrator_on_the_host(tmp_path):
    """what needs no kernel: the constructor's checks, the refusal of CPU tensors, state_dict and save / load"""
    import utils
    cal = utils.EcdfCalibrator(14, 400.0, nbins=1024, first_class=1)
    assert cal.n_known == 13 and tuple(cal.hist.shape) == (13, 1024) and cal.hist.dtype == torch.int64
    assert cal.counts().tolist() == [0] * 13
    with pytest.raises(TypeError):
        cal.update(torch.zeros(1, 14, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))       # CPU tensors: no fallback
    with pytest.raises(TypeError):
        cal.score(torch.zeros(1, 14, 4, 4))
    with pytest.raises(TypeError):
        utils.ecdf_certainty_score(torch.zeros(1, 14, 4, 4), torch.zeros(1024, 16), 400.0)
    for bad in ((14, 400.0, 1024, 14), (40, 400.0, 1024, 0), (14, 0.0, 1024, 0), (14, float("inf"), 1024, 0), (14, 400.0, 0, 0),
                (14, 400.0, 4096, 0), (32, 400.0, 2048, 0)):
        with pytest.raises(ValueError):
            utils.EcdfCalibrator(*bad)
    h = EC.calib_hist(13, 1024, 3, empty=(12,), single=(0,))
    h[5, 17] = 2 ** 33 + 5
    cal.load_state_dict({"hist": torch.from_numpy(h), "num_classes": 14, "clip": 400.0, "nbins": 1024, "first_class": 1})
    assert np.array_equal(cal.counts(), h.sum(axis=1))
    path = str(tmp_path / "calibration.npz")
    cal.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["clip", "first_class", "hist", "nbins", "num_classes"] and z["hist"].dtype == np.int64
    back = utils.EcdfCalibrator.load(path)
    assert (back.num_classes, back.clip, back.nbins, back.first_class) == (14, 400.0, 1024, 1)
    assert np.array_equal(back.hist.numpy(), h)
    sd = back.state_dict()
    sd["hist"][0, 0] += 1                                              # a copy: the calibrator keeps its own
    assert np.array_equal(back.hist.numpy(), h)
    with pytest.raises(ValueError):
        utils.EcdfCalibrator(13, 400.0).load_state_dict(cal.state_dict())
    assert np.array_equal(back.fit_thresholds(), utils.fit_gmm_thresholds(h, 400.0))
    # fitted once per calibration: a second call does not fit again, a new histogram does, and the caller gets a copy
    fits = []
    real_fit = utils.scores.fit_gmm_thresholds
    utils.scores.fit_gmm_thresholds = lambda *a, **kw: (fits.append(1), real_fit(*a, **kw))[1]
    try:
        first = back.fit_thresholds()
        assert fits == []
        first[0] = -1.0
        assert back.fit_thresholds()[0] != -1.0
        back.load_state_dict(cal.state_dict())
        assert np.array_equal(back.fit_thresholds(), real_fit(h, 400.0)) and fits == [1]
        back.fit_thresholds()
        assert fits == [1]
    finally:
        utils.scores.fit_gmm_thresholds = real_fit
    assert "main_embedding.py:106-113" in utils.EcdfCalibrator.__doc__
