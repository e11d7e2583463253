"""CPU: the definitions behind the pooled (dataset-level) OOD measures, before any kernel is involved.

* tests/pooled_cases.finalize_ref (Python integers and Fractions on the histogram) == oracle/ood_measures_ref.get_measures on the
  quantised scores -bin, on every case and recall level: AUROC within 1e-15, FPR equal, AUPR within open_set_cases.ood_aupr_bar of
  the quantised positives -- the project's bars for the same quantities (tests/test_open_set_refs.py).
* the oracle's AUROC of the UNquantised scores lies inside [AUROC - T / 2, AUROC + T / 2], T the tie mass.
* the bin's float32 definition on its edges; the state's counters; states add.
* plumbing: the header, the binding and the plan table know both calls; every argument check that needs no device memory; the
  drivers' flags; the accumulator's host-side checks and its refusal of CPU tensors.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import helpers as H
import open_set_cases as OC
import pooled_cases as PC
from oracle import ood_measures_ref as OR


# ---------------------------------------------------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.FINALIZE))
def test_finalize_formulas_equal_the_oracle_on_the_quantised_scores(name):
    c = PC.FINALIZE[name]
    state = PC.finalize_state(name)
    pos, neg, pos_raw, neg_raw = PC.quantised_scores(c["conf"], c["lab"], c["mask"], c["out"], c["lo"], c["hi"], c["NB"])
    assert state[:c["NB"]].sum() == pos.size and state[c["NB"]:2 * c["NB"]].sum() == neg.size
    for level in PC.LEVELS:
        r = PC.finalize_ref(state, c["NB"], level)
        assert (r["P"], r["N"]) == (pos.size, neg.size)
        if pos.size == 0 or neg.size == 0:
            assert r["auroc"] is None and r["aupr"] is None and r["fpr"] is None and r["cut"] == -1
            continue
        auroc, aupr, fpr = OR.get_measures(pos, neg, level)
        assert abs(float(r["auroc"]) - auroc) <= 1e-15, (level, float(r["auroc"]), auroc)
        assert r["fpr"] == fpr, (level, r["fpr"], fpr)
        assert abs(float(r["aupr"]) - aupr) <= OC.ood_aupr_bar(pos), (level, float(r["aupr"]), aupr)
        assert r["pos_bins"] == np.unique(pos).size and 0 <= r["cut"] < c["NB"] and state[r["cut"]] > 0
        # binning is monotone: only pairs inside one bin can change order
        exact = OR.get_measures(pos_raw, neg_raw, level)[0]
        half = float(r["tie_mass"]) / 2
        assert float(r["auroc"]) - half - 1e-15 <= exact <= float(r["auroc"]) + half + 1e-15, (float(r["auroc"]), half, exact)


def test_the_degenerate_cases_are_what_they_are_built_to_be():
    fr = lambda name, level=0.95: PC.finalize_ref(PC.finalize_state(name), PC.FINALIZE[name]["NB"], level)     # noqa: E731
    assert fr("sep_pos_low")["auroc"] == 1 and fr("sep_pos_low")["tie_mass"] == 0 and fr("sep_pos_low")["fpr"] == 0.0
    assert fr("sep_pos_high")["auroc"] == 0 and fr("sep_pos_high")["fpr"] == 1.0
    r = fr("one_bin")
    assert r["auroc"] * 2 == 1 and r["tie_mass"] == 1 and r["fpr"] == 1.0 and r["cut"] == 0 and r["aupr"] * 100 == 40
    assert fr("p1")["P"] == 1 and fr("n1")["N"] == 1 and fr("p0")["P"] == 0 and fr("n0")["N"] == 0
    # four positives in four bins: recalls 1/4 .. 1; 0.5 exists, 0.625 is half-way between 0.5 and 0.75 and takes the higher
    for level, recall in ((0.5, 0.5), (0.625, 0.75), (0.95, 1.0), (0.0, 0.25), (0.3, 0.25)):
        r = fr("recall_ties", level)
        st = PC.finalize_state("recall_ties")
        assert st[:r["cut"] + 1].sum() == 4 * recall, (level, r["cut"])


def test_the_big_state_needs_more_than_64_bits():
    st = PC.big_state()
    r = PC.finalize_ref(st, 4096, 0.95)
    assert 2.9e11 < r["P"] < 3.0e11 and 2.9e11 < r["N"] < 3.0e11
    assert r["auroc"].numerator * (2 * r["P"] * r["N"] // r["auroc"].denominator) > 2 ** 64
    assert 0 < r["pos_bins"] < 4096 and Fraction_in_unit(r["auroc"]) and Fraction_in_unit(r["aupr"])


def Fraction_in_unit(f):
    return 0 < f < 1


# ---------------------------------------------------------------------------------------------------------------------
# the bin and the state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", PC.RANGES)
@pytest.mark.parametrize("NB", PC.NBS)
def test_bin_on_its_edges(lo, hi, NB):
    v = PC.edge_values(lo, hi, NB)
    b = PC.bin32(v, lo, hi, NB)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        assert (b[np.isnan(v)] == -1).all() and (b[~np.isnan(v)] >= 0).all() and (b < NB).all()
        assert (b[v >= hi32] == NB - 1).all() and (b[v <= lo32] == 0).all()
    assert b[np.isposinf(v)] == NB - 1 and b[np.isneginf(v)] == 0
    zeros = PC.bin32(np.array([0.0, -0.0], np.float32), lo, hi, NB)
    assert zeros[0] == zeros[1]
    # monotone: a larger confidence never lands in a lower bin
    fin = np.sort(v[~np.isnan(v)])
    assert (np.diff(PC.bin32(fin, lo, hi, NB)) >= 0).all()
    # against float64 the bin is off by at most one, and only next to an edge
    inside = fin[(fin > lo32) & (fin < hi32)].astype(np.float64)
    b64 = np.minimum(np.floor((inside - np.float64(lo32)) * NB / (np.float64(hi32) - np.float64(lo32))), NB - 1)
    assert (np.abs(PC.bin32(inside.astype(np.float32), lo, hi, NB) - b64) <= 1).all()


def test_state_counters_and_additivity():
    conf, lab, m = PC.frame(4000, -37.5, 2.25, 77, OC.OOD_OUT8, edges_nb=4095, mask=True)
    NB = 4095
    st = PC.state_ref(conf, lab, m, OC.OOD_OUT8, -37.5, 2.25, NB)
    keep = m != 0
    with np.errstate(invalid="ignore"):
        assert st[2 * NB + 0] == (np.isnan(conf) & keep).sum() and st[2 * NB + 3] == (~keep).sum() and st[2 * NB + 4] == 1
        assert st[2 * NB + 1] == ((conf < np.float32(-37.5)) & keep).sum() > 0
        assert st[2 * NB + 2] == ((conf > np.float32(2.25)) & keep).sum() > 0
    assert st[:2 * NB].sum() + st[2 * NB] + st[2 * NB + 3] == conf.size
    assert st[:NB].sum() == (np.isin(lab, OC.OOD_OUT8) & keep & ~np.isnan(conf)).sum()
    # three updates == one update on the concatenation, except for the frame count
    parts = np.array_split(np.arange(conf.size), 3)
    acc = None
    for p in parts:
        acc = PC.state_ref(conf[p], lab[p], m[p], OC.OOD_OUT8, -37.5, 2.25, NB, acc)
    assert np.array_equal(acc[:-1], st[:-1]) and acc[-1] == 3
    assert np.array_equal(PC.state_ref(conf[:0], lab[:0], None, OC.OOD_OUT8, -37.5, 2.25, NB), np.zeros(2 * NB + 5, np.int64))


def test_case_tables_cover_the_issue():
    assert PC.NBS == (1, 2, 3, 4095, 4096, 8192) and PC.LEVELS == (0.95, 0.5, 0.999)
    assert PC.SIZES[:8] == (0, 1, 63, 64, 65, PC.SPAN - 1, PC.SPAN, PC.SPAN + 1) and PC.SIZES[-1] > PC.MAX_BLOCKS * PC.SPAN
    assert (-37.5, 2.25) in PC.RANGES
    for name in ("sep_pos_low", "sep_pos_high", "one_bin", "p1", "n1", "p0", "out8_masked_edges", "one_each"):
        assert name in PC.FINALIZE
    assert {PC.FINALIZE[n]["NB"] for n in PC.FINALIZE} >= {1, 2, 3, 17, 256, 4095, 4096, 8192}
    v = PC.edge_values(0.0, 1.0, 4096)
    assert np.isnan(v).any() and np.isinf(v).sum() == 2 and (np.abs(v[v != 0]) < 1e-40).any() and np.signbit(v[v == 0]).any()


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_planned():
    from dmlnet import _lib
    hdr = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("dml_pooled_ood_update", 10), ("dml_pooled_ood_finalize", 4)):
        assert name in _lib.EXPORTS and re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M)
        fid = lib.dml_plan_fn_id(name.encode())
        assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(getattr(lib, name).argtypes) - 1 == nargs
    assert lib.dml_abi_version() == 6
    assert (_lib.POOLED_OOD_SPAN, _lib.POOLED_OOD_MAX_BLOCKS) == (PC.SPAN, PC.MAX_BLOCKS)
    assert (_lib.POOLED_OOD_MAX_BINS, _lib.POOLED_OOD_MAX_OUT, _lib.POOLED_OOD_COUNTERS) == (PC.MAX_BINS, PC.MAX_OUT, PC.COUNTERS)
    src = open(os.path.join(H.PKG, "csrc", "pooled_ood.hip")).read()
    assert "POOLED_MAX_BINS = %d" % PC.MAX_BINS in src and "POOLED_MAX_BLOCKS = %d" % PC.MAX_BLOCKS in src
    assert "POOLED_THREADS = 256, POOLED_PX = 8" in src and PC.SPAN == 256 * 8
    assert "pooled_ood.hip" in open(os.path.join(H.PKG, "csrc", "Makefile")).read()


def test_argument_checks_return_before_any_launch():
    """every code that needs no device memory: the checks run on the host, before the first HIP call"""
    import ctypes as C
    from dmlnet import _lib
    lib = _lib.load()
    P = 4096                                                           # a stand-in for a device address: never dereferenced
    out = (C.c_int64 * 8)(*OC.OOD_OUT8)

    def update(conf=P, lab=P, mask=None, n=16, ol=out, n_out=1, lo=0.0, hi=1.0, NB=4096, state=P):
        return lib.dml_pooled_ood_update(conf, lab, mask, n, ol, n_out, lo, hi, NB, state, None)

    def finalize(state=P, NB=4096, level=0.95, result=P):
        return lib.dml_pooled_ood_finalize(state, NB, level, result, None)

    inf, nan, big = float("inf"), float("nan"), 3.0e38
    for kw in ({"conf": None}, {"lab": None}, {"ol": None}, {"state": None}, {"n": -1}, {"NB": 0}, {"NB": -4}, {"NB": 8193},
               {"n_out": 0}, {"n_out": 9}, {"n_out": -1}, {"lo": 1.0}, {"lo": 2.0}, {"hi": 0.0}, {"hi": -1.0}, {"lo": nan},
               {"hi": nan}, {"lo": -inf}, {"hi": inf}, {"lo": -big, "hi": big}):
        assert update(**kw) == -1, kw
    for kw in ({"conf": P + 2}, {"conf": P + 1}, {"lab": P + 4}, {"state": P + 4}, {"state": P + 1}):
        assert update(**kw) == -2, kw
    assert update(n=0) == 0 and update(n=0, mask=P + 1, conf=P + 4, n_out=8, NB=1, lo=-37.5, hi=2.25) == 0       # a no-op
    assert update(n=2 ** 41 + 2 ** 30) == -3 and update(n=2 ** 62) == -3                  # a workgroup's 32-bit cells
    for kw in ({"state": None}, {"result": None}, {"NB": 0}, {"NB": 8193}, {"level": nan}):
        assert finalize(**kw) == -1, kw
    assert finalize(state=P + 4) == -2 and finalize(result=P + 4) == -2


def test_driver_flags_and_signatures():
    import eval_ood_rec as R
    import eval_ood_traditional as T
    for mod, ood in ((T, "dissum"), (R, "rec")):
        p = mod.build_parser()
        o = p.parse_args([])
        assert (o.pooled, o.pooled_bins, tuple(o.pooled_range), o.pooled_curve, o.ood) == (False, 4096, (0.0, 1.0), "", ood)
        o = p.parse_args(["--synthetic", "--pooled", "--pooled_bins", "256", "--pooled_range", "-37.5", "2.25", "--pooled_curve",
                          "c.npz", "--num_images", "2"])
        assert (o.pooled, o.pooled_bins, list(o.pooled_range), o.pooled_curve, o.num_images) == (True, 256, [-37.5, 2.25], "c.npz", 2)
        assert T.make_pooled(o, (13,)).bins == 256 and T.make_pooled(p.parse_args([]), (13,)) is None
        for bad in (["--pooled_range", "0"], ["--pooled_bins", "many"], ["--pooled_bins"], ["--ood", "nonsense"],
                    ["--pooled_range", "a", "b"], ["--dtype", "f64"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
        help_text = " ".join(p.format_help().split())
        assert "--pooled_range LO HI" in help_text and "maxlogit, background and knn" in help_text
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(["--open_set_thresholds", "0.5"])  # still not one of that driver's flags
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--ood", "rec"])
    acc = T.make_pooled(T.build_parser().parse_args(["--pooled", "--pooled_bins", "17", "--pooled_range", "-3", "5"]), (13, 7))
    assert (acc.bins, acc.lo, acc.hi, acc.out_labels, acc.recall_level, acc.state) == (17, -3.0, 5.0, (13, 7), 0.95, None)
    # eval_ood_rec.evaluate takes the accumulator as its last keyword; eval_ood_traditional.evaluate's parameter list is pinned by
    # tests/test_open_sweep_refs.py and tests/test_ecdf_refs.py, so there it travels in the module's settings, as the calibration
    sig = inspect.signature(R.evaluate)
    assert list(sig.parameters)[-1] == "pooled" and sig.parameters["pooled"].default is None
    assert list(inspect.signature(T.evaluate).parameters)[-1] == "open_set_thresholds"
    assert T.POOLED["measures"] is None
    with T.use_pooled(acc) as held:
        assert held is acc and T.POOLED["measures"] is acc
    assert T.POOLED["measures"] is None
    with pytest.raises(KeyError):
        with T.use_pooled(acc):
            raise KeyError("out")
    assert T.POOLED["measures"] is None


def test_accumulator_on_the_host():
    """what needs no kernel: the constructor's checks, merge's refusal, the refusal of CPU tensors"""
    import anom_utils
    A = anom_utils.PooledOodMeasures
    for kw in ({"out_labels": ()}, {"out_labels": tuple(range(9))}, {"bins": 0}, {"bins": 8193}, {"lo": 1.0}, {"hi": float("inf")},
               {"lo": float("nan")}, {"lo": -3e38, "hi": 3e38}, {"recall_level": float("nan")}):
        args = {"out_labels": (13,), **kw}
        with pytest.raises(ValueError):
            A(**args)
    a = A(OC.OOD_OUT8, lo=-37.5, hi=2.25, bins=4095, recall_level=0.5)
    assert a.out_labels == OC.OOD_OUT8 and (a.lo, a.hi, a.bins, a.recall_level) == (-37.5, 2.25, 4095, 0.5) and a.state is None
    assert A((13,), lo=0.1).lo == float(np.float32(0.1))                 # the range is what the kernel sees: float32
    for other in (A(OC.OOD_OUT8, lo=-37.5, hi=2.25, bins=4096), A(OC.OOD_OUT8, lo=-37.0, hi=2.25, bins=4095),
                  A(OC.OOD_OUT8[:7], lo=-37.5, hi=2.25, bins=4095), A(OC.OOD_OUT8, lo=-37.5, hi=2.5, bins=4095), object()):
        with pytest.raises(ValueError):
            a.merge(other)
    assert a.merge(A(OC.OOD_OUT8, lo=-37.5, hi=2.25, bins=4095)) is a and a.state is None     # nothing to add yet
    conf, lab = torch.zeros(8), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(TypeError, match="no CPU fallback"):
        a.update(conf, lab)
    with pytest.raises(TypeError):
        a.update(conf.numpy(), lab)
    assert a.state is None
    sd = a.state_dict()
    assert sd["state"].dtype == torch.int64 and sd["state"].numel() == 2 * 4095 + 5 and not sd["state"].any()
    assert (sd["lo"], sd["hi"], sd["bins"], sd["out_labels"], sd["recall_level"]) == (-37.5, 2.25, 4095, list(OC.OOD_OUT8), 0.5)
    with pytest.raises(ValueError):
        A((13,)).load_state_dict(sd)
    a.reset()
    assert a.state is None
