"""GPU: the pooled (dataset-level) OOD measures -- dml_pooled_ood_update / dml_pooled_ood_finalize through the C ABI and through
anom_utils.PooledOodMeasures -- against tests/pooled_cases.py.  The histogram is integer: every comparison of a state is exact
equality with the numpy definition, and the state sits between guard elements that must come back untouched.  The finalize is
compared with the Fraction reference under the bars derived in pooled_cases' docstring.
"""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import helpers as H
import open_set_cases as OC
import pooled_cases as PC

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 64, -7          # int64 elements before and after the state, and what they hold
EPS64 = PC.EPS64


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    assert (_lib.POOLED_OOD_SPAN, _lib.POOLED_OOD_MAX_BLOCKS) == (PC.SPAN, PC.MAX_BLOCKS)
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a, offset=0):
    """a host array on the device behind `offset` elements: (buffer, pointer to the first element of the copy)"""
    t = torch.from_numpy(np.array(a))
    buf = torch.zeros(t.numel() + offset + 1, dtype=t.dtype, device="cuda")          # one spare element: never a NULL pointer
    buf[offset:offset + t.numel()] = t.cuda()
    return buf, buf.data_ptr() + offset * t.element_size()


def run_update(lib, frames, out, lo, hi, NB, state0=None, offset=0):
    """dml_pooled_ood_update once per (conf, lab, mask) of `frames` onto one state -> int64 [2 NB + 5] as numpy.  `offset` moves
    every device pointer off its 16-byte boundary by one element."""
    n_state = 2 * NB + PC.COUNTERS
    sbuf = torch.full((n_state + 2 * GUARD + offset,), GUARD_VALUE, dtype=torch.int64, device="cuda")
    sbuf[GUARD + offset:GUARD + offset + n_state] = 0 if state0 is None else torch.from_numpy(np.array(state0)).cuda()
    oo = (C.c_int64 * len(out))(*out)
    keep = []
    for conf, lab, mask in frames:
        bufs = [dev(np.asarray(conf, np.float32), offset), dev(np.asarray(lab, np.int64), offset),
                dev(np.asarray(mask, np.uint8), offset) if mask is not None else (None, None)]
        keep.append((bufs, (conf, lab, mask)))
        rc = lib.dml_pooled_ood_update(bufs[0][1], bufs[1][1], bufs[2][1], int(np.asarray(conf).size), oo, len(out), lo, hi, NB,
                                       sbuf.data_ptr() + 8 * (GUARD + offset), st())
        assert rc == 0, "dml_pooled_ood_update returned %d" % rc
    torch.cuda.synchronize()
    s = sbuf.cpu().numpy()[offset:]
    assert (s[:GUARD] == GUARD_VALUE).all() and (s[GUARD + n_state:] == GUARD_VALUE).all(), "a guard element of the state was written"
    for bufs, arrs in keep:                                              # the inputs are read only
        for (buf, _), a, dt in zip(bufs, arrs, (np.float32, np.int64, np.uint8)):
            if buf is not None:
                a = np.asarray(a, dt).reshape(-1)
                assert np.array_equal(buf.cpu().numpy()[offset:offset + a.size].view(np.uint8), a.view(np.uint8))
    return s[GUARD:GUARD + n_state]


def run_finalize(lib, state, NB, level):
    """dml_pooled_ood_finalize on a host state -> float64 [8]"""
    sbuf, sp = dev(np.asarray(state, np.int64))
    rbuf = torch.full((8 + 2 * GUARD,), -5.0, dtype=torch.float64, device="cuda")
    rc = lib.dml_pooled_ood_finalize(sp, NB, level, rbuf.data_ptr() + 8 * GUARD, st())
    assert rc == 0, "dml_pooled_ood_finalize returned %d" % rc
    torch.cuda.synchronize()
    r = rbuf.cpu().numpy()
    assert (r[:GUARD] == -5.0).all() and (r[GUARD + 8:] == -5.0).all(), "a guard element of the result was written"
    assert np.array_equal(sbuf.cpu().numpy()[:-1], np.asarray(state, np.int64)), "the state was written"
    return r[GUARD:GUARD + 8]


def check_finalize(got, ref, what):
    """float64 result[8] of the kernel against finalize_ref's exact values, under pooled_cases' bars"""
    assert (got[3], got[4]) == (ref["P"], ref["N"]) and got[7] == 0.0, what
    if ref["P"] == 0 or ref["N"] == 0:
        assert np.isnan(got[[0, 1, 2, 5]]).all() and got[6] == -1.0, what
        return
    for idx, key in ((0, "auroc"), (5, "tie_mass")):
        err, bar = abs(Fraction(float(got[idx])) - ref[key]), 4 * Fraction(EPS64) * ref[key]
        print("%s %s: got %.17g, error %.3g, bar %.3g" % (what, key, got[idx], float(err), float(bar)))
        assert err <= bar, (what, key, got[idx], float(ref[key]))
    err, bar = abs(Fraction(float(got[1])) - ref["aupr"]), (ref["pos_bins"] + 4) * Fraction(EPS64)
    print("%s aupr: got %.17g, error %.3g, bar %.3g" % (what, got[1], float(err), float(bar)))
    assert err <= bar, (what, got[1], float(ref["aupr"]))
    assert got[2] == ref["fpr"] and got[6] == ref["cut"], (what, got[2], ref["fpr"], got[6], ref["cut"])


# ---------------------------------------------------------------------------------------------------------------------
# the histogram
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,n", list(enumerate(PC.SIZES)))
def test_histogram_at_every_size(lib, i, n):
    """0, 1, 63 .. 65 pixels, a pass minus one / exact / plus one, and the first size at which workgroups make a second pass"""
    NB, (lo, hi) = PC.NBS[i % len(PC.NBS)], PC.RANGES[i % 2]
    conf, lab, mask = PC.frame(n, lo, hi, 9500 + i, edges_nb=NB if n > 100 else 0, mask=bool(i % 2))
    got = run_update(lib, [(conf, lab, mask)], PC.OUT1, lo, hi, NB)
    want = PC.state_ref(conf, lab, mask, PC.OUT1, lo, hi, NB)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert got[-1] == (1 if n else 0) and got[:2 * NB].sum() + got[2 * NB] + got[2 * NB + 3] == n


@pytest.mark.parametrize("lo,hi", PC.RANGES)
@pytest.mark.parametrize("NB", PC.NBS)
def test_histogram_at_every_bin_count_on_the_edges(lib, NB, lo, hi):
    """lo and hi and one ulp either side, bin edges and their neighbours, both zeros, subnormals, the infinities, NaN; eight
    out-labels with ids below 0 and above 2^31; with and without a mask; every pointer one element off its 16-byte boundary"""
    conf, lab, mask = PC.frame(PC.SPAN + 77, lo, hi, 9600 + NB, OC.OOD_OUT8, edges_nb=NB, mask=True)
    edges = PC.edge_values(lo, hi, NB).size
    mask[:edges] = 1                                                     # the edge values are all counted ...
    for m in (None, mask):
        got = run_update(lib, [(conf, lab, m)], OC.OOD_OUT8, lo, hi, NB, offset=0 if m is None else 1)
        want = PC.state_ref(conf, lab, m, OC.OOD_OUT8, lo, hi, NB)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert got[2 * NB] == 1 and got[2 * NB + 1] >= 4 and got[2 * NB + 2] >= 4          # ... NaN once, and the outside ones
    both = np.isin(lab, OC.OOD_OUT8)                                     # ... and as positives and as negatives alike
    for flip in (both, ~both):
        lab2 = np.where(flip, 13, 1)
        lab2[:edges] = np.where(flip[:edges], 1, 13)
        got = run_update(lib, [(conf, lab2, None)], PC.OUT1, lo, hi, NB)
        assert np.array_equal(got, PC.state_ref(conf, lab2, None, PC.OUT1, lo, hi, NB))


def test_labels_mask_and_accumulation(lib):
    """OOD_OUT8; the mask that leaves one positive and one negative; three updates == one update on the concatenation, bit for
    bit; accumulation onto counts beyond 2^32; two runs give identical states"""
    conf, lab = OC.ood_labelled()
    lo, hi, NB = -2.75, 2.0, 256                                        # narrower than the confidences: both sides are outside
    whole = run_update(lib, [(conf, lab, None)], OC.OOD_OUT8, lo, hi, NB)
    assert np.array_equal(whole, PC.state_ref(conf, lab, None, OC.OOD_OUT8, lo, hi, NB))
    assert whole[:NB].sum() == np.isin(lab, OC.OOD_OUT8).sum() and whole[2 * NB + 1] > 0
    parts = np.array_split(np.arange(conf.size), 3)
    three = run_update(lib, [(conf[p], lab[p], None) for p in parts], OC.OOD_OUT8, lo, hi, NB)
    assert np.array_equal(three[:-1], whole[:-1]) and three[-1] == 3
    again = run_update(lib, [(conf[p], lab[p], None) for p in parts], OC.OOD_OUT8, lo, hi, NB)
    assert np.array_equal(again, three)
    start = np.full(2 * NB + PC.COUNTERS, 2 ** 33 + 5, np.int64)
    onto = run_update(lib, [(conf, lab, None)], OC.OOD_OUT8, lo, hi, NB, state0=start)
    assert np.array_equal(onto, whole + start)
    conf, lab, mask = OC.ood_one_each()
    got = run_update(lib, [(conf, lab, mask.astype(np.uint8))], PC.OUT1, -4.0, 4.0, 4096)
    assert np.array_equal(got, PC.state_ref(conf, lab, mask, PC.OUT1, -4.0, 4.0, 4096))
    assert got[:4096].sum() == 1 and got[4096:8192].sum() == 1 and got[2 * 4096 + 3] == conf.size - 2
    # any non-zero mask byte counts
    m = (np.arange(conf.size) % 5).astype(np.uint8) * 63
    assert np.array_equal(run_update(lib, [(conf, lab, m)], PC.OUT1, -4.0, 4.0, 17), PC.state_ref(conf, lab, m, PC.OUT1, -4.0, 4.0, 17))


@pytest.mark.parametrize("NB", (1, 4096, 8192))
def test_one_bin_takes_every_pixel(lib, NB):
    """every lane of every wave adds to the same LDS cell"""
    n = 300007
    conf = np.full(n, 0.6251, np.float32)
    lab = np.ones(n, np.int64)
    got = run_update(lib, [(conf, lab, None)], PC.OUT1, 0.0, 1.0, NB)
    b = int(PC.bin32(conf[:1], 0.0, 1.0, NB)[0])
    assert got[NB + b] == n and got.sum() == n + 1
    lab[::3] = 13
    got = run_update(lib, [(conf, lab, None)], PC.OUT1, 0.0, 1.0, NB)
    assert got[b] == (n + 2) // 3 and got[NB + b] == n - (n + 2) // 3 and got.sum() == n + 1


# ---------------------------------------------------------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.FINALIZE))
def test_finalize_on_accumulated_states(lib, name):
    """the state accumulated on the device in three updates equals the definition's; its measures at recall 0.95, 0.5 and 0.999
    against the Fraction reference"""
    c = PC.FINALIZE[name]
    parts = np.array_split(np.arange(c["conf"].size), 3)
    frames = [(c["conf"][p], c["lab"][p], None if c["mask"] is None else c["mask"][p]) for p in parts]
    state = run_update(lib, frames, c["out"], c["lo"], c["hi"], c["NB"])
    assert np.array_equal(state, PC.finalize_state(name))
    for level in PC.LEVELS:
        check_finalize(run_finalize(lib, state, c["NB"], level), PC.finalize_ref(state, c["NB"], level), "%s @ %g" % (name, level))


def test_finalize_named_values(lib):
    fin = lambda name: run_finalize(lib, PC.finalize_state(name), PC.FINALIZE[name]["NB"], 0.95)      # noqa: E731
    assert fin("sep_pos_low")[0] == 1.0 and fin("sep_pos_low")[5] == 0.0 and fin("sep_pos_low")[2] == 0.0
    assert fin("sep_pos_high")[0] == 0.0 and fin("sep_pos_high")[2] == 1.0
    r = fin("one_bin")
    assert r[0] == 0.5 and r[5] == 1.0 and r[2] == 1.0 and r[6] == 0 and r[1] == 0.4
    assert fin("p1")[3] == 1 and fin("n1")[4] == 1
    for name in ("p0", "n0"):
        r = fin(name)
        assert np.isnan(r[0]) and np.isnan(r[1]) and np.isnan(r[2]) and r[3] + r[4] == 3000 and r[3] * r[4] == 0


@pytest.mark.parametrize("NB", (4096, 8192, 4095))
def test_finalize_beyond_64_bits(lib, NB):
    """a state written directly with about 3 10^11 counts per class: the AUROC numerator is about 10^23.  A numerator summed in 64
    bits wraps and fails this."""
    state = PC.big_state(NB, seed=9400 + NB)
    for level in (0.95, 0.5):
        ref = PC.finalize_ref(state, NB, level)
        assert ref["auroc"] * 2 * ref["P"] * ref["N"] > 2 ** 64
        check_finalize(run_finalize(lib, state, NB, level), ref, "big nb%d @ %g" % (NB, level))
    # 2^40 pixels, all in two bins: the largest products the header promises
    state = np.zeros(2 * NB + PC.COUNTERS, np.int64)
    state[[3, NB - 1]] = 2 ** 38, 2 ** 38
    state[[NB + 3, 2 * NB - 1]] = 2 ** 37, 3 * 2 ** 37
    check_finalize(run_finalize(lib, state, NB, 0.95), PC.finalize_ref(state, NB, 0.95), "2^40 nb%d" % NB)


# ---------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_state_alone(lib):
    NB = 256
    conf, cp = dev(np.linspace(0, 1, 64, dtype=np.float32), 1)
    lab, lp = dev(np.ones(64, np.int64), 1)
    state = torch.zeros(2 * NB + PC.COUNTERS + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(9, dtype=torch.float64, device="cuda")
    sp, rp = state.data_ptr(), res.data_ptr()
    out = (C.c_int64 * 8)(*OC.OOD_OUT8)
    inf, nan = float("inf"), float("nan")

    def update(conf=cp, lab=lp, mask=None, n=64, ol=out, n_out=8, lo=0.0, hi=1.0, NB=NB, state=sp):
        return lib.dml_pooled_ood_update(conf, lab, mask, n, ol, n_out, lo, hi, NB, state, st())

    for kw in ({"conf": None}, {"lab": None}, {"ol": None}, {"state": None}, {"n": -1}, {"NB": 0}, {"NB": 8193}, {"n_out": 0},
               {"n_out": 9}, {"lo": 1.0}, {"hi": -0.5}, {"lo": nan}, {"hi": nan}, {"lo": -inf}, {"hi": inf}, {"lo": -3e38, "hi": 3e38}):
        assert update(**kw) == -1, kw
    for kw in ({"conf": cp + 2}, {"lab": lp + 4}, {"state": sp + 4}):
        assert update(**kw) == -2, kw
    assert update(n=0) == 0
    assert lib.dml_pooled_ood_finalize(None, NB, 0.95, rp, st()) == -1 and lib.dml_pooled_ood_finalize(sp, NB, 0.95, None, st()) == -1
    assert lib.dml_pooled_ood_finalize(sp, 0, 0.95, rp, st()) == -1 and lib.dml_pooled_ood_finalize(sp, 8193, 0.95, rp, st()) == -1
    assert lib.dml_pooled_ood_finalize(sp, NB, nan, rp, st()) == -1
    assert lib.dml_pooled_ood_finalize(sp + 4, NB, 0.95, rp, st()) == -2 and lib.dml_pooled_ood_finalize(sp, NB, 0.95, rp + 4, st()) == -2
    torch.cuda.synchronize()
    assert not state.any() and not res.any()                             # nothing was launched
    assert update(state=sp + 8) == 0                                     # natural alignment is enough
    torch.cuda.synchronize()
    assert state[1:1 + 2 * NB].sum() == 64 and state[0] == 0
    import anom_utils
    acc = anom_utils.PooledOodMeasures((13,))
    with pytest.raises(TypeError, match="no CPU fallback"):
        acc.update(torch.zeros(8), torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(8, device="cuda", dtype=torch.float64), torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda"), mask=torch.ones(8))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(8, device="cuda"), torch.zeros(7, dtype=torch.int64, device="cuda"))
    assert acc.state is None and acc.get_results() is None


# ---------------------------------------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------------------------------------
def test_accumulator_class(lib):
    import anom_utils
    c = PC.FINALIZE["out8_masked_edges"]
    lo, hi, NB = c["lo"], c["hi"], c["NB"]
    parts = np.array_split(np.arange(c["conf"].size), 3)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                                 # noqa: E731
    new = lambda level=0.95: anom_utils.PooledOodMeasures(c["out"], lo=lo, hi=hi, bins=NB, recall_level=level)     # noqa: E731
    a = new()
    for p in parts:
        a.update(cuda(c["conf"][p]).reshape(1, -1), cuda(c["lab"][p]).reshape(1, -1), cuda(c["mask"][p]).reshape(1, -1) != 0)
    want = PC.finalize_state("out8_masked_edges")
    assert np.array_equal(a.state.cpu().numpy(), want)
    # merge: two accumulators over disjoint frames add up to the one over all of them
    b1, b2 = new(), new()
    b1.update(cuda(c["conf"][parts[0]]), cuda(c["lab"][parts[0]]), cuda(c["mask"][parts[0]]))
    for p in parts[1:]:
        b2.update(cuda(c["conf"][p]), cuda(c["lab"][p]), cuda(c["mask"][p]))
    assert b1.merge(b2) is b1 and np.array_equal(b1.state.cpu().numpy(), want)
    empty = new()
    assert empty.merge(a) is empty and np.array_equal(empty.state.cpu().numpy(), want) and empty.state is not a.state
    # results
    ref = PC.finalize_ref(want, NB, 0.95)
    r = a.get_results()
    check_finalize(np.array([r["auroc"], r["aupr"], r["fpr"], r["positives"], r["negatives"], r["tie_mass"], r["cut_bin"], 0.0]),
                   ref, "class")
    assert set(r) >= {"auroc", "aupr", "fpr", "positives", "negatives", "tie_mass", "auroc_bounds", "n_nan", "n_below", "n_above",
                      "frames"}
    assert (r["n_nan"], r["n_below"], r["n_above"], r["n_masked"], r["frames"]) == tuple(int(v) for v in want[2 * NB:])
    assert r["auroc_bounds"] == (r["auroc"] - 0.5 * r["tie_mass"], r["auroc"] + 0.5 * r["tie_mass"])
    t = a.threshold_at_recall()
    assert t == np.float64(a.lo) + (ref["cut"] + 1) * (np.float64(a.hi) - np.float64(a.lo)) / NB == r["threshold"]
    # every counted pixel below the threshold sits in a bin up to the cut-off bin, which holds a positive
    tp, fp, edges = a.curve()
    assert tp.dtype == np.int64 and np.array_equal(tp, np.cumsum(want[:NB])) and np.array_equal(fp, np.cumsum(want[NB:2 * NB]))
    assert edges.shape == (NB + 1,) and edges[0] == a.lo and edges[-1] == a.hi and edges[ref["cut"] + 1] == t
    assert fp[ref["cut"]] <= round(ref["fpr"] * ref["N"]) <= fp[-1]
    # another recall level is another accumulator over the same state
    sd = a.state_dict()
    half = new(0.5)
    half.load_state_dict(sd)
    assert np.array_equal(half.state.cpu().numpy(), want) and half.state.is_cuda
    assert half.get_results()["cut_bin"] == PC.finalize_ref(want, NB, 0.5)["cut"]
    half.update(cuda(c["conf"][parts[0]]), cuda(c["lab"][parts[0]]))                                  # resumed
    assert np.array_equal(a.state.cpu().numpy(), want)                                               # and no state is shared
    a.reset()
    assert not a.state.any() and a.get_results() is None and a.threshold_at_recall() is None
    only_neg = new()
    only_neg.update(cuda(c["conf"]), torch.ones(c["conf"].size, dtype=torch.int64, device="cuda"))
    assert only_neg.get_results() is None


# ---------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_frames(seg_size=(96, 128), n=2):
    g = torch.Generator().manual_seed(11)
    out = []
    for _ in range(n):
        imgs = [torch.randn(1, 3, h, w, generator=g).cuda() for h, w in ((96, 128), (120, 160))]
        lab = torch.randint(0, 14, (seg_size[0] // 8, seg_size[1] // 8), generator=g)
        lab = lab.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()
        lab[:3] = 255
        out.append((imgs, lab.cuda()))
    return out


def test_driver_evaluate_returns_the_pooled_measures():
    import anom_utils
    import eval_ood_traditional as T
    import models
    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights="")
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, weights="", use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).cuda().eval()
    seg.set_compute_dtype(torch.float32, fp32_products="exact")
    frames = _tiny_frames()
    base = T.evaluate(seg, frames, 14, "msp", (13,))
    assert "pooled" not in base
    acc = anom_utils.PooledOodMeasures((13,), bins=256)
    with T.use_pooled(acc):
        got = T.evaluate(seg, frames, 14, "msp", (13,))
    assert T.POOLED["measures"] is None and set(got) == set(base) | {"pooled"}
    for k in ("auroc", "aupr", "fpr"):
        assert got[k] == base[k] or (np.isnan(got[k]) and np.isnan(base[k])), k
    assert np.array_equal(got["known_iou"], base["known_iou"])
    # the class fed by hand with the driver's own conf / label
    mine = anom_utils.PooledOodMeasures((13,), bins=256)
    confs = []
    for imgs, lab in frames:
        scores, ft1 = models.evaluate_multiscale(seg, imgs, tuple(lab.shape))
        confs.append(T.confidence(scores, "msp", False, feats=ft1))
        mine.update(confs[-1], lab)
    assert torch.equal(mine.state, acc.state) and got["pooled"] == mine.get_results()
    p = got["pooled"]
    assert p is not None, acc.state[-5:].tolist()                        # msp: finite on every pixel, whatever the weights
    assert p["frames"] == 2 and p["positives"] + p["negatives"] + p["n_nan"] == 2 * 96 * 128 and p["n_below"] == p["n_above"] == 0
    want = PC.state_ref(torch.stack(confs).cpu().numpy(), torch.stack([f[1] for f in frames]).cpu().numpy(), None, (13,), 0.0, 1.0, 256)
    assert np.array_equal(acc.state.cpu().numpy()[:-1], want[:-1])
    check_finalize(np.array([p["auroc"], p["aupr"], p["fpr"], p["positives"], p["negatives"], p["tie_mass"], p["cut_bin"], 0.0]),
                   PC.finalize_ref(want, 256, 0.95), "driver")


def test_evaluation_driver_with_pooled(tmp_path):
    """eval_ood_traditional.py --synthetic --pooled end to end at a small frame size, in a child process (msp: the untrained model's
    `dissum` map is constant, and its per-frame normalisation 0 / 0)"""
    drv = os.path.join(H.PKG, "eval_ood_traditional.py")
    curve = str(tmp_path / "curve.npz")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--ood", "msp", "--pooled", "--pooled_bins", "512", "--pooled_curve",
                        curve, "--num_images", "2", "--height", "360", "--width", "640", "--dtype", "bf16"], capture_output=True,
                       text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("mean auroc = ")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("pooled auroc = "), r.stdout[-2000:]
    ln = lines[at[0] + 1]
    for word in ("pooled aupr = ", "pooled fpr = ", "auroc bounds = [", "threshold at recall 0.95 = ", "below range = 0 above range = 0"):
        assert word in ln, ln
    assert 0.0 <= float(ln.split("pooled auroc = ")[1].split()[0]) <= 1.0
    z = np.load(curve)
    assert z["tp"].shape == z["fp"].shape == (512,) and z["edges"].shape == (513,)
    nan = int(ln.split(" nan = ")[1].split()[0])
    assert z["tp"][-1] + z["fp"][-1] + nan == 2 * 360 * 640 and z["tp"][-1] > 0 and z["fp"][-1] > 0
