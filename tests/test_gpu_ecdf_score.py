"""GPU: the per-class ECDF certainty score -- dml_ecdf_collect, dml_ecdf_table and dml_ecdf_score (csrc/ecdf_score.hip) through the
C ABI, through utils.EcdfCalibrator and through the open-set driver's `--ood ecdf`.

Every array a kernel reads or writes lies between two 256-byte guards of 0xAA bytes that must come back untouched.
  collect   exact integer equality with tests/ecdf_cases.collect_ref (the bitwise-defined distance sum and bin make that possible),
            on seeded random frames and on constructed ones.
  table     modes 0 and 2 bit for bit against ecdf_cases.table_ref; mode 1 within table_bar on every entry.
  score     within ecdf_cases.score_bar on EVERY pixel against the float64 definition on the same float32 logits and table; the
            NaN pattern must be the definition's exactly.
Each float check prints "MEASURE <case> err=<largest error> bar=<bar> worst err/bar=<largest share>" before it asserts.
Largest share measured on one MI355X: score 0.108 of the bar (ecdf_k13), sigmoid table 0.41 (the calibrator's, 13 x 2048).

Single-line mutants of the kernels, each built as a second library and run against this file on the device:
  an exclusive prefix sum in the table         caught by test_table_bitwise
  `>=` for `>` at the cut                      caught by test_table_ecdf_equal_to_the_cut and test_table_bitwise
  `label - k_first` dropped in collect         caught by test_collect_exact, every first1 case
  `>=` for `>` in the arg-max (last maximum)   caught by test_collect_ties_and_frames_without_a_match alone: random logits have no ties
  `s > clip` for `s >= clip` in bin()          survives, and has to: at s == clip the product s * inv_w is NB or just below it, and
                                               the last bin's clamp gives NB - 1 either way.  The `>=` is the header's wording of
                                               one behaviour, not a second one.
  the last bin's clamp removed                 not run on the device: it counts one cell past the histogram.
                                               tests/test_ecdf_refs.py shows on the host that the constructed sums hold a value below
                                               the clip whose product reaches NB (clip 1000, 1024 bins: the float below 1000), and
                                               test_collect_edges / test_score_edges feed that value to the kernels.
"""
import numpy as np
import pytest
import torch

import ecdf_cases as EC
import helpers as H  # noqa: F401  (puts the package on sys.path)

pytestmark = pytest.mark.gpu

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
F32, F64 = np.float32, np.float64
GUARD = 256                      # bytes before and after every array: 0xAA, and the array keeps its 256-byte alignment


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """a device array between two 0xAA guards; `off` bytes move it off its 256-byte alignment"""

    def __init__(self, arr=None, nbytes=None, off=0):
        self.nbytes = int(arr.nbytes if arr is not None else nbytes)
        self.off = off
        self.buf = torch.full((GUARD + off + self.nbytes + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        if arr is not None and self.nbytes:
            flat = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
            self.buf[GUARD + off:GUARD + off + self.nbytes] = torch.from_numpy(np.array(flat)).cuda()
        self.ptr = self.buf.data_ptr() + GUARD + off

    def read(self, dtype, shape):
        host = self.buf.cpu().numpy()
        lo, hi = GUARD + self.off, GUARD + self.off + self.nbytes
        assert (host[:lo] == 0xAA).all() and (host[hi:] == 0xAA).all(), "a guard byte was written"
        return host[lo:hi].copy().view(dtype).reshape(shape)


def run_collect(lib, lg, lab, k_first, clip, NB, hist0=None, offs=(0, 0, 0), rc_want=0):
    B, K, Hh, Ww = lg.shape
    Kn = K - k_first
    hist0 = np.zeros((Kn, NB), np.int64) if hist0 is None else hist0
    dl, dlab, dh = Dev(lg, off=offs[0]), Dev(lab, off=offs[1]), Dev(hist0, off=offs[2])
    rc = lib.dml_ecdf_collect(dl.ptr, dlab.ptr, dh.ptr, B, K, Hh, Ww, k_first, clip, NB, st())
    assert rc == rc_want, "dml_ecdf_collect returned %d" % rc
    torch.cuda.synchronize()
    dl.read(F32, lg.shape), dlab.read(np.int64, lab.shape)             # the inputs' guards
    return dh.read(np.int64, (Kn, NB))


def run_table(lib, hist, Kp, mode, cut=0.15, slope=50.0, thr=None, clip=400.0, offs=(0, 0)):
    Kn, NB = hist.shape
    dh, dt = Dev(hist, off=offs[0]), Dev(nbytes=4 * NB * Kp)
    dthr = None if thr is None else Dev(np.asarray(thr, F32), off=offs[1])
    rc = lib.dml_ecdf_table(dh.ptr, dt.ptr, None if dthr is None else dthr.ptr, Kn, Kp, NB, clip, mode, cut, slope, st())
    assert rc == 0, "dml_ecdf_table returned %d" % rc
    torch.cuda.synchronize()
    assert np.array_equal(dh.read(np.int64, hist.shape), hist)
    return dt.read(F32, (NB, Kp))


def run_score(lib, lg, table, k_first, clip, offs=(0, 0)):
    B, K, Hh, Ww = lg.shape
    dl, dt, dc = Dev(lg, off=offs[0]), Dev(table), Dev(nbytes=4 * B * Hh * Ww, off=offs[1])
    rc = lib.dml_ecdf_score(dl.ptr, dt.ptr, dc.ptr, B, K, Hh, Ww, k_first, table.shape[1], clip, table.shape[0], st())
    assert rc == 0, "dml_ecdf_score returned %d" % rc
    torch.cuda.synchronize()
    dl.read(F32, lg.shape), dt.read(F32, table.shape)
    return dc.read(F32, (B, Hh, Ww))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(what, got, want, bar):
    """the definition's NaN pattern exactly, every other element to the bar (a scalar or an array)"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: %d NaN, the definition has %d" % (what, np.isnan(got).sum(), nan.sum())
    bar = np.broadcast_to(np.asarray(bar, F64), want.shape)
    err = np.where(nan, 0.0, np.abs(got.astype(F64) - np.where(nan, 0.0, want)))
    share = err[~nan] / np.maximum(bar[~nan], 2.0 ** -149) if (~nan).any() else np.zeros(1)      # a zero bar: err must be 0
    print("MEASURE %s err=%.3e bar=%.3e worst err/bar=%.3e" % (what, err.max(), bar.max(), share.max()))
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, "%s: %d elements above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]])
    return share.max()


# ---------------------------------------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.COLLECT))
def test_collect_exact(lib, name):
    c = EC.COLLECT[name]
    lg, lab = EC.collect_inputs(name)
    want = EC.collect_ref(lg, lab, c["k_first"], c["clip"], c["NB"])
    got = run_collect(lib, lg, lab, c["k_first"], c["clip"], c["NB"])
    assert np.array_equal(got, want), "%d cells differ, counted %d of %d" % ((got != want).sum(), got.sum(), want.sum())
    if lg.shape[0] * lg.shape[2] * lg.shape[3] > 64:
        assert want.sum() > 0 and (want.sum(axis=1) > 0).sum() >= min(2, want.shape[0])


@pytest.mark.parametrize("clip,NB", [(400.0, 1024), (1000.0, 1024), (400.0, 2048), (1000.0, 2), (400.0, 1)])
def test_collect_edges(lib, clip, NB):
    """K = 1: sums exactly on a bin edge and one ulp either side, == clip, > clip, < 0, both zeros, the infinities and NaN"""
    lg, lab = EC.edge_inputs(clip, NB)
    want = EC.collect_ref(lg, lab, 0, clip, NB)
    assert want.sum() == lg.size - 1                                   # all but the NaN
    assert np.array_equal(run_collect(lib, lg, lab, 0, clip, NB), want)
    # the same sums as the second of two classes: k_first = 1 and a first plane that must not count
    lg2 = np.concatenate([np.full_like(lg, 1e30), lg], axis=1)
    assert np.array_equal(run_collect(lib, lg2, lab + 1, 1, clip, NB), want)


def test_collect_ties_and_frames_without_a_match(lib):
    lg, lab, counts = EC.tie_inputs()
    want = EC.collect_ref(lg, lab, 1, 400.0, 8)
    assert want.sum() == counts.sum()
    assert np.array_equal(run_collect(lib, lg, lab, 1, 400.0, 8), want)
    # no pixel matches: every label ignored, out of range, below k_first or another class than the prediction
    lg, lab = EC.collect_inputs("kn13_first1")
    K = lg.shape[1]
    pred = EC.pred_first(lg, 1) + 1
    for other in (np.full_like(lab, 255), np.full_like(lab, -1), np.full_like(lab, K), np.zeros_like(lab),
                  1 + (pred - 1 + 1) % (K - 1)):
        seed = np.zeros((K - 1, 2048), np.int64)
        seed[3, 7] = 5
        assert np.array_equal(run_collect(lib, lg, other.astype(np.int64), 1, 400.0, 2048, hist0=seed), seed)


def test_collect_accumulates(lib):
    """two frames into one histogram, onto a cell that already holds 2^33"""
    la, laba = EC.collect_inputs("kn13_first0")
    lb, labb = EC.collect_inputs("nb2048_clip400")
    seed = np.zeros((13, 2048), np.int64)
    first = EC.collect_ref(la, laba, 0, 400.0, 2048)
    cell = np.unravel_index(np.argmax(first), first.shape)
    seed[cell] = 2 ** 33
    h1 = run_collect(lib, la, laba, 0, 400.0, 2048, hist0=seed)
    assert np.array_equal(h1, seed + first) and h1[cell] > 2 ** 33
    h2 = run_collect(lib, lb, labb, 0, 400.0, 2048, hist0=h1)
    assert np.array_equal(h2, EC.collect_ref(lb, labb, 0, 400.0, 2048, hist=h1))
    # and the result does not depend on the run
    assert np.array_equal(h2, run_collect(lib, lb, labb, 0, 400.0, 2048, hist0=h1))


@pytest.mark.parametrize("name", EC.OFFSET_CASES)
def test_collect_pointers_one_element_off(lib, name):
    """logits 4 bytes, labels 8 bytes, the histogram 8 bytes off a 16-byte boundary: each alone and all together"""
    c = EC.COLLECT[name]
    lg, lab = EC.collect_inputs(name)
    want = EC.collect_ref(lg, lab, c["k_first"], c["clip"], c["NB"])
    for offs in ((4, 0, 0), (0, 8, 0), (0, 0, 8), (4, 8, 8)):
        assert np.array_equal(run_collect(lib, lg, lab, c["k_first"], c["clip"], c["NB"], offs=offs), want), offs


def test_collect_error_codes(lib):
    lg, lab = EC.collect_inputs("px64")
    dl, dlab = Dev(lg), Dev(lab)
    dh = Dev(np.zeros((32, 1024), np.int64))

    def call(l=dl.ptr, y=dlab.ptr, h=dh.ptr, B=1, K=13, Hh=1, Ww=64, k_first=0, clip=400.0, NB=1024):
        return lib.dml_ecdf_collect(l, y, h, B, K, Hh, Ww, k_first, clip, NB, st())

    assert call(l=None) == EINVAL and call(y=None) == EINVAL and call(h=None) == EINVAL
    for kw in ({"B": 0}, {"K": 0}, {"Hh": 0}, {"Ww": 0}, {"B": -1}, {"Ww": -3}, {"k_first": -1}, {"k_first": 13}, {"clip": 0.0},
               {"clip": -400.0}, {"clip": float("inf")}, {"clip": float("nan")}, {"NB": 0}, {"NB": -1}):
        assert call(**kw) == EINVAL, kw
    for kw in ({"K": 33}, {"K": 34, "k_first": 1}, {"NB": 2049}, {"K": 17, "NB": 2048}, {"K": 32, "NB": 1025}, {"B": 65536},
               {"B": 2, "Hh": 2 ** 20, "Ww": 2 ** 20}, {"B": 65535, "Hh": 2 ** 30, "Ww": 2 ** 30}):
        assert call(**kw) == EUNSUPPORTED, kw
    assert call(l=dl.ptr + 2) == EALIGN and call(y=dlab.ptr + 4) == EALIGN and call(h=dh.ptr + 4) == EALIGN
    torch.cuda.synchronize()
    assert (dh.read(np.int64, (32, 1024)) == 0).all()                  # nothing was launched, and the guards are intact
    dl.read(F32, lg.shape), dlab.read(np.int64, lab.shape)


# ---------------------------------------------------------------------------------------------------------------------
# table
# ---------------------------------------------------------------------------------------------------------------------
def _cut_hist(NB):
    """three classes whose ECDF hits the cut exactly: 1/4 of 4 samples (cut 0.25), and float32(0.15) of 2^26 samples"""
    h = np.zeros((3, NB), np.int64)
    h[0, 0], h[0, NB // 2], h[0, NB - 1] = 1, 1, 2
    m = int(np.float64(F32(0.15)) * 2 ** 26)
    assert m / 2 ** 26 == np.float64(F32(0.15))
    h[1, 1], h[1, NB - 1] = m, 2 ** 26 - m
    h[2, 0], h[2, 1], h[2, NB - 1] = m - 1, 2, 2 ** 26 - m - 1         # one sample below the cut, then one above
    return h


@pytest.mark.parametrize("Kn,Kp,NB", [(13, 16, 1024), (16, 16, 2048), (1, 4, 1), (2, 4, 2), (19, 20, 1000), (32, 32, 1024),
                                       (13, 20, 257)])
def test_table_bitwise(lib, Kn, Kp, NB):
    """modes 0 and 2 bit for bit: an empty class, a one-sample class, a count beyond 2^32, padding columns"""
    h = EC.calib_hist(Kn, NB, 40 + Kn, empty=(Kn - 1,) if Kn > 1 else (), single=(0,) if Kn > 2 else ())
    if Kn > 4:
        h[2, NB // 3] += 2 ** 33
    for mode in (0, 2):
        for cut in (0.15, 0.5):
            want, _ = EC.table_ref(h, Kp, mode, cut=cut)
            got = run_table(lib, h, Kp, mode, cut=cut, offs=(8, 0))
            assert np.array_equal(bits(got), bits(want)), "mode %d cut %g: %d entries differ" % (mode, cut, (got != want).sum())
    if Kn > 1:
        assert (got[:, Kn - 1] == 1.0).all()                           # the empty class passes through
    assert (got[:, Kn:] == 0.0).all()
    # an all-empty histogram
    z = np.zeros_like(h)
    assert np.array_equal(bits(run_table(lib, z, Kp, 0)), bits(EC.table_ref(z, Kp, 0)[0]))


def test_table_ecdf_equal_to_the_cut(lib):
    for NB in (4, 1024):
        h = _cut_hist(NB)
        for cut in (0.25, float(F32(0.15))):
            want, _ = EC.table_ref(h, 4, 0, cut=cut)
            got = run_table(lib, h, 4, 0, cut=cut)
            assert np.array_equal(bits(got), bits(want))
        assert got[1, 1] == F32(0.15) and got[0, 2] < F32(0.15) and got[1, 2] == 1.0      # E == cut stays E


@pytest.mark.parametrize("Kn,Kp,NB,clip,slope", [(13, 16, 1024, 400.0, 50.0), (19, 20, 1024, 1000.0, 20.0), (3, 4, 2048, 400.0, 200.0)])
def test_table_sigmoid_within_the_bar(lib, Kn, Kp, NB, clip, slope):
    h = EC.calib_hist(Kn, NB, 90 + Kn, empty=(Kn - 1,), single=(0,))
    thr = np.linspace(-5.0, 1.1 * clip, Kn).astype(F32)
    want, bar = EC.table_ref(h, Kp, 1, slope=slope, thresholds=thr, clip=clip)
    got = run_table(lib, h, Kp, 1, slope=slope, thr=thr, clip=clip, offs=(0, 4))
    check("sigmoid table %d x %d" % (Kn, NB), got[:, :Kn], want[:, :Kn], bar[:, :Kn])
    assert (got[:, Kn:] == 0.0).all() and (got[:, Kn - 1] == 1.0).all()
    assert np.array_equal(bits(got), bits(run_table(lib, h, Kp, 1, slope=slope, thr=thr, clip=clip)))
    # a NaN threshold: NaN certainties for that class alone
    thr2 = thr.copy()
    thr2[1] = np.nan
    got2 = run_table(lib, h, Kp, 1, slope=slope, thr=thr2, clip=clip)
    assert np.isnan(got2[:, 1]).all() and np.array_equal(bits(np.delete(got2, 1, axis=1)), bits(np.delete(got, 1, axis=1)))


def test_table_error_codes(lib):
    h = EC.calib_hist(13, 1024, 5)
    dh, dt, dthr = Dev(h), Dev(nbytes=4 * 1024 * 16), Dev(np.zeros(13, F32))

    def call(hh=dh.ptr, t=dt.ptr, thr=None, Kn=13, Kp=16, NB=1024, clip=400.0, mode=0):
        return lib.dml_ecdf_table(hh, t, thr, Kn, Kp, NB, clip, mode, 0.15, 50.0, st())

    for kw in ({"hh": None}, {"t": None}, {"Kn": 0}, {"NB": 0}, {"clip": 0.0}, {"clip": float("inf")}, {"Kp": 14}, {"Kp": 12},
               {"mode": 3}, {"mode": -1}, {"mode": 1}):
        assert call(**kw) == EINVAL, kw
    assert call(Kn=33, Kp=36) == EUNSUPPORTED and call(NB=2049) == EUNSUPPORTED
    assert call(hh=dh.ptr + 4) == EALIGN and call(t=dt.ptr + 4) == EALIGN and call(mode=1, thr=dthr.ptr + 2) == EALIGN
    torch.cuda.synchronize()
    assert (dt.read(np.uint8, (4 * 1024 * 16,)) == 0xAA).all()


# ---------------------------------------------------------------------------------------------------------------------
# score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.SCORE))
def test_score_against_float64(lib, name):
    c = EC.SCORE[name]
    lg, table, want, bar = EC.score_inputs(name)
    got = run_score(lib, lg, table, c["k_first"], c["clip"])
    check(name, got, want, bar)
    if c["kind"] == "special":
        flat = np.isnan(want).reshape(want.shape[0], -1)
        assert flat[:, [3, 5, 6]].all() and not flat[:, [4, 7]].any() and flat.sum() == 3 * want.shape[0]
    else:
        assert not np.isnan(want).any()
    # two runs are bitwise equal
    assert np.array_equal(bits(got), bits(run_score(lib, lg, table, c["k_first"], c["clip"])))
    # image b of the batch equals the same image run alone, bitwise
    if lg.shape[0] > 1:
        for b in range(lg.shape[0]):
            alone = run_score(lib, lg[b:b + 1], table, c["k_first"], c["clip"])
            assert np.array_equal(bits(alone[0]), bits(got[b])), "image %d differs from its solo run" % b


@pytest.mark.parametrize("clip,NB", [(400.0, 1024), (1000.0, 1024), (400.0, 2048), (1000.0, 2), (400.0, 1)])
def test_score_edges(lib, clip, NB):
    """K = 1, where conf is the table entry of the pixel's bin itself: the edge sums pick exactly the definition's rows"""
    lg, _ = EC.edge_inputs(clip, NB)
    table = np.zeros((NB, 4), F32)
    table[:, 0] = (np.arange(NB) + 1.0) / (NB + 1.0)                   # every row another value
    b = EC.bin32(EC.dist_sum32(lg), clip, NB)
    want = np.where(b < 0, np.nan, table[np.maximum(b, 0), 0].astype(F64))
    want = np.where(np.isinf(lg[:, 0]), np.nan, want)                  # the only logit is the maximum: exp(inf - inf)
    got = run_score(lib, lg, table, 0, clip)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)].astype(F32))       # e = 1, num / den = t exactly


@pytest.mark.parametrize("name", EC.SCORE_OFFSET_CASES)
def test_score_pointers_one_float_off(lib, name):
    """logits or conf 4 bytes off a 16-byte boundary take the one-pixel-per-lane path: the same bits"""
    c = EC.SCORE[name]
    lg, table, want, bar = EC.score_inputs(name)
    base = run_score(lib, lg, table, c["k_first"], c["clip"])
    for offs in ((4, 0), (0, 4), (4, 4)):
        got = run_score(lib, lg, table, c["k_first"], c["clip"], offs=offs)
        check("%s offset %s" % (name, offs), got, want, bar)
        assert np.array_equal(bits(got), bits(base))


def test_score_first_class_skips_the_background(lib):
    c = EC.SCORE["kn13_first1"]
    lg, table, want, bar = EC.score_inputs("kn13_first1")
    got = run_score(lib, lg, table, 1, c["clip"])
    assert np.array_equal(bits(got), bits(run_score(lib, np.ascontiguousarray(lg[:, 1:]), table, 0, c["clip"])))
    other = np.array(lg)
    other[:, 0] = 1e30
    assert np.array_equal(bits(got), bits(run_score(lib, other, table, 1, c["clip"])))


def test_score_error_codes(lib):
    lg, table, _, _ = EC.score_inputs("odd_k13")
    dl, dt, dc = Dev(lg), Dev(table), Dev(nbytes=4 * 15)

    def call(l=dl.ptr, t=dt.ptr, o=dc.ptr, B=1, K=13, Hh=3, Ww=5, k_first=0, Kp=16, clip=400.0, NB=1024):
        return lib.dml_ecdf_score(l, t, o, B, K, Hh, Ww, k_first, Kp, clip, NB, st())

    assert call(l=None) == EINVAL and call(t=None) == EINVAL and call(o=None) == EINVAL
    for kw in ({"B": 0}, {"K": 0}, {"Hh": 0}, {"Ww": -1}, {"k_first": -1}, {"k_first": 13}, {"Kp": 15}, {"Kp": 12}, {"clip": 0.0},
               {"clip": float("nan")}, {"NB": 0}):
        assert call(**kw) == EINVAL, kw
    for kw in ({"K": 33, "Kp": 36}, {"NB": 2049}, {"B": 65536}, {"B": 2, "Hh": 2 ** 20, "Ww": 2 ** 20}):
        assert call(**kw) == EUNSUPPORTED, kw
    assert call(l=dl.ptr + 2) == EALIGN and call(o=dc.ptr + 2) == EALIGN and call(t=dt.ptr + 4) == EALIGN
    torch.cuda.synchronize()
    assert (dc.read(np.uint8, (60,)) == 0xAA).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not np.isnan(dc.read(F32, (15,))).any()


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface and the driver
# ---------------------------------------------------------------------------------------------------------------------
def test_calibrator_class(lib, tmp_path):
    import utils
    c = EC.COLLECT["kn13_first1"]
    lg, lab = EC.collect_inputs("kn13_first1")
    lg2, lab2 = EC.collect_inputs("kn13_first0")
    lg2 = np.concatenate([np.zeros_like(lg2[:, :1]), lg2], axis=1)     # 14 planes like lg
    cal = utils.EcdfCalibrator(14, c["clip"], nbins=c["NB"], first_class=1)
    cal.update(torch.from_numpy(np.array(lg)).cuda(), torch.from_numpy(lab).cuda())
    cal.update(torch.from_numpy(lg2).cuda(), torch.from_numpy(lab2 + 1).cuda())
    want = EC.collect_ref(lg2, lab2 + 1, 1, c["clip"], c["NB"], hist=EC.collect_ref(lg, lab, 1, c["clip"], c["NB"]))
    assert cal.hist.is_cuda and np.array_equal(cal.hist.cpu().numpy(), want)
    assert np.array_equal(cal.counts(), want.sum(axis=1))
    t = torch.from_numpy(np.array(lg)).cuda()
    for mode, mid in (("hard", 0), ("ecdf", 2)):
        tab = cal.table(mode)
        assert tab.is_cuda and tuple(tab.shape) == (c["NB"], 16)
        assert np.array_equal(bits(tab.cpu().numpy()), bits(EC.table_ref(want, 16, mid)[0]))
        conf = cal.score(t, mode=mode)
        assert np.array_equal(bits(conf.cpu().numpy()), bits(run_score(lib, lg, tab.cpu().numpy(), 1, c["clip"])))
        assert torch.equal(conf, utils.ecdf_certainty_score(t, tab, c["clip"], first_class=1))
    # the sigmoid mode fits its thresholds on the host when none are given
    thr = cal.fit_thresholds()
    assert thr.shape == (13,) and np.array_equal(thr, utils.fit_gmm_thresholds(want, c["clip"]))
    tab = cal.table("sigmoid")
    ref, bar = EC.table_ref(want, 16, 1, thresholds=thr.astype(F32), clip=c["clip"])
    check("calibrator sigmoid table", tab.cpu().numpy()[:, :13], ref[:, :13], bar[:, :13])
    assert (tab.cpu().numpy()[:, 13:] == 0.0).all()
    assert torch.equal(cal.table("sigmoid", thresholds=thr), tab)
    assert cal.table("sigmoid") is tab and cal.table("sigmoid", device="cuda") is tab     # "cuda" is the device it is on: kept
    conf = cal.score(t, mode="sigmoid")
    # one fit per calibration: further scores and tables use the thresholds that were fitted, an update fits anew
    fits = []
    real_fit = utils.scores.fit_gmm_thresholds
    utils.scores.fit_gmm_thresholds = lambda *a, **kw: (fits.append(1), real_fit(*a, **kw))[1]
    try:
        for _ in range(3):
            assert torch.equal(cal.score(t, mode="sigmoid"), conf)
        cal.table("sigmoid", slope=20.0)
        assert fits == []
        before = cal.hist.clone()
        cal.update(t, torch.from_numpy(lab).cuda())
        cal.score(t, mode="sigmoid")
        cal.score(t, mode="sigmoid")
        assert fits == [1]
        cal.load_state_dict(dict(cal.state_dict(), hist=before.cpu()))
        assert torch.equal(cal.score(t, mode="sigmoid"), conf) and fits == [1, 1]
    finally:
        utils.scores.fit_gmm_thresholds = real_fit
    check("calibrator sigmoid score", conf.cpu().numpy(), EC.score_ref(lg, tab.cpu().numpy(), 1, c["clip"]), EC.score_bar(13))
    # calibrate once, reuse
    path = str(tmp_path / "cal.npz")
    cal.save(path)
    back = utils.EcdfCalibrator.load(path)
    assert not back.hist.is_cuda and torch.equal(back.score(t), cal.score(t))
    with pytest.raises(TypeError):
        cal.update(t.cpu(), torch.from_numpy(lab))
    with pytest.raises(TypeError):
        cal.update(t.double(), torch.from_numpy(lab).cuda())
    with pytest.raises(ValueError):
        cal.update(t[:, 1:], torch.from_numpy(lab).cuda())
    with pytest.raises(ValueError):
        cal.table("soft")


def _tiny_frames(seg_size=(96, 128), n=2, seed=11, classes=14):
    """the smallest synthetic frames of the driver tests (tests/test_gpu_open_sweep.py)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        imgs = [torch.randn(1, 3, h, w, generator=g).cuda() for h, w in ((96, 128), (120, 160))]
        lab = torch.randint(0, classes, (seg_size[0] // 8, seg_size[1] // 8), generator=g)
        lab = lab.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()
        lab[:3] = 255
        out.append((imgs, lab.cuda()))
    return out


def test_driver_calibrates_and_evaluates(lib):
    import eval_ood_traditional as T
    import metrics
    import models
    import utils
    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights="")
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, weights="", use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).cuda().eval()
    seg.set_compute_dtype(torch.float32, fp32_products="exact")
    calib, frames = _tiny_frames(seed=5, classes=13), _tiny_frames()
    for exclude_back in (False, True):
        first = 1 if exclude_back else 0
        cal = T.calibrate(seg, calib, 13, exclude_back)
        assert (cal.num_classes, cal.first_class, cal.nbins, cal.clip) == (13, first, T.ECDF["bins"], T.ECDF["clip"])
        want = None
        for imgs, lab in calib:
            scores, _ = models.evaluate_multiscale(seg, imgs, tuple(lab.shape))
            want = EC.collect_ref(scores.cpu().numpy(), lab[None].cpu().numpy(), first, cal.clip, cal.nbins, hist=want)
        assert np.array_equal(cal.hist.cpu().numpy(), want) and want.sum() > 0
        assert T.calibrate(seg, calib, 13, exclude_back, max_frames=1).counts().sum() < want.sum()
        m = metrics.OpenSetSweepMetrics(14, (0.1, 0.5, 0.9), 13, (13,))
        with T.use_calibrator(cal) as held:
            assert held is cal and T.ECDF["calibrator"] is cal
            got = T.evaluate(seg, frames, 14, "ecdf", (13,), exclude_back, open_set_thresholds=(0.1, 0.5, 0.9))
            for imgs, lab in frames:
                scores, ft1 = models.evaluate_multiscale(seg, imgs, tuple(lab.shape))
                conf = T.confidence(scores, "ecdf", exclude_back, feats=ft1)
                assert conf.shape == lab.shape and torch.equal(conf, cal.score(scores)[0])
                assert float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0 + 1e-6
                m.update(lab, utils.argmax_msp(scores)[0], conf)
        assert T.ECDF["calibrator"] is None                              # put back on the way out
        assert len(got["open_set"]) == 3
        for a, b in zip(got["open_set"], m.get_results()):
            for k in a:
                np.testing.assert_array_equal(a[k], b[k])
        assert 0.0 <= got["auroc"] <= 1.0
    # the settings reach the kernels from where main() leaves them; the sigmoid's thresholds are fitted once for all frames
    saved = dict(T.ECDF)
    fits = []
    real_fit = utils.scores.fit_gmm_thresholds
    utils.scores.fit_gmm_thresholds = lambda *a, **kw: (fits.append(1), real_fit(*a, **kw))[1]
    try:
        T.ECDF.update(mode="sigmoid", slope=20.0)
        with T.use_calibrator(cal):
            scores, _ = models.evaluate_multiscale(seg, frames[0][0], tuple(frames[0][1].shape))
            assert torch.equal(T.confidence(scores, "ecdf", True), cal.score(scores, mode="sigmoid", slope=20.0)[0])
            T.evaluate(seg, frames, 14, "ecdf", (13,), True)
            assert len(fits) == 1, "%d mixture fits for one calibration" % len(fits)
            with pytest.raises(ValueError):
                T.confidence(scores, "ecdf", False)                      # the calibration left the background out
            with pytest.raises(RuntimeError):
                with T.use_calibrator(None):
                    assert T.ECDF["calibrator"] is None
                    raise RuntimeError("leaves through the manager")
            assert T.ECDF["calibrator"] is cal                           # the inner block put the outer one's back
        assert T.ECDF["calibrator"] is None
        with pytest.raises(ValueError):
            T.evaluate(seg, frames, 14, "ecdf", (13,))
    finally:
        utils.scores.fit_gmm_thresholds = real_fit
        T.ECDF.update(saved)
