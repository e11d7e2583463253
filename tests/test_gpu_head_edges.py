"""GPU: the pixel-to-prototype distance head at its edges, through the C ABI -- dml_proto_dist_fwd, dml_upsample_dist_fwd,
dml_proto_dist_bwd (csrc/head.hip) and dml_proto_dist_nhwc (csrc/pool_resize.hip) on every case of tests/head_cases.py.

Every comparison is against the float64 definitions of tests/head_cases.py on the same float32 inputs (proved right on these inputs,
without a GPU, by tests/test_head_refs.py) and goes through head_cases.check_head / check_close / check_argmax, the functions whose
teeth that file shows.  Exact (dyadic) inputs must be reproduced EXACTLY, the first maximum of every tie included; real-valued
inputs per element against bars that count the float32 roundings of the contract, with the argmax free only at near-ties inside
those bars.  The feature copy of dml_proto_dist_fwd is compared bit for bit (-0.0 and NaN included); an inf and a NaN in the
upsampled head's embedding go through head_cases.check_propagation.  Every output sits between two
guard regions of 0xAA bytes, each longer than a row of the output, which must be bitwise unchanged afterwards; an output that is not
requested (NULL) cannot be written at all.  Each float check prints "MEASURE <what> err=<error> bar=<its bar>" for the element that
takes the largest share of its bar (run with -s to see the figures).

DIST_NT_DEFAULT (non-temporal stores of logits and features) is a compile-time constant of common.h: only the compiled variant of the
C = K = 16 kernels can be tested here.

Measured on the MI355X (the whole file, 65 tests, takes about 4.5 s there; the slowest test, an above-the-cap case, 0.7 s), as the
largest share of its bar, error of bar:
  exact cases (logits, features, argmax, dissum, df, NHWC; every tie)   all equal
  forward logits     C = K = 16  2.7e-5 of 9.0e-5;  <4,16> 2.9e-6 of 4.1e-6 (C = 1);  <4,32> 1.2e-5 of 4.6e-5;  <1,16> 3.0e-6 of 4.4e-6
  forward dissum     C = K = 16  2.3e-4 of 2.2e-3;  the feature copy bit-identical everywhere
  upsampled features staged x4 2.0e-4 of 8.7e-4 (beside the 1e3 pixel);  gathered 6.6e-7 of 3.0e-6;  generic 1.4e-6 of 4.1e-6 (C = 24)
  upsampled logits   staged x4 3.5e-6 of 3.2e-5;  gathered 5.2e-5 of 4.2e-4;  generic 1.7 of 10 (|logit| 1e7);  dissum 0.080 of 0.51
  backward           C = K = 16  3.2e-6 of 1.0e-5;  generic 5.9e-8 of 6.3e-8 (C = 17, K = 1 with gfeats: five roundings, all counted)
  NHWC               5.9e-6 of 3.7e-5 (K = Kp = 32)
  argmax, real data  no pixel with a clear margin differs; near-ties: 1 pixel of 1028 in one case, none elsewhere
  inf / NaN          dml_proto_dist_fwd and dml_proto_dist_nhwc as the definition; the upsampled head non-finite wherever a tap of
                     non-zero weight is, with argmax 0 there, and inside the clean embedding's bars (logits 4.1e-6 of 2.7e-5) away
                     from those taps

Tried on scratch builds of head.hip, one at a time, and caught by this file: `>=` for `>` in the running maximum (32 tests,
the tie cases), the last channel left out of the distance when C % 4 != 0 (8), src_tap without the half-pixel offset (19), gfeats
not added (7), twice the stride in proto_dist_fwd_kernel's loop (the two above-the-cap cases).  No kernel had to be changed.
"""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import head_cases as HC

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 16384                                  # guard elements before and after: more than a row of any output here
KINDS = ("exact", "real")
ESIZE = {"f32": (torch.float32, 4), "u8": (torch.uint8, 1)}


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pkinds(kind):
    return HC.PROTO_KINDS if kind == "exact" else ("real",)


def measure(what, seen):
    for name, (err, bar) in sorted(seen.items()):
        print("MEASURE %s %s err=%.3e bar=%.3e" % (what, name, err, bar))


class Out:
    """GUARD elements, n elements, GUARD elements on the device, every byte 0xAA"""

    def __init__(self, n, dtype="f32", data=None):
        self.n = n
        self.tdt, self.esize = ESIZE[dtype]
        self.raw = torch.full(((2 * GUARD + n) * self.esize,), 0xAA, dtype=torch.uint8, device="cuda")
        self.body = self.raw.view(self.tdt)[GUARD:GUARD + n]
        self.ptr = self.body.data_ptr()
        if data is not None:
            self.body.copy_(dev(data).reshape(-1))

    def get(self, shape):
        return self.body.cpu().numpy().reshape(shape)

    def untouched(self):
        lo, hi = GUARD * self.esize, (GUARD + self.n) * self.esize
        assert bool((self.raw[:lo] == 0xAA).all()) and bool((self.raw[hi:] == 0xAA).all()), "a byte outside the output was written"


def same_bits(a, b):
    return (np.ascontiguousarray(a, F32).view(np.uint32) == np.ascontiguousarray(b, F32).view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------------------------
# dml_proto_dist_fwd
# ---------------------------------------------------------------------------------------------------------------------
def run_fwd(lib, kind, pkind, case, want=(True, True, True, True)):
    """one call with the requested outputs (logits, feats, argmax, dissum) checked against the definition"""
    B, Hh, Ww, C, K = case
    f, P = HC.plain_input(kind, pkind, case)
    exact = kind == "exact"
    ref = HC.head_fwd(f, P, bars=not exact)
    x, Pd = dev(f.transpose(0, 3, 1, 2)), dev(P)
    n = B * Hh * Ww
    bufs = {"logits": Out(n * K), "feats": Out(n * C), "argmax": Out(n, "u8"), "dissum": Out(n)}
    ptr = [bufs[name].ptr if on else None for name, on in zip(("logits", "feats", "argmax", "dissum"), want)]
    chk(lib.dml_proto_dist_fwd(x.data_ptr(), Pd.data_ptr(), ptr[0], ptr[1], ptr[2], ptr[3], B, C, K, Hh, Ww, st()))
    shapes = {"logits": (B, K, Hh, Ww), "feats": (B, Hh, Ww, C), "argmax": (B, Hh, Ww), "dissum": (B, Hh, Ww)}
    got = {name: bufs[name].get(shapes[name]) for name, on in zip(shapes, want) if on}
    what = "fwd %s %s %s %s" % (HC.dispatch("fwd", C, K, Hh, Ww), kind, pkind, case)
    seen = HC.check_head(what, got, ref, f, None, exact)
    if want[1]:
        assert same_bits(got["feats"], f), what + ": the feature copy is not bit-identical"
    if not exact:
        measure(what, seen)
    for b in bufs.values():
        b.untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_forward_c16_group_counts(lib, kind):
    """1, 15 (one wave over three images), 63, 64, 65, 257 and 514 four-pixel groups; ties go to the first prototype"""
    for B, Hh, Ww in HC.C16_SHAPES:
        for pkind in pkinds(kind):
            run_fwd(lib, kind, pkind, (B, Hh, Ww, 16, 16))


def test_forward_c16_every_combination_of_null_outputs(lib):
    for want in HC.NULL_COMBOS:
        for kind, pkind in (("exact", "dup"), ("real", "real")):
            run_fwd(lib, kind, pkind, HC.NULL_SHAPE + (16, 16), want)


@pytest.mark.parametrize("pair", HC.PAIRS + [(16, 16)], ids=lambda p: "C%d-K%d" % p)
def test_forward_generic_kernels(lib, pair):
    """<4, 16>, <4, 32>, <1, 16>, <1, 32>: C % 4 != 0 (the scalar feature stores) with and without feats, K up to 33, H W in {1, 3, 35}"""
    C, K = pair
    for B, Hh, Ww in (HC.PX1_SHAPES if pair == (16, 16) else HC.PX4_SHAPES + HC.PX1_SHAPES):
        for kind in KINDS:
            for pkind in pkinds(kind):
                run_fwd(lib, kind, pkind, (B, Hh, Ww, C, K))
            if C % 4:
                run_fwd(lib, kind, pkinds(kind)[0], (B, Hh, Ww, C, K), (True, False, True, True))


@pytest.mark.parametrize("case", [HC.BIG_PX1, HC.BIG_PX4], ids=["px1", "px4"])
def test_forward_above_the_grid_cap(lib, case):
    """more items than 4096 workgroups of 256: the grid-stride loop takes a second trip"""
    run_fwd(lib, "exact", "eye", case)


# ---------------------------------------------------------------------------------------------------------------------
# dml_upsample_dist_fwd
# ---------------------------------------------------------------------------------------------------------------------
def run_up(lib, kind, pkind, case):
    B, h, w, Hh, Ww, C, K, am, ds = case
    e, P = HC.upsample_input(kind, pkind, case)
    assert kind in HC.upsample_kinds(case)
    exact = kind == "exact"
    f, Df, ref = HC.upsample_head(e, P, Hh, Ww, exact)
    ed, Pd = dev(e), dev(P)
    n = B * Hh * Ww
    bufs = {"logits": Out(n * K), "feats": Out(n * C), "argmax": Out(n, "u8"), "dissum": Out(n)}
    chk(lib.dml_upsample_dist_fwd(ed.data_ptr(), Pd.data_ptr(), bufs["logits"].ptr, bufs["feats"].ptr, bufs["argmax"].ptr if am else None,
                                  bufs["dissum"].ptr if ds else None, B, h, w, C, K, Hh, Ww, st()))
    got = {"logits": bufs["logits"].get((B, K, Hh, Ww)), "feats": bufs["feats"].get((B, Hh, Ww, C))}
    if am:
        got["argmax"] = bufs["argmax"].get((B, Hh, Ww))
    if ds:
        got["dissum"] = bufs["dissum"].get((B, Hh, Ww))
    what = "upsample %s %s %s %s" % (HC.dispatch("up", C, K, Hh, Ww, h, w, am, ds), kind, pkind, case)
    seen = HC.check_head(what, got, ref, f, Df, exact)
    if not exact:
        measure(what, seen)
    for b in bufs.values():
        b.untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_upsample_staged_x4_and_gathered_c16(lib, kind):
    """the staged kernel at 1 x 1, 3 x 5, one whole 256-column segment and a second one of one lane; the gathered one at ratios
    that are not x4 (enlarging, shrinking, identity, x2)"""
    for geom in HC.UP_X4 + HC.UP_C16:
        case = (HC.UP_B,) + geom + (16, 16, False, False)
        for pkind in (pkinds(kind) if kind in HC.upsample_kinds(case) else ()):
            run_up(lib, kind, pkind, case)


@pytest.mark.parametrize("way", HC.UP_PX4_WAYS, ids=lambda v: "C%d-K%d-argmax%d-dissum%d" % v)
def test_upsample_generic_four_pixel_kernel(lib, way):
    """W % 4 == 0 with a real class count, C = 24 and C = 5, or C = K = 16 with a map requested: logits, features, argmax, dissum"""
    for geom in HC.UP_PX4_GEOMS:
        for kind in HC.upsample_kinds((HC.UP_B,) + geom + way):
            for pkind in pkinds(kind):
                run_up(lib, kind, pkind, (HC.UP_B,) + geom + way)


@pytest.mark.parametrize("way", HC.UP_PX1_WAYS, ids=lambda v: "C%d-K%d-argmax%d-dissum%d" % v)
def test_upsample_generic_one_pixel_kernel(lib, way):
    for geom in HC.UP_PX1_GEOMS:
        for kind in HC.upsample_kinds((HC.UP_B,) + geom + way):
            for pkind in pkinds(kind):
                run_up(lib, kind, pkind, (HC.UP_B,) + geom + way)


@pytest.mark.parametrize("case", HC.UP_SPECIAL, ids=lambda c: "%dx%d-%dx%d-C%d-K%d" % c[1:7])
def test_upsample_propagates_inf_and_nan(lib, case):
    """every pixel that interpolates the inf or the NaN with a non-zero weight is non-finite in features, logits and dissum and has
    argmax 0; every
    pixel whose taps and their neighbouring columns are clean is inside the bars of the clean embedding"""
    B, h, w, Hh, Ww, C, K, am, ds = case
    bad, e, P, must, may = HC.upsample_special(case)
    f, Df, ref = HC.upsample_head(e, P, Hh, Ww, False)
    ed, Pd = dev(bad), dev(P)
    n = B * Hh * Ww
    bufs = {"logits": Out(n * K), "feats": Out(n * C), "argmax": Out(n, "u8"), "dissum": Out(n)}
    chk(lib.dml_upsample_dist_fwd(ed.data_ptr(), Pd.data_ptr(), bufs["logits"].ptr, bufs["feats"].ptr, bufs["argmax"].ptr if am else None,
                                  bufs["dissum"].ptr if ds else None, B, h, w, C, K, Hh, Ww, st()))
    got = {"logits": bufs["logits"].get((B, K, Hh, Ww)), "feats": bufs["feats"].get((B, Hh, Ww, C)),
           "dissum": bufs["dissum"].get((B, Hh, Ww)) if ds else None, "argmax": bufs["argmax"].get((B, Hh, Ww)) if am else None}
    what = "upsample %s inf / NaN %s" % (HC.dispatch("up", C, K, Hh, Ww, h, w, am, ds), case)
    measure(what, HC.check_propagation(what, got, ref, f, Df, must, may))
    for b in bufs.values():
        b.untouched()


@pytest.mark.parametrize("case", [HC.UP_BIG_PX1, HC.UP_BIG_PX4], ids=["px1", "px4"])
def test_upsample_above_the_grid_cap(lib, case):
    run_up(lib, "exact", "eye", case + (True, True))


# ---------------------------------------------------------------------------------------------------------------------
# dml_proto_dist_bwd
# ---------------------------------------------------------------------------------------------------------------------
def run_bwd(lib, kind, pkind, case):
    B, Hh, Ww, C, K = case
    P = HC.protos(pkind, K, C)
    g, f, gf = HC.gradients(kind, B, K, Hh, Ww, C, P)
    gd, fd, gfd, Pd = dev(g), dev(f), dev(gf), dev(P)
    exact = kind == "exact"
    for gfeats in (None, gf):
        df, bar = HC.head_bwd(g, f, P, gfeats, bars=not exact)
        out = Out(B * Hh * Ww * C)
        chk(lib.dml_proto_dist_bwd(gd.data_ptr(), None if gfeats is None else gfd.data_ptr(), fd.data_ptr(), Pd.data_ptr(), out.ptr,
                                   B, C, K, Hh, Ww, st()))
        what = "bwd %s %s %s %s gfeats=%d" % (HC.dispatch("bwd", C, K, Hh, Ww), kind, pkind, case, gfeats is not None)
        seen = HC.check_close(what, out.get(df.shape), df, bar, exact)
        if not exact:
            measure(what, {"df": seen})
        out.untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_backward_c16_group_counts(lib, kind):
    for B, Hh, Ww in HC.C16_SHAPES:
        for pkind in pkinds(kind):
            run_bwd(lib, kind, pkind, (B, Hh, Ww, 16, 16))


@pytest.mark.parametrize("pair", HC.PAIRS + [(16, 16)], ids=lambda p: "C%d-K%d" % p)
def test_backward_generic_kernels(lib, pair):
    """with and without gfeats; a pixel whose g_k are all zero; a channel where gs f and gm cancel (the bar is absolute)"""
    C, K = pair
    for B, Hh, Ww in (HC.PX1_SHAPES if pair == (16, 16) else HC.PX4_SHAPES + HC.PX1_SHAPES):
        for kind in KINDS:
            for pkind in pkinds(kind):
                run_bwd(lib, kind, pkind, (B, Hh, Ww, C, K))


@pytest.mark.parametrize("case", [HC.BIG_PX1, HC.BIG_PX4], ids=["px1", "px4"])
def test_backward_above_the_grid_cap(lib, case):
    run_bwd(lib, "exact", "int", case)


# ---------------------------------------------------------------------------------------------------------------------
# dml_proto_dist_nhwc
# ---------------------------------------------------------------------------------------------------------------------
def run_nhwc(lib, kind, pkind, M, K, Kp, lde, ldo):
    e, P = HC.nhwc_inputs(kind, M, K, Kp, pkind)
    ref, bar = HC.nhwc_dist(e, P, K, bars=kind != "exact")
    ew = np.full((M, lde), np.nan, F32)                                         # columns Kp .. lde - 1 are never read: NaN would show
    ew[:, :Kp] = e
    ed, Pd, out = dev(ew), dev(P), Out(M * ldo)
    chk(lib.dml_proto_dist_nhwc(ed.data_ptr(), Pd.data_ptr(), out.ptr, M, K, Kp, lde, ldo, st()))
    got = out.get((M, ldo))
    what = "nhwc %s %s M=%d K=%d Kp=%d lde=%d ldo=%d" % (kind, pkind, M, K, Kp, lde, ldo)
    seen = HC.check_close(what, got[:, :K], ref[:, :K], None if bar is None else bar[:, :K], kind == "exact")
    assert same_bits(got[:, K:Kp], np.zeros((M, Kp - K), F32)), what + ": the pad columns are not +0.0"
    assert (np.ascontiguousarray(got[:, Kp:]).view(np.uint32) == 0xAAAAAAAA).all(), what + ": a column beyond Kp was written"
    if kind != "exact":
        measure(what, {"out": seen})
    out.untouched()


@pytest.mark.parametrize("kkp", HC.NHWC_KKP + [HC.NHWC_BIG[1:]], ids=lambda v: "K%d-Kp%d" % v)
def test_nhwc_low_resolution_distance(lib, kkp):
    """M around a workgroup, dense and with lde / ldo above Kp: pad columns exactly 0, columns beyond Kp untouched"""
    K, Kp = kkp
    for M in HC.NHWC_M:
        for lde, ldo in HC.nhwc_pitches(Kp):
            for kind in KINDS:
                for pkind in pkinds(kind):
                    run_nhwc(lib, kind, pkind, M, K, Kp, lde, ldo)


def test_nhwc_above_the_grid_cap(lib):
    M, K, Kp = HC.NHWC_BIG
    for lde, ldo in HC.nhwc_pitches(Kp):
        run_nhwc(lib, "exact", "int", M, K, Kp, lde, ldo)
