"""GPU: the BatchNorm kernels of csrc/bn.hip at their edges, through the C ABI -- statistics, the one-stage and the folded finalize,
the column-stationary and the planes-only apply (forward and backward), the backward reduce / fold / finalize, the synchronised
pieces, the plane-scale bound kernels and the bound fused into the finalize launches.

Every comparison is against the float64 definitions of tests/bn_cases.py on the same float32 / bfloat16 inputs (proved right on these
inputs, without a GPU, by tests/test_bn_refs.py).  Exact (dyadic) inputs must be reproduced EXACTLY -- values with ==, mask bytes
and fp16 planes bit for bit -- at every geometry the host dispatch distinguishes; real-valued inputs against bars that count the
float32 roundings of the contract.  Every output buffer is longer and wider than needed and pre-filled with a sentinel (NaN, 0xAA
bytes for masks and planes) that must survive outside the addressed rows x channels.  Each float check prints
"MEASURE <what> err=<largest error> bar=<bar>" before it asserts (run with -s to see the figures).

Largest share of its bar measured on the MI355X, as error of bar (the whole file, 73 tests, takes about 3 s there; the slowest
test 0.5 s):
  exact cases (apply, planes, masks, dropout, reduce, backward apply, sums, amax / gmax words)   all equal: 0 of 0
  apply z, f32             3.1e-7  of 6.6e-7   (297 x 48 with residual; dropout 6.2e-7 of 1.6e-6)
  apply z, bf16            7.8e-3  of 7.8e-3   (a tie of the bfloat16 store: half an ulp of its binade is reached, never passed)
  apply amax               2.7e-7  of 1.2e-6
  mask elements left out   0 of 14 256 and 0 of 512, in every case (cap: 1 in 10 000)
  reduce sum g             2.4e-7  of 6.0e-7   (2 x 256);  sum g xhat 5.3e-7 of 1.7e-6
  backward apply dy, f32   2.9e-8  of 1.4e-7;  dres 1.2e-7 of 2.4e-7;  bf16: ties of the store, as above
  dml_bn_stats             sum 1.1e-4 of 1.0e-3 (449 rows, std = 1e3);  M2 3.8e-5 of 1.4e-4 (bf16, 64 rows)
  finalize                 mean 98 %, invstd 97 %, scale 87 % of the one / two final roundings; running mean 43 %, running var 44 %
  backward finalize coef   1.1e-10 of 1.2e-10  (one rounding; dgamma / dbeta equal)
  synchronised forward     moments 3 %, merged statistics 2-3 % of the bars of the float32 partials they are merged from
  synchronised backward    sums equal; coef 6.5e-9 of 7.9e-9
  eval coefficients        1.1e-7  of 1.9e-7
  plane scales             every work[1024] equal to the scale of the float64 bound
  reaching the bound       planes finite, max |z| / un in [2^14, 2^15) at M = 297; hi + lo against z 1.9e-6 of 1.2e-5, dy 7.5e-9 of 5.0e-8

Not as the issue words it, on purpose: N = 264 sits at plane offset 40 of pitch 304 (offset 256 + 264 channels would run into the next
row; the 48 channels of the fall-back case sit at offset 256); the bfloat16 store is given half an ulp of the value's binade
(between 2^-9 and 2^-8 of it) -- 2^-9 |ref| is less than round-to-nearest itself can promise.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import bn_cases as CS

pytestmark = pytest.mark.gpu

EINVAL, EALIGN = -1, -2
F32, F64 = np.float32, np.float64
DT = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (None, torch.float16), "u8": (None, torch.uint8)}
UN = 2.0 ** -9                                 # plane scale of the exact cases: |z| < 64 lands below 2^15
RES_UN = 2.0 ** -11                            # scale of a residual given as planes: (hi + lo) * RES_UN is the residual, exactly


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_le(what, err, bar):
    err, bar = np.asarray(err, F64), np.asarray(bar, F64) * np.ones_like(np.asarray(err, F64))
    assert np.isfinite(err).all(), "%s: non-finite error" % what
    k = int(np.argmax(np.where(err > bar, np.inf, err / np.maximum(bar, 1e-300)))) if err.size else 0      # the worst share of its bar
    print("MEASURE %s err=%.3e bar=%.3e" % (what, err.flat[k] if err.size else 0.0, bar.flat[k] if err.size else 0.0))
    assert (err <= bar).all(), "%s: error %.3e above the bar %.3e" % (what, err.flat[k], bar.flat[k])


class Buf:
    """[planes][1 + M + 1 rows][ld] on the device, filled with a sentinel (NaN; 0xAA bytes for fp16 planes and mask bytes), the
    addressed M x N region at row 1, column `off`; `lead` shifts the whole thing by that many elements (alignment cases)"""

    def __init__(self, M, N, ld=None, off=0, dtype="f32", data=None, planes=1, lead=0):
        self.M, self.N, self.ld, self.off, self.kind = M, N, ld or N, off, dtype
        assert off + N <= self.ld and M >= 1
        tdt = DT[dtype][1]
        self.lead = lead
        self.raw = torch.empty(lead + planes * (M + 2) * self.ld, dtype=tdt, device="cuda")
        if dtype in ("f16", "u8"):
            self.raw.view(torch.uint8).fill_(0xAA)
        else:
            self.raw.fill_(float("nan"))
        self.t = self.raw[lead:].view(planes, M + 2, self.ld)
        if data is not None:
            src = torch.from_numpy(np.ascontiguousarray(data))
            self.t[:, 1:M + 1, off:off + N] = (src if dtype in ("f16", "u8") else src.float()).to(tdt).cuda().view(-1, M, N)
        self.ptr = self.t.data_ptr() + (self.ld + off) * self.raw.element_size()
        self.plane_stride = (M + 2) * self.ld

    def get(self):
        r = self.t[:, 1:self.M + 1, self.off:self.off + self.N]
        r = r.cpu() if self.kind in ("f16", "u8") else r.float().cpu()
        r = r.numpy()
        return r[0] if r.shape[0] == 1 else r

    def assert_untouched_outside(self):
        c = self.raw.clone()
        if self.kind in ("f16", "u8"):
            v = c[self.lead:].view(self.t.shape)
            v[:, 1:self.M + 1, self.off:self.off + self.N] = v[:, 0:1, 0:1].expand(v.shape[0], self.M, self.N)
            assert bool((c.view(torch.uint8) == 0xAA).all()), "a byte outside the addressed region was written"
        else:
            c[self.lead:].view(self.t.shape)[:, 1:self.M + 1, self.off:self.off + self.N] = float("nan")
            assert bool(torch.isnan(c).all()), "an element outside the addressed region was written"


def vecbuf(n, data=None, tail=5):
    """per-channel float32 array with a NaN tail"""
    t = torch.full((n + tail,), float("nan"), device="cuda")
    if data is not None:
        t[:n] = dev(np.asarray(data, F32))
    return t


def tail_ok(t, n):
    return bool(torch.isnan(t[n:]).all())


def f16bits(a):
    return np.ascontiguousarray(a).view(np.int16)


# ---------------------------------------------------------------------------------------------------------------------
# forward apply
# ---------------------------------------------------------------------------------------------------------------------
def apply(lib, dtype, d, M, N, *, res, relu, side, want_z=True, py=None, pres=None, pz=None, planes=None, res_planes=False,
          drop=0.0, seed=0):
    """one dml_bn_apply launch on the inputs d (exact or real); returns the outputs as numpy.  py / pres / pz: (pitch, offset) of y,
    res, z; planes: None or (ldp, off, lead elements); side: mask and amax on."""
    V = CS.vec(dtype)
    dt = DT[dtype][0]
    py, pres, pz = py or (N, 0), pres or (N, 0), pz or (N, 0)
    yb = Buf(M, N, py[0], py[1], dtype, d["y"])
    rb = None
    rps, run = 0, None
    if res and res_planes:
        hi, lo = CS.h2_planes(d["res"].astype(F32), RES_UN)
        assert ((hi.astype(F64) + lo.astype(F64)) * RES_UN == d["res"]).all()
        rb = Buf(M, N, pres[0], pres[1], "f16", np.stack([hi, lo]), planes=2)
        rps = rb.plane_stride
        run = dev(np.array([RES_UN], F32))
    elif res:
        rb = Buf(M, N, pres[0], pres[1], dtype, d["res"])
    zb = Buf(M, N, pz[0], pz[1], dtype) if want_z else None
    mk = Buf(M, N // V, dtype="u8") if side else None
    amax = torch.zeros(1024 + 3, device="cuda") if side else None
    pb, unscale = None, None
    if planes is not None:
        pb = Buf(M, N, planes[0], planes[1], "f16", planes=2, lead=planes[2])
        unscale = dev(np.array([UN], F32))
    sc, sh, mu = (vecbuf(N, d[k]) for k in ("scale", "shift", "mean"))
    rc = lib.dml_bn_apply(yb.ptr, rb.ptr if rb else None, zb.ptr if zb else None, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                          mk.ptr if mk else None, M, N, py[0], pres[0], pz[0], relu, dt, drop, seed,
                          amax.data_ptr() if side else None, pb.ptr if pb else None, pb.plane_stride if pb else 0,
                          planes[0] if pb else 0, unscale.data_ptr() if pb else None, rps, run.data_ptr() if run is not None else None, st())
    chk(rc)
    torch.cuda.synchronize()
    out = {}
    for name, b in (("z", zb), ("mask", mk), ("planes", pb)):
        if b is not None:
            b.assert_untouched_outside()
            out[name] = b.get()
    if side:
        assert bool((amax[1024:] == 0).all())
        out["amax"] = float(amax.max().item())
    return out


def check_apply_exact(lib, dtype, d, M, N, res, relu, side, **kw):
    V = CS.vec(dtype)
    z, _ = CS.fwd_ref(d["y"], d["res"] if res else None, d["mean"], d["scale"], d["shift"], relu)
    zs = CS.store(z, dtype)
    out = apply(lib, dtype, d, M, N, res=res, relu=relu, side=side, **kw)
    if "z" in out:
        assert (out["z"] == zs).all(), "z differs from the exact value at %d elements" % int((out["z"] != zs).sum())
    if side:
        assert (out["mask"] == CS.pack_mask(z > 0, V)).all(), "mask bits"
        assert out["amax"] == np.abs(z).max(), "amax %r against max |z| %r" % (out["amax"], np.abs(z).max())
    if "planes" in out:
        hi, lo = CS.h2_planes(z.astype(F32), UN)
        assert (f16bits(out["planes"][0]) == f16bits(hi)).all(), "hi plane"
        assert (f16bits(out["planes"][1]) == f16bits(lo)).all(), "lo plane"
    return out


COMBOS = [(res, relu, side) for res in (0, 1) for relu in (0, 1) for side in (0, 1)]


@pytest.mark.parametrize("N,M", CS.apply_shapes("f32"))
def test_apply_exact_f32(lib, N, M):
    d = CS.exact_inputs(M, N)
    for res, relu, side in COMBOS:
        check_apply_exact(lib, "f32", d, M, N, res, relu, side)


@pytest.mark.parametrize("N,M", CS.apply_shapes("bf16"))
def test_apply_exact_bf16(lib, N, M):
    d = CS.exact_inputs(M, N)
    for res, relu, side in COMBOS:
        check_apply_exact(lib, "bf16", d, M, N, res, relu, side)


@pytest.mark.parametrize("dtype,case", [(dt, c) for dt in ("f32", "bf16") for c in CS.SLICES[dt]])
def test_apply_exact_in_channel_slices(lib, dtype, case):
    """y, res and z each in a slice of its own pitch: the ASPP branches (256 of 1280) and the decoder concat (48 of 304)"""
    N, M, pz = case
    py, pres = CS.slice_pitches(N, CS.vec(dtype))
    d = CS.exact_inputs(M, N)
    for res, relu, side in COMBOS:
        check_apply_exact(lib, dtype, d, M, N, res, relu, side, py=py, pres=pres, pz=pz)


@pytest.mark.parametrize("N,M", CS.PLANES_SHAPES)
def test_apply_planes_only_exact(lib, N, M):
    """z == NULL: the eight-channel kernel (N % 8 == 0, 16-byte aligned planes) or its fall-back to the four-channel one (N = 12;
    N = 48 with the planes 8- but not 16-byte aligned); the residual as fp32 and as planes of its own pitch"""
    d = CS.exact_inputs(M, N, fine_res=True)
    pl = {264: (304, 40, 0), 48: (304, 256, 4)}.get(N, (N, 0, 0))      # (pitch, channel offset, halves the pointer is shifted by)
    py = (N + 12, 8) if N == 264 else (N, 0)
    for relu in (0, 1):
        for res, rp in ((0, False), (1, False), (1, True)):
            pres = (N + 8, 8) if rp else (N + 4, 0)
            o = check_apply_exact(lib, "f32", d, M, N, res, relu, 1, want_z=False, py=py, pres=pres, planes=pl, res_planes=rp)
            assert "z" not in o
    # and beside z (the four-channel kernel writes both)
    o = check_apply_exact(lib, "f32", d, M, N, 1, 1, 1, planes=pl, py=py)
    assert (f16bits(o["planes"][1]) != 0).any()               # the lo plane carries something


def test_apply_dropout_pattern_follows_the_logical_index(lib):
    """p = 0.5 (keep scale 2, exact): the hash is indexed by m N + c, so the kept pattern does not depend on the pitches; kept values
    are exactly 2 z and the mask bit is that of the dropped value"""
    N, M = 48, 297
    d = CS.exact_inputs(M, N)
    z, _ = CS.fwd_ref(d["y"], d["res"], d["mean"], d["scale"], d["shift"], 1)
    for dtype in ("f32", "bf16"):
        a = apply(lib, dtype, d, M, N, res=1, relu=1, side=1, drop=0.5, seed=1234)
        py, pres = CS.slice_pitches(N, CS.vec(dtype))
        b = apply(lib, dtype, d, M, N, res=1, relu=1, side=1, drop=0.5, seed=1234, py=py, pres=pres, pz=(304, 256))
        assert (a["z"] == b["z"]).all() and (a["mask"] == b["mask"]).all() and a["amax"] == b["amax"]
        kept = a["z"] != 0
        assert (a["z"][kept] == 2 * z[kept]).all() and (z[~kept & (z != 0)] != 0).all()
        assert (a["mask"] == CS.pack_mask(a["z"] > 0, CS.vec(dtype))).all()
        assert a["amax"] == np.abs(a["z"]).max()
        n = int((z != 0).sum())
        frac = kept.sum() / n
        print("MEASURE dropout kept share %s err=%.3e bar=%.3e" % (dtype, abs(frac - 0.5), 3.0 / np.sqrt(n)))
        assert abs(frac - 0.5) <= 3.0 / np.sqrt(n)               # six standard deviations of a fair coin
        c = apply(lib, dtype, d, M, N, res=1, relu=1, side=0, drop=0.5, seed=99)
        assert ((c["z"] != 0) != kept).any()                         # another seed, another pattern


# ---------------------------------------------------------------------------------------------------------------------
# backward reduce
# ---------------------------------------------------------------------------------------------------------------------
def reduce(lib, dtype, d, M, N, *, relu, how, z=None, on=None, pitches=None, gscale=CS.GSCALE):
    """one dml_bn_bwd_reduce launch; how: "mask" | "z" | None; returns (partials[nblocks, N, 2] float64, nblocks, gmax)"""
    V = CS.vec(dtype)
    pdz, py, pz = pitches or ((N, 0), (N, 0), (N, 0))
    dzb, yb = Buf(M, N, pdz[0], pdz[1], dtype, d["dz"]), Buf(M, N, py[0], py[1], dtype, d["y"])
    zb = Buf(M, N, pz[0], pz[1], dtype, z) if how == "z" else None
    mk = Buf(M, N // V, dtype="u8", data=CS.pack_mask(on, V)) if how == "mask" else None
    mu, inv = vecbuf(N, d["mean"]), vecbuf(N, d["invstd"])
    rows = 1100
    part = torch.full((rows, N, 2), float("nan"), device="cuda")
    gmax = torch.zeros(1024 + 3, device="cuda")
    nb = C.c_int(-1)
    chk(lib.dml_bn_bwd_reduce(dzb.ptr, yb.ptr, zb.ptr if zb else None, mk.ptr if mk else None, mu.data_ptr(), inv.data_ptr(),
                              part.data_ptr(), M, N, pdz[0], py[0], pz[0], relu, gscale, DT[dtype][0], C.byref(nb),
                              gmax.data_ptr(), st()))
    torch.cuda.synchronize()
    nb = nb.value
    assert 1 <= nb <= rows and bool(torch.isnan(part[nb:]).all()), "rows from nblocks on were written"
    assert bool((gmax[1024:] == 0).all())
    return part[:nb].cpu().numpy().astype(F64), nb, float(gmax.max().item())


def check_reduce_exact(lib, dtype, N, M, pitches=None):
    d = CS.exact_inputs(M, N)
    z, _ = CS.fwd_ref(d["y"], d["res"], d["mean"], d["scale"], d["shift"], 1)
    on = z > 0
    got = {}
    for relu, how in ((1, "mask"), (1, "z"), (0, None)):
        g = CS.bwd_g(d["dz"], on if relu else None, CS.GSCALE)
        ref = CS.bwd_sums(g, d["y"], d["mean"], d["invstd"])
        part, nb, gmax = reduce(lib, dtype, d, M, N, relu=relu, how=how, z=CS.store(z, dtype), on=on, pitches=pitches)
        assert nb >= -(-M // CS.RED_MAX_ROWS)
        assert np.isfinite(part).all()
        s = part.sum(0).T
        assert (s == ref).all(), "sums over the %d partial rows (%s) differ at %d channels" % (nb, how, int((s != ref).any(0).sum()))
        assert gmax == np.abs(g).max()
        got[how] = part
    assert (got["mask"] == got["z"]).all()                         # ReLU from the mask and from z: the same partials


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bwd_reduce_exact(lib, dtype):
    for N, M in CS.reduce_shapes(dtype):
        check_reduce_exact(lib, dtype, N, M)
    V = CS.vec(dtype)
    for N, M, pz in CS.SLICES[dtype]:
        check_reduce_exact(lib, dtype, N, M, pitches=((N + V, V), (N + 3 * V, 2 * V), pz))


# ---------------------------------------------------------------------------------------------------------------------
# backward apply
# ---------------------------------------------------------------------------------------------------------------------
def bwd_apply(lib, dtype, d, M, N, *, relu, how, z=None, on=None, dres=None, want_dy=True, planes=None, side=False, sliced=False,
              gscale=CS.GSCALE):
    """one dml_bn_bwd_apply launch; dres: None | "set" | "accum"; planes: None or (ldp, off, lead); sliced: dz, y, dy (and dres)
    in slices of their own pitch"""
    V = CS.vec(dtype)
    pdz, py, pdy, pdr = ((N + V, V), (N + 3 * V, 2 * V), (304 if N <= 296 else N + 4 * V, 8), (N + 2 * V, V)) if sliced else ((N, 0),) * 4
    if dres == "accum":
        pdr = (N + 2 * V, V)                                        # always into a slice of another pitch
    dzb, yb = Buf(M, N, pdz[0], pdz[1], dtype, d["dz"]), Buf(M, N, py[0], py[1], dtype, d["y"])
    zb = Buf(M, N, dtype=dtype, data=z) if how == "z" else None
    mk = Buf(M, N // V, dtype="u8", data=CS.pack_mask(on, V)) if how == "mask" else None
    dyb = Buf(M, N, pdy[0], pdy[1], dtype) if want_dy else None
    drb = Buf(M, N, pdr[0], pdr[1], dtype, d["dres0"] if dres == "accum" else None) if dres else None
    coef = vecbuf(4 * N, np.asarray(d["coef"], F32).reshape(-1))
    amax = torch.zeros(1024 + 3, device="cuda") if side else None
    pb, unscale = None, None
    if planes is not None:
        pb = Buf(M, N, planes[0], planes[1], "f16", planes=2, lead=planes[2])
        unscale = dev(np.array([UN], F32))
    chk(lib.dml_bn_bwd_apply(dzb.ptr, yb.ptr, zb.ptr if zb else None, mk.ptr if mk else None, coef.data_ptr(),
                             dyb.ptr if dyb else None, drb.ptr if drb else None, M, N, pdz[0], py[0], N, pdy[0], pdr[0] if drb else 0,
                             relu, gscale, 1 if dres == "accum" else 0, DT[dtype][0], amax.data_ptr() if side else None,
                             pb.ptr if pb else None, pb.plane_stride if pb else 0, planes[0] if pb else 0,
                             unscale.data_ptr() if pb else None, st()))
    torch.cuda.synchronize()
    out = {}
    for name, b in (("dy", dyb), ("dres", drb), ("planes", pb)):
        if b is not None:
            b.assert_untouched_outside()
            out[name] = b.get()
    if side:
        out["amax"] = float(amax.max().item())
    return out


def check_bwd_apply_exact(lib, dtype, d, M, N, *, relu, how, dres, **kw):
    z, _ = CS.fwd_ref(d["y"], d["res"], d["mean"], d["scale"], d["shift"], 1)
    on = z > 0
    g = CS.bwd_g(d["dz"], on if relu else None, CS.GSCALE)
    dy = CS.bwd_apply_ref(g, d["y"], d["coef"])
    out = bwd_apply(lib, dtype, d, M, N, relu=relu, how=how, z=CS.store(z, dtype), on=on, dres=dres, **kw)
    if "dy" in out:
        assert (out["dy"] == CS.store(dy, dtype)).all(), "dy differs at %d elements" % int((out["dy"] != CS.store(dy, dtype)).sum())
    if dres:
        want = g + (d["dres0"] if dres == "accum" else 0.0)
        assert (out["dres"] == CS.store(want, dtype)).all(), "dres (%s)" % dres
    if "amax" in out:
        assert out["amax"] == np.abs(dy.astype(F32)).max()
    if "planes" in out:
        hi, lo = CS.h2_planes(dy.astype(F32), UN)
        assert (f16bits(out["planes"][0]) == f16bits(hi)).all() and (f16bits(out["planes"][1]) == f16bits(lo)).all(), "dy planes"
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bwd_apply_exact_four_channel_kernel(lib, dtype):
    V = CS.vec(dtype)
    for N, M in CS.BWD_APPLY_SHAPES:
        if N % V:
            continue
        d = CS.exact_inputs(M, N)
        for relu, how in ((1, "mask"), (1, "z"), (0, None)):
            for dres in (None, "set", "accum"):
                check_bwd_apply_exact(lib, dtype, d, M, N, relu=relu, how=how, dres=dres, side=(dres == "set"),
                                      sliced=(dres != "set"))


@pytest.mark.parametrize("N,M", [(n, m) for n, m in CS.BWD_APPLY_SHAPES if n % 8 == 0])
def test_bwd_apply_exact_planes_only(lib, N, M):
    """dy == NULL: the eight-channel kernel, and its fall-backs (an amax pointer; planes 8- but not 16-byte aligned), which must write
    the same planes"""
    d = CS.exact_inputs(M, N)
    pl = (304, 256, 0) if N <= 48 else (N + 8, 8, 0)
    for relu, how in ((1, "mask"), (0, None)):
        for dres in (None, "set", "accum"):
            o = check_bwd_apply_exact(lib, "f32", d, M, N, relu=relu, how=how, dres=dres, want_dy=False, planes=pl, sliced=True)
            assert "dy" not in o
    o = check_bwd_apply_exact(lib, "f32", d, M, N, relu=1, how="mask", dres="set", want_dy=False, planes=pl, side=True)
    assert (f16bits(o["planes"][1]) != 0).any()
    check_bwd_apply_exact(lib, "f32", d, M, N, relu=1, how="mask", dres="accum", want_dy=False, planes=(pl[0] + 4, pl[1], 4))
    check_bwd_apply_exact(lib, "f32", d, M, N, relu=1, how="z", dres=None, want_dy=True, planes=pl, side=True)


# ---------------------------------------------------------------------------------------------------------------------
# rounding, real-valued inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,N", CS.REAL_SHAPES)
def test_rounding_on_real_valued_inputs(lib, M, N, dtype):
    """forward apply, reduce and backward apply against the derived bars: 4 eps32 on the magnitudes of the terms (5 under dropout),
    half a bfloat16 ulp for bf16 storage, (n + 3) eps32 sum |term| for the sums with n the rows of one partial"""
    d = CS.real_case(M, N, dtype)
    V = CS.vec(dtype)
    tag = "%s %dx%d" % (dtype, M, N)
    for res in (0, 1):
        r = d["res"] if res else None
        z, pre = CS.fwd_ref(d["y"], r, d["mean"], d["scale"], d["shift"], 1)
        bar = CS.apply_bar(d["y"], r, d["mean"], d["scale"], d["shift"], dtype)
        o = apply(lib, dtype, d, M, N, res=res, relu=1, side=1)
        check_le("apply z %s res=%d" % (tag, res), np.abs(o["z"].astype(F64) - z), CS.stored_bar(bar, z, dtype))
        decided = np.abs(pre) > bar
        assert (~decided).sum() <= CS.EXCLUDE_CAP * M * N
        assert (CS.unpack_mask(o["mask"], V) == (pre > 0))[decided].all(), "mask bits"
        check_le("apply amax %s res=%d" % (tag, res), abs(o["amax"] - np.abs(z).max()), np.max(bar))
        print("MEASURE mask elements left out %s res=%d err=%d bar=%d" % (tag, res, (~decided).sum(), int(CS.EXCLUDE_CAP * M * N)))
    # dropout: one more rounding
    keep_src = apply(lib, dtype, d, M, N, res=1, relu=1, side=0, drop=0.5, seed=7)["z"]
    kept = keep_src != 0
    bar5 = 2 * CS.apply_bar(d["y"], d["res"], d["mean"], d["scale"], d["shift"], dtype, dropout=True)
    check_le("apply dropout %s" % tag, np.abs(keep_src.astype(F64) - 2 * z)[kept], CS.stored_bar(bar5, 2 * z, dtype)[kept])
    # backward, from the reference's own mask / z (no decision left to the kernel)
    on = z > 0
    g = CS.bwd_g(d["dz"], on, CS.GSCALE)
    ref = CS.bwd_sums(g, d["y"], d["mean"], d["invstd"])
    for how in ("mask", "z"):
        part, nb, gmax = reduce(lib, dtype, d, M, N, relu=1, how=how, z=CS.store(z, dtype) if dtype == "f32" else np.where(on, 1.0, 0.0),
                                on=on)
        bars = CS.reduce_bars(g, d["y"], d["mean"], d["invstd"], CS.partial_rows_bound(M, nb))
        s = part.sum(0).T
        check_le("reduce sum g %s (%s)" % (tag, how), np.abs(s[0] - ref[0]), bars[0])
        check_le("reduce sum g xhat %s (%s)" % (tag, how), np.abs(s[1] - ref[1]), bars[1])
        check_le("reduce gmax %s" % tag, abs(gmax - np.abs(g).max()), CS.EPS32 * np.abs(g).max())
    coef = CS.bwd_coef(ref, d["gamma"], d["mean"], d["invstd"], M).astype(F32)
    d2 = dict(d, coef=coef, dres0=d["res"])
    dy = CS.bwd_apply_ref(g, d["y"], coef)
    bar = CS.bwd_apply_bar(g, d["y"], coef, CS.GSCALE)
    o = bwd_apply(lib, dtype, d2, M, N, relu=1, how="mask", on=on, dres="accum", side=True)
    check_le("bwd apply dy %s" % tag, np.abs(o["dy"].astype(F64) - dy), CS.stored_bar(bar, dy, dtype))
    dr = g + d["res"].astype(F64)
    check_le("bwd apply dres %s" % tag, np.abs(o["dres"].astype(F64) - dr),
             CS.stored_bar(2 * CS.EPS32 * (np.abs(g) + np.abs(d["res"].astype(F64))), dr, dtype))
    check_le("bwd apply amax %s" % tag, abs(o["amax"] - np.abs(dy).max()), np.max(bar))


# ---------------------------------------------------------------------------------------------------------------------
# dml_bn_stats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M", CS.STATS_MS)
def test_stats_partials(lib, M, dtype):
    for N in CS.STATS_NS:
        y = CS.stats_inputs(M, N, dtype)
        yb = Buf(M, N, N + 16, 8, dtype, y)
        G = -(-M // CS.STAT_ROWS)
        part = torch.full((G + 2, N, 2), float("nan"), device="cuda")
        chk(lib.dml_bn_stats(yb.ptr, part.data_ptr(), M, N, N + 16, DT[dtype][0], st()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(part[G:]).all())
        got = part[:G].cpu().numpy().astype(F64)
        ref = CS.partials(y, CS.STAT_ROWS)
        sb, mb = CS.stats_bars(y)
        check_le("stats sum %s M=%d N=%d" % (dtype, M, N), np.abs(got[:, :, 0] - ref[:, :, 0]), sb)
        check_le("stats M2 %s M=%d N=%d" % (dtype, M, N), np.abs(got[:, :, 1] - ref[:, :, 1]), mb)
        if M % CS.STAT_ROWS == 1:
            assert (got[-1, :, 1] == 0).all() and (got[-1, :, 0] == y[-1]).all()      # a last group of one row


# ---------------------------------------------------------------------------------------------------------------------
# finalize from hand-built partials
# ---------------------------------------------------------------------------------------------------------------------
def finalize(lib, part, M, N, sr, prm, mom, null="none", fused=None):
    """dml_bn_finalize (fused: dml_bn_finalize_bound with (count, mult, res_words, work, state)) on a copy of part"""
    pd = dev(part)
    gamma = None if null == "gamma" else vecbuf(N, prm["gamma"])
    beta = None if null == "beta" else vecbuf(N, prm["beta"])
    rm = None if null == "running" else vecbuf(N, prm["rm"])
    rv = None if null == "running" else vecbuf(N, prm["rv"])
    sc, sh, mu = vecbuf(N), vecbuf(N), vecbuf(N)
    inv = None if null == "save_invstd" else vecbuf(N)
    p = lambda t: None if t is None else t.data_ptr()
    args = (pd.data_ptr(), M, N, sr, p(gamma), p(beta), p(rm), p(rv), mom, CS.BN_EPS, p(sc), p(sh), p(mu), p(inv))
    if fused is None:
        chk(lib.dml_bn_finalize(*args, st()))
    else:
        count, mult, resw, work, state = fused
        chk(lib.dml_bn_finalize_bound(*args, count, mult, p(resw), work.data_ptr(), state.data_ptr(), st()))
    torch.cuda.synchronize()
    out = {"scale": sc, "shift": sh, "mean": mu, "invstd": inv, "running_mean": rm, "running_var": rv}
    for k, t in out.items():
        if t is not None:
            assert tail_ok(t, N), k
    return {k: t[:N].cpu().numpy().astype(F64) for k, t in out.items() if t is not None}


def check_finalize(got, ref, bars, what):
    for k in ("mean", "invstd", "scale", "running_mean", "running_var"):
        if k in got and k in ref:
            check_le("finalize %s %s" % (k, what), np.abs(got[k] - ref[k]), bars[k])
    assert (got["shift"] == ref["shift"]).all()


@pytest.mark.parametrize("G", CS.FIN_GS)
def test_finalize_from_hand_built_partials(lib, G):
    """the merge only: Chan's pairwise merge in float64 of the same float32 partials is the reference; bars = the final float32
    roundings plus the float64 cancellation of Q + P - S^2 / M"""
    for sr, N, ragged, mom, null in CS.fin_combos(G):
        part, rows, M = CS.hand_partials(G, N, sr, ragged)
        prm = CS.fin_params(N)
        cnt, mean, m2 = CS.chan_merge(part, rows)
        ref = CS.finalize_ref(M, mean, m2, None if null == "gamma" else prm["gamma"], None if null == "beta" else prm["beta"],
                              None if null == "running" else prm["rm"], None if null == "running" else prm["rv"], mom)
        got = finalize(lib, part, M, N, sr, prm, mom, null)
        what = "G=%d N=%d rows=%d last=%d mom=%g null=%s" % (G, N, sr, rows[-1], mom, null)
        check_finalize(got, ref, CS.finalize_bars(ref), what)
        if M == 1:
            assert (got["mean"] == part[0, :, 0]).all()
            if "invstd" in got:
                assert (got["invstd"] == F64(F32(1.0 / np.sqrt(F64(F32(CS.BN_EPS)))))).all()
        if mom == 0.0 and null != "running":
            assert (got["running_mean"] == prm["rm"]).all() and (got["running_var"] == prm["rv"]).all()
    if G >= 2048:                                   # the folded finalize reads doubles: a 4-byte-aligned pointer is refused
        N = 5
        part, rows, M = CS.hand_partials(G, N, 64, True)
        pd = torch.zeros(part.size + 1, device="cuda")
        v = [vecbuf(N) for _ in range(3)]
        assert lib.dml_bn_finalize(pd.data_ptr() + 4, M, N, 64, None, None, None, None, 0.1, CS.BN_EPS, v[0].data_ptr(), v[1].data_ptr(),
                                   v[2].data_ptr(), None, st()) == EALIGN


# ---------------------------------------------------------------------------------------------------------------------
# dml_bn_bwd_finalize
# ---------------------------------------------------------------------------------------------------------------------
def bwd_finalize(lib, h, nb, M, N, fused=None, null_gamma=False):
    pd = dev(h["part"])
    gamma = None if null_gamma else vecbuf(N, h["gamma"])
    mu, inv = vecbuf(N, h["mean"]), vecbuf(N, h["invstd"])
    dg, db, coef = vecbuf(N, h["dgamma0"]), vecbuf(N, h["dbeta0"]), vecbuf(4 * N)
    args = (pd.data_ptr(), nb, M, N, gamma.data_ptr() if gamma is not None else None, mu.data_ptr(), inv.data_ptr(), dg.data_ptr(),
            db.data_ptr(), coef.data_ptr())
    if fused is None:
        chk(lib.dml_bn_bwd_finalize(*args, st()))
    else:
        count, gw, work, state = fused
        chk(lib.dml_bn_bwd_finalize_bound(*args, count, gw.data_ptr(), work.data_ptr(), state.data_ptr(), st()))
    torch.cuda.synchronize()
    assert tail_ok(dg, N) and tail_ok(db, N) and tail_ok(coef, 4 * N)
    return dg[:N].cpu().numpy().astype(F64), db[:N].cpu().numpy().astype(F64), coef[:4 * N].cpu().numpy().astype(F64).reshape(4, N)


def check_bwd_finalize(lib, nb, N, M, fused=None, null_gamma=False):
    h = CS.bwd_hand_partials(nb, N)
    sums = h["part"].astype(F64).sum(0).T
    ref = CS.bwd_coef(sums, None if null_gamma else h["gamma"], h["mean"], h["invstd"], M)
    dg, db, coef = bwd_finalize(lib, h, nb, M, N, fused, null_gamma)
    assert (dg == h["dgamma0"] + sums[1]).all() and (db == h["dbeta0"] + sums[0]).all(), "dgamma / dbeta accumulate the exact sums"
    check_le("bwd finalize coef nb=%d N=%d M=%d" % (nb, N, M), np.abs(coef - ref), CS.EPS32 * np.abs(ref))
    assert (coef[3] == h["mean"]).all() and (coef[0] == ref[0]).all()
    if M == 0:
        assert (coef[1] == 0).all() and (coef[2] == 0).all()
    return ref, h


@pytest.mark.parametrize("nb", CS.BWD_FIN_BLOCKS)
def test_bwd_finalize_from_exact_partials(lib, nb):
    for i, N in enumerate(CS.BWD_FIN_NS):
        check_bwd_finalize(lib, nb, N, 64 * nb - 5, null_gamma=(i == 1 and nb == 65))
    # M = 0: fixed statistics -- no correction terms, and the parameter gradients ARE accumulated (float64 autograd of an eval()
    # BatchNorm: test_bn_refs.py::test_fixed_statistics_backward_adds_the_parameter_gradients)
    check_bwd_finalize(lib, nb, 5, 0)


# ---------------------------------------------------------------------------------------------------------------------
# synchronised pieces against the whole batch
# ---------------------------------------------------------------------------------------------------------------------
def test_sync_forward_against_the_statistics_of_the_whole_batch(lib):
    y = CS.sync_inputs()
    R, Me, N = y.shape
    moments = torch.full((R, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    refp, sbs, mbs, rows = [], [], [], []
    for r in range(R):
        yb = Buf(Me, N, data=y[r])
        G = -(-Me // 64)
        part = torch.zeros(G, N, 2, device="cuda")
        chk(lib.dml_bn_stats(yb.ptr, part.data_ptr(), Me, N, N, 0, st()))
        chk(lib.dml_bn_moments(part.data_ptr(), Me, N, 64, moments[r].data_ptr(), st()))
        p = CS.partials(y[r], 64)
        sb, mb = CS.stats_bars(y[r])
        refp.append(p), sbs.append(sb), mbs.append(mb), rows.append(CS.group_rows(Me, 64))
        torch.cuda.synchronize()
        # this rank's moments
        mean_bar, m2_bar = CS.merged_bars(p, rows[-1], sb, mb)
        _, mean, m2 = CS.chan_merge(p, rows[-1])
        got = moments[r].cpu().numpy()
        check_le("sync moments mean rank %d" % r, np.abs(got[:, 0] - mean), mean_bar + 1e-15 * np.abs(mean))
        check_le("sync moments M2 rank %d" % r, np.abs(got[:, 1] - m2), m2_bar + 1e-13 * (m2 + Me * mean ** 2))
    prm = CS.fin_params(N)
    mom = 0.1
    sc, sh, mu, inv, rm, rv = vecbuf(N), vecbuf(N), vecbuf(N), vecbuf(N), vecbuf(N, prm["rm"]), vecbuf(N, prm["rv"])
    g_d, b_d = dev(prm["gamma"]), dev(prm["beta"])
    chk(lib.dml_bn_finalize_moments(moments.data_ptr(), R, Me, N, g_d.data_ptr(), b_d.data_ptr(),
                                    rm.data_ptr(), rv.data_ptr(), mom, CS.BN_EPS, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                                    inv.data_ptr(), st()))
    torch.cuda.synchronize()
    allp, allr = np.concatenate(refp), np.concatenate(rows)
    mean_bar, m2_bar = CS.merged_bars(allp, allr, np.concatenate(sbs), np.concatenate(mbs))
    whole = y.reshape(-1, N).astype(F64)
    M = R * Me
    ref = CS.finalize_ref(M, whole.mean(0), whole.var(0) * M, prm["gamma"], prm["beta"], prm["rm"], prm["rv"], mom)
    bars = CS.finalize_bars(ref)
    dvar = m2_bar / M / (whole.var(0) + CS.BN_EPS)                  # relative movement of var + eps
    bars["mean"] = bars["mean"] + mean_bar
    bars["invstd"] = bars["invstd"] + 0.5 * dvar * ref["invstd"] * (1 + dvar)
    bars["scale"] = bars["scale"] + 0.5 * dvar * np.abs(ref["scale"]) * (1 + dvar)
    bars["running_mean"] = bars["running_mean"] + mom * mean_bar
    bars["running_var"] = bars["running_var"] + mom * m2_bar / (M - 1)
    got = {k: t[:N].cpu().numpy().astype(F64) for k, t in (("scale", sc), ("shift", sh), ("mean", mu), ("invstd", inv),
                                                             ("running_mean", rm), ("running_var", rv))}
    for t in (sc, sh, mu, inv, rm, rv):
        assert tail_ok(t, N)
    check_finalize(got, ref, bars, "sync, %d ranks of %d rows" % (R, Me))
    # the running variance is the unbiased one over the GLOBAL count: the biased one, or a per-rank count, is outside the bar
    assert (np.abs(mom * whole.var(0) / (M - 1)) > 4 * bars["running_var"]).all()


def test_sync_backward_against_float64_coefficients(lib):
    N, nb, R = 12, 7, 3
    hs = [CS.bwd_hand_partials(nb, N, seed=r) for r in range(R)]
    tot = np.zeros((N, 2))
    for h in hs:
        sums = torch.full((N + 2, 2), float("nan"), dtype=torch.float64, device="cuda")
        dg, db = vecbuf(N, h["dgamma0"]), vecbuf(N, h["dbeta0"])
        pd = dev(h["part"])
        chk(lib.dml_bn_bwd_sums(pd.data_ptr(), nb, N, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), st()))
        torch.cuda.synchronize()
        s = h["part"].astype(F64).sum(0)
        assert (sums[:N].cpu().numpy() == s).all() and bool(torch.isnan(sums[N:]).all())
        assert (dg[:N].cpu().numpy() == h["dgamma0"] + s[:, 1]).all() and (db[:N].cpu().numpy() == h["dbeta0"] + s[:, 0]).all()
        assert tail_ok(dg, N) and tail_ok(db, N)
        tot += s
    h = hs[0]
    M_total = R * CS.SYNC_M_EACH
    coef = vecbuf(4 * N)
    keep = [dev(a) for a in (tot, h["gamma"], h["mean"], h["invstd"])]
    chk(lib.dml_bn_bwd_coef(keep[0].data_ptr(), M_total, N, keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), coef.data_ptr(),
                            st()))
    torch.cuda.synchronize()
    ref = CS.bwd_coef(tot.T, h["gamma"], h["mean"], h["invstd"], M_total)
    assert tail_ok(coef, 4 * N)
    check_le("sync bwd coef", np.abs(coef[:4 * N].cpu().numpy().astype(F64).reshape(4, N) - ref), CS.EPS32 * np.abs(ref))


# ---------------------------------------------------------------------------------------------------------------------
# plane-scale bounds
# ---------------------------------------------------------------------------------------------------------------------
def new_work():
    return torch.full((1027,), float("nan"), device="cuda")


def work_scale(work):
    torch.cuda.synchronize()
    w = work.cpu().numpy()
    assert np.isnan(w[:1024]).all() and np.isnan(w[1025:]).all(), "the bound kernels write work[1024] only"
    return float(w[1024])


def optr(a):
    return None if a is None else a.data_ptr()


def test_bound_kernels_single_calls(lib):
    for name, case in CS.fwd_bound_cases().items():
        gamma, beta, N, count, mult, w = case
        keep = [None if a is None else dev(a) for a in (gamma, beta, w)]
        work = new_work()
        chk(lib.dml_h2_bound_bn(optr(keep[0]), optr(keep[1]), N, count, mult, optr(keep[2]), work.data_ptr(), st()))
        assert work_scale(work) == CS.unscale_of_bound(CS.fwd_bound_of(case)), name
    for name, case in CS.bwd_bound_cases().items():
        coef, invstd, count, w = case
        keep = [dev(coef.reshape(-1)), dev(invstd), dev(w)]
        work = new_work()
        chk(lib.dml_h2_bound_bn_bwd(keep[0].data_ptr(), keep[1].data_ptr(), coef.shape[1], count, keep[2].data_ptr(), work.data_ptr(), st()))
        assert work_scale(work) == CS.unscale_of_bound(CS.bwd_bound_of(case)), name


def rc32(count):
    return float(F32(np.sqrt(F32(count))) * F32(1.0001))


def test_bound_table_and_multi(lib):
    from dmlnet._lib import H2BoundDesc
    cases = {k: c for k, c in CS.fwd_bound_cases().items() if c[5] is None}
    keep, works, descs = [], [], []
    for name, (gamma, beta, N, count, mult, _) in cases.items():
        g, b, work = (None if gamma is None else dev(gamma)), (None if beta is None else dev(beta)), new_work()
        keep += [g, b]
        works.append(work)
        descs.append(H2BoundDesc(optr(g), optr(b), work.data_ptr(), N, rc32(count), mult, 0))
    raw = bytes((H2BoundDesc * len(descs))(*descs))
    tab = dev(np.frombuffer(raw, np.uint8).copy())
    chk(lib.dml_h2_bound_bn_table(tab.data_ptr(), len(descs), st()))
    for (name, case), work in zip(cases.items(), works):
        assert work_scale(work) == CS.unscale_of_bound(CS.fwd_bound_of(case)), name
    assert lib.dml_h2_bound_bn_table(tab.data_ptr(), 0, st()) == 0
    # one scale for a tensor several BatchNorms write slices of: the largest of the entries' bounds
    for Ns in CS.MULTI_CASES:
        descs, bounds, keep = [], [], []
        for i, N in enumerate(Ns):
            gamma, beta = CS.bound_params(N, seed=i)
            g, b = dev(gamma), dev(beta)
            keep += [g, b]
            descs.append(H2BoundDesc(g.data_ptr(), b.data_ptr(), None, N, rc32(297 * (i + 1)), 1.0 + i, 0))
            bounds.append(CS.fwd_bound(gamma, beta, N, 297 * (i + 1), 1.0 + i))
        tab = dev(np.frombuffer(bytes((H2BoundDesc * len(descs))(*descs)), np.uint8).copy())
        work = new_work()
        chk(lib.dml_h2_bound_bn_multi(tab.data_ptr(), len(descs), work.data_ptr(), st()))
        assert work_scale(work) == CS.unscale_of_bound(max(bounds)), Ns
        if len(Ns) > 1:
            assert len({CS.unscale_of_bound(b) for b in bounds}) > 1     # the entries would not all give that scale


@pytest.mark.parametrize("G,N,sr,mult,at", CS.FUSED_CASES)
def test_finalize_bound_equals_the_two_calls(lib, G, N, sr, mult, at):
    """dml_bn_finalize_bound: the statistics of dml_bn_finalize, the scale from the float64 bound, both state words zero afterwards;
    a second call on the same state with smaller parameters gives the smaller scale (no stale maximum, no stale ticket)"""
    part, rows, M = CS.hand_partials(G, N, sr, True)
    resw = None if at is None else dev(CS.words(CS.FUSED_RES_MAX, at))
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    scales = []
    for small in (False, True, False):
        gamma, beta = CS.bound_params(N, small=small)
        prm = dict(CS.fin_params(N), gamma=gamma, beta=beta)
        work = new_work()
        plain = finalize(lib, part, M, N, sr, prm, 0.1)
        fused = finalize(lib, part, M, N, sr, prm, 0.1, fused=(M, mult, resw, work, state))
        for k in plain:
            assert (plain[k] == fused[k]).all(), k
        want = CS.unscale_of_bound(CS.fwd_bound(gamma, beta, N, M, mult, 0.0 if at is None else CS.FUSED_RES_MAX))
        assert work_scale(work) == want, (small, work_scale(work), want)
        assert bool((state == 0).all()), "state words after the call: %s" % state.tolist()
        scales.append(want)
    assert scales[1] < scales[0] == scales[2]


@pytest.mark.parametrize("nb,N", CS.BWD_FUSED_CASES)
def test_bwd_finalize_bound_equals_the_two_calls(lib, nb, N):
    """dml_bn_bwd_finalize_bound: coefficients and parameter gradients of dml_bn_bwd_finalize, the scale from the float64 bound, the
    state words zero afterwards; a second call with everything 2^-8 smaller gives the 2^-8 smaller scale"""
    M = 64 * nb - 5
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    scales = []
    for f in (1.0, 2.0 ** -8, 1.0):
        h, gm, b = CS.bwd_fused_case(nb, N, f)
        gw = dev(CS.words(gm, 1023 if N == 260 else 0))
        work = new_work()
        dg, db, coef = bwd_finalize(lib, h, nb, M, N)
        dg2, db2, coef2 = bwd_finalize(lib, h, nb, M, N, fused=(M, gw, work, state))
        assert (dg == dg2).all() and (db == db2).all() and (coef == coef2).all()
        assert work_scale(work) == CS.unscale_of_bound(b), (f, work_scale(work), CS.unscale_of_bound(b))
        assert bool((state == 0).all()), "state words after the call: %s" % state.tolist()
        scales.append(CS.unscale_of_bound(b))
    assert scales[1] == scales[0] * 2.0 ** -8 and scales[0] == scales[2]


@pytest.mark.parametrize("M", CS.REACH_MS)
def test_reaching_the_bound(lib, M):
    """one row of ones among zeros drives xhat to sqrt(M - 1): stats -> finalize_bound -> apply with planes stays finite and below
    2^15, and hi + lo reconstructs z; the backward twin through reduce -> bwd_finalize_bound -> bwd_apply"""
    y, dz, gamma, beta = CS.reach_case(M)
    N = y.shape[1]
    yb = Buf(M, N, data=y)
    G = -(-M // 64)
    part = torch.zeros(G, N, 2, device="cuda")
    chk(lib.dml_bn_stats(yb.ptr, part.data_ptr(), M, N, N, 0, st()))
    sc, sh, mu, inv = vecbuf(N), vecbuf(N), vecbuf(N), vecbuf(N)
    g_d, b_d = dev(gamma), dev(beta)
    work, state = new_work(), torch.zeros(2, dtype=torch.int32, device="cuda")
    chk(lib.dml_bn_finalize_bound(part.data_ptr(), M, N, 64, g_d.data_ptr(), b_d.data_ptr(), None, None, 0.1, CS.BN_EPS, sc.data_ptr(),
                                  sh.data_ptr(), mu.data_ptr(), inv.data_ptr(), M, 1.0, None, work.data_ptr(), state.data_ptr(), st()))
    un = work_scale(work)
    bound = CS.fwd_bound(gamma, beta, N, M)
    assert un == CS.unscale_of_bound(bound)
    zb, pb = Buf(M, N), Buf(M, N, dtype="f16", planes=2)
    for zptr in (zb.ptr, None):                                     # beside z (four channels) and planes only (eight)
        chk(lib.dml_bn_apply(yb.ptr, None, zptr, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), None, M, N, N, N, N, 0, 0, 0.0, 0, None,
                             pb.ptr, pb.plane_stride, N, work.data_ptr() + 4096, 0, None, st()))
        torch.cuda.synchronize()
        z = zb.get().astype(F64)
        mean, var = CS.batch_stats(y)
        zref, _ = CS.fwd_ref(y, None, mean, gamma.astype(F64) / np.sqrt(var + CS.BN_EPS), beta, 0)
        check_le("reach z M=%d" % M, np.abs(z - zref), 1e-5 * np.abs(zref).max())
        p = pb.get()
        zmax = np.abs(z).max()
        assert np.isfinite(p.astype(F32)).all() and zmax / un < 2.0 ** 15
        if M > 2:
            assert zmax / un >= 2.0 ** 14                              # the top binade: half the bound would overflow
        check_le("reach planes reconstruct z M=%d" % M, np.abs((p[0].astype(F64) + p[1].astype(F64)) * un - z),
                 2.0 ** -21 * zmax + 2.0 ** -32 * bound)
        pb.assert_untouched_outside()
    # backward
    dzb = Buf(M, N, data=dz)
    bpart = torch.full((1100, N, 2), float("nan"), device="cuda")
    gw, nb = torch.zeros(1024, device="cuda"), C.c_int(0)
    chk(lib.dml_bn_bwd_reduce(dzb.ptr, yb.ptr, None, None, mu.data_ptr(), inv.data_ptr(), bpart.data_ptr(), M, N, N, N, N, 0, 1.0, 0,
                              C.byref(nb), gw.data_ptr(), st()))
    dg, db, coef = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), vecbuf(4 * N)
    dwork = new_work()
    chk(lib.dml_bn_bwd_finalize_bound(bpart.data_ptr(), nb.value, M, N, g_d.data_ptr(), mu.data_ptr(), inv.data_ptr(), dg.data_ptr(),
                                      db.data_ptr(), coef.data_ptr(), M, gw.data_ptr(), dwork.data_ptr(), state.data_ptr(), st()))
    dun = work_scale(dwork)
    assert bool((state == 0).all())
    dyb, dpb = Buf(M, N), Buf(M, N, dtype="f16", planes=2)
    chk(lib.dml_bn_bwd_apply(dzb.ptr, yb.ptr, None, None, coef.data_ptr(), dyb.ptr, None, M, N, N, N, N, N, 0, 0, 1.0, 0, 0, None,
                             dpb.ptr, dpb.plane_stride, N, dwork.data_ptr() + 4096, st()))
    torch.cuda.synchronize()
    dy = dyb.get().astype(F64)
    mean, var = CS.batch_stats(y)
    invstd = 1.0 / np.sqrt(var + CS.BN_EPS)
    g = CS.bwd_g(dz, None, 1.0)
    cref = CS.bwd_coef(CS.bwd_sums(g, y, mean, invstd), gamma, mean, invstd, M)
    dref = CS.bwd_apply_ref(g, y, cref)
    terms = np.abs(cref[0] * g) + np.abs(cref[1] * (y - cref[3])) + np.abs(cref[2])      # (M = 2: dy itself cancels to ~0)
    check_le("reach dy M=%d" % M, np.abs(dy - dref), 1e-5 * terms.max())
    bb = CS.bwd_bound(cref, invstd, M, np.abs(g).max())
    dmax = np.abs(dy).max()
    p = dpb.get()
    assert np.log2(dun) == np.round(np.log2(dun)) and dun <= CS.unscale_of_bound(bb * 1.001) and dun >= CS.unscale_of_bound(bb * 0.999)
    assert np.isfinite(p.astype(F32)).all() and dmax / dun < 2.0 ** 15
    check_le("reach planes reconstruct dy M=%d" % M, np.abs((p[0].astype(F64) + p[1].astype(F64)) * dun - dy),
             2.0 ** -21 * dmax + 2.0 ** -32 * bb)


# ---------------------------------------------------------------------------------------------------------------------
# dml_bn_eval_coeffs_table
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_coeffs_table(lib):
    from dmlnet._lib import BnEvalDesc
    rs = np.random.RandomState(8)
    ents, descs, keep = [], [], []
    for i, N in enumerate((5, 72, 260)):
        gamma, beta = (None, None) if i == 1 else (rs.standard_normal(N).astype(F32), rs.standard_normal(N).astype(F32))
        rm, rv, eps = rs.standard_normal(N).astype(F32), rs.uniform(1e-7, 2.0, N).astype(F32), (1e-5, 1e-3, 1e-5)[i]
        t = [None if a is None else dev(a) for a in (gamma, beta, rm, rv)]
        sc, sh, sc1, sh1 = vecbuf(N), vecbuf(N), vecbuf(N), vecbuf(N)
        keep += t
        ents.append((N, gamma, beta, rv, eps, sc, sh, sc1, sh1))
        descs.append(BnEvalDesc(optr(t[0]), optr(t[1]), t[3].data_ptr(), sc.data_ptr(), sh.data_ptr(), N, eps))
        chk(lib.dml_bn_eval_coeffs(optr(t[0]), optr(t[1]), t[2].data_ptr(), t[3].data_ptr(), eps, sc1.data_ptr(), sh1.data_ptr(), N, st()))
    tab = dev(np.frombuffer(bytes((BnEvalDesc * 3)(*descs)), np.uint8).copy())
    chk(lib.dml_bn_eval_coeffs_table(tab.data_ptr(), 3, st()))
    torch.cuda.synchronize()
    for N, gamma, beta, rv, eps, sc, sh, sc1, sh1 in ents:
        assert tail_ok(sc, N) and tail_ok(sh, N) and torch.equal(sc[:N], sc1[:N]) and torch.equal(sh[:N], sh1[:N])
        g64 = np.ones(N) if gamma is None else gamma.astype(F64)
        # float32: rv + eps, sqrt, 1 / x, the product: the sum's rounding reaches the result halved
        ref = g64 / np.sqrt(rv.astype(F64) + F64(F32(eps)))
        check_le("eval coeffs scale N=%d" % N, np.abs(sc[:N].cpu().numpy() - ref), 3.5 * CS.EPS32 * np.abs(ref))
        assert (sh[:N].cpu().numpy() == (np.zeros(N, F32) if beta is None else beta)).all()


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(lib):
    M = 4
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    nb = C.c_int(0)

    def ap(N, ldy, ldres, ldz, dt, res=True, z=True, planes=None, relu=1, mask=None):
        return lib.dml_bn_apply(p, p if res else None, p if z else None, p, p, p, mask, M, N, ldy, ldres, ldz, relu, dt, 0.0, 0, None,
                                planes, 1024, N, p if planes else None, 0, None, st())

    for dt, V in ((0, 4), (1, 8)):
        assert ap(V + 2, 16, 16, 16, dt) == EALIGN                 # N
        assert ap(8, 8 + V // 2, 16, 16, dt) == EALIGN             # ldy
        assert ap(8, 16, 8 + V // 2, 16, dt) == EALIGN             # ldres
        assert ap(8, 16, 16, 8 + V // 2, dt) == EALIGN             # ldz
        assert lib.dml_bn_bwd_reduce(p, p, p, None, p, p, p, M, V + 2, 16, 16, 16, 1, 1.0, dt, C.byref(nb), None, st()) == EALIGN
        assert lib.dml_bn_bwd_reduce(p, p, p, None, p, p, p, M, 8, 8 + V // 2, 16, 16, 1, 1.0, dt, C.byref(nb), None, st()) == EALIGN
        assert lib.dml_bn_bwd_reduce(p, p, None, None, p, p, p, M, 8, 16, 16, 16, 1, 1.0, dt, C.byref(nb), None, st()) == EINVAL
        assert lib.dml_bn_bwd_apply(p, p, p, None, p, p, None, M, 8, 16, 16, 16, 8 + V // 2, 0, 1, 1.0, 0, dt, None, None, 0, 0, None,
                                    st()) == EALIGN                 # lddy
        assert lib.dml_bn_bwd_apply(p, p, p, None, p, p, p, M, 8, 16, 16, 16, 16, 8 + V // 2, 1, 1.0, 0, dt, None, None, 0, 0, None,
                                    st()) == EALIGN                 # lddres
        assert lib.dml_bn_bwd_apply(p, p, None, None, p, p, None, M, 8, 16, 16, 16, 16, 0, 1, 1.0, 0, dt, None, None, 0, 0, None,
                                    st()) == EINVAL                 # relu without z and mask
    assert ap(8, 8, 8, 8, 1, planes=p) == EINVAL                   # planes with bf16
    assert lib.dml_bn_bwd_apply(p, p, p, None, p, p, None, M, 8, 8, 8, 8, 8, 0, 1, 1.0, 0, 1, None, p, 1024, 8, p, st()) == EINVAL
    assert ap(8, 8, 8, 8, 0, z=False) == EINVAL                    # neither z nor planes
    st32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    fin = (p, 64, 4, 64, p, p, None, None, 0.1, 1e-5, p, p, p, p)
    assert lib.dml_bn_finalize_bound(*fin, 0, 1.0, None, p, st32.data_ptr(), st()) == EINVAL         # count <= 0
    assert lib.dml_bn_finalize_bound(*fin, 64, 1.0, None, p, None, st()) == EINVAL                    # no state
    bf = (p, 1, 64, 4, p, p, p, p, p, p)
    assert lib.dml_bn_bwd_finalize_bound(*bf, 0, p, p, st32.data_ptr(), st()) == EINVAL
    assert lib.dml_bn_bwd_finalize_bound(*bf, 64, p, p, None, st()) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and bool((st32 == 0).all())        # a refused call launches nothing
