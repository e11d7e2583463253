"""GPU: the pooling, resize and broadcast kernels of csrc/pool_resize.hip and the optimizer step, fill and conversion of
csrc/optim_layout.hip at their edges, through the C ABI -- every case of tests/pool_cases.py.

Every comparison is against the float64 definitions of tests/pool_cases.py on the same float32 / bfloat16 inputs (proved right on
these inputs, without a GPU, by tests/test_pool_refs.py).  Exact (dyadic) inputs must be reproduced EXACTLY -- a bfloat16 output as
the single rounding of the float64 value; maxima, argmax bytes, copies and conversions bit for bit -- real-valued inputs per
element against bars that count the float32 roundings of the contract.  Every output sits between two guard regions of 0xAA bytes,
and in a slice also beside columns of them: all of that must be bitwise unchanged afterwards.  Each float check prints
"MEASURE <what> err=<largest share of its bar> bar=<that bar>" before it asserts (run with -s to see the figures).

Largest share of its bar measured on the MI355X, as error of bar (the whole file, 73 tests, takes about 4 s there; the slowest
test 0.4 s):
  exact cases (max pool values / argmax / gradients, sums, broadcasts, resizes, upsample, SGD, fill, convert)   all equal
  sums over HW, f32          2.5e-5  of 1.9e-4   (HW = 32, the channel with |mean| / std = 1e4);  with 1 / HW 5.1e-7 of 4.0e-6
  avgpool_bwd set / add, f32 1.1e-8  of 1.5e-8;  1.1e-8 of 2.4e-8   (HW = 33)
  bilinear forward, f32      1.6e-6  of 5.2e-6   (33 x 33 -> 129 x 129, C = 256);  transpose 4.8e-8 of 1.6e-7 (13 x 10 <- 5 x 4)
  adaptive average pool, f32 1.2e-7  of 2.6e-7
  NHWC -> NCHW upsample      5.4e-8  of 1.4e-7
  SGD                        v 1.4e-8 of 2.3e-8;  p 3.3e-10 of 9.4e-10
  every bfloat16 output      ties of the store: half an ulp of the value's binade is reached, never passed

Tried on a scratch copy, one at a time, and caught by this file: `>=` for `>` in maxpool_fwd_kernel (the tie cases), blockDim.x as
sgd_kernel's stride (above the cap), a bfloat16 store in reduce_hw_kernel<bf16_t, float> (257), an accumulating dml_avgpool_bwd_set
(the NaN prefill), truncation in f32_to_bf16 (convert, and every bfloat16 store with a bar).  NOT caught, and not catchable:
dropping the +-1 margin of Y0 / Y1 in the bilinear_bwd kernels.  floor / ceil of the inverse map already enclose every destination
row with a non-zero weight; a float32 emulation of the window finds none lost at any pair of extents up to 96 (nor at the
geometries here), so the kernel without the margin computes the same numbers.  The identity, shrinking and extent-1 resizes are
right as they stand: no kernel had to be changed.
"""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import pool_cases as PC

pytestmark = pytest.mark.gpu

EINVAL, EALIGN = -1, -2
F32, F64 = np.float32, np.float64
DT = {"f32": (0, torch.float32, 4), "bf16": (1, torch.bfloat16, 2), "u8": (None, torch.uint8, 1)}
GUARD = 256                                    # guard elements before and after (a multiple of every vector length)
DTYPES = ("f32", "bf16")


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc
    torch.cuda.synchronize()


def check_le(what, err, bar):
    err, bar = np.asarray(err, F64), np.asarray(bar, F64) * np.ones_like(np.asarray(err, F64))
    assert np.isfinite(err).all(), "%s: non-finite error" % what
    k = int(np.argmax(np.where(err > bar, np.inf, err / np.maximum(bar, 1e-300)))) if err.size else 0      # the worst share of its bar
    print("MEASURE %s err=%.3e bar=%.3e" % (what, err.flat[k] if err.size else 0.0, bar.flat[k] if err.size else 0.0))
    assert (err <= bar).all(), "%s: error %.3e above the bar %.3e at %d elements" % (what, err.flat[k], bar.flat[k], int((err > bar).sum()))


def check_eq(what, got, ref):
    ok = PC.same(got, ref)
    assert ok.all(), "%s: %d of %d elements differ from the exact value" % (what, int((~ok).sum()), ok.size)


class Buf:
    """GUARD elements, rows x ld elements, GUARD elements on the device, every byte 0xAA; the addressed rows x N region starts at column
    `off`; `lead` shifts everything by that many elements (alignment cases).  data: float values, or bit patterns (unsigned integers of
    the element's width), or bytes for u8."""

    def __init__(self, rows, N, ld=None, off=0, dtype="f32", data=None, lead=0):
        self.rows, self.N, self.ld, self.off, self.kind = rows, N, ld or N, off, dtype
        assert off + N <= self.ld and rows >= 1
        _, self.tdt, self.esize = DT[dtype]
        self.raw = torch.full(((lead + 2 * GUARD + rows * self.ld) * self.esize,), 0xAA, dtype=torch.uint8, device="cuda")
        self.body = self.raw.view(self.tdt)[lead + GUARD:lead + GUARD + rows * self.ld].view(rows, self.ld)
        self.ptr = self.body.data_ptr() + off * self.esize
        if data is not None:
            self.set(data)

    def region(self):
        return self.body[:, self.off:self.off + self.N]

    def set(self, data):
        a = np.ascontiguousarray(data)
        if a.dtype in (np.uint32, np.uint16) and self.kind != "u8":
            t = torch.from_numpy(a.view(F32 if a.dtype == np.uint32 else np.int16).reshape(self.rows, self.N))
            t = t if self.kind == "f32" else t.view(torch.bfloat16)
        elif self.kind == "u8":
            t = torch.from_numpy(a.astype(np.uint8).reshape(self.rows, self.N))
        else:
            t = torch.from_numpy(a.astype(F32).reshape(self.rows, self.N)).to(self.tdt)
        assert t.dtype == self.tdt
        self.region().copy_(t.cuda())

    def get(self, shape=None):
        r = self.region()
        r = (r.cpu() if self.kind == "u8" else r.float().cpu()).numpy()
        return r if shape is None else r.reshape(shape)

    def bits(self):
        r = self.region().contiguous().cpu()
        return r.numpy().view(np.uint32).reshape(-1) if self.kind == "f32" else r.view(torch.int16).numpy().view(np.uint16).reshape(-1)

    def untouched(self):
        c = self.raw.clone()
        v = c.view(self.tdt)
        lo = v.numel() - GUARD - self.rows * self.ld
        v[lo:lo + self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.N] = v[0]
        assert bool((c == 0xAA).all()), "a byte outside the addressed region was written"


def sliced(rows, C, lay, dtype, data=None):
    """a buffer for `lay` = (ld, offset)"""
    return Buf(rows, C, lay[0], lay[1], dtype, data)


# ---------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", PC.MAXPOOL_KINDS)
def test_maxpool_forward_ties_and_backward_scatter(lib, kind, dtype):
    """the value is the window maximum bit for bit (NaN: a NaN), the argmax byte the first maximum in tap order -- with ReLU data, a
    constant image, -inf windows -- and the backward puts every window's gradient where the reference's tap says"""
    dt = DT[dtype][0]
    for B, Hh, Ww, Cc in PC.maxpool_cases(dtype):
        what = "%s %s B=%d %dx%d C=%d" % (kind, dtype, B, Hh, Ww, Cc)
        x = PC.maxpool_input(kind, B, Hh, Ww, Cc, dtype)
        y, tap = PC.maxpool_fwd(x)
        Ho, Wo = y.shape[1:3]
        xb, yb, ab = Buf(B * Hh * Ww, Cc, dtype=dtype, data=x), Buf(B * Ho * Wo, Cc, dtype=dtype), Buf(B * Ho * Wo, Cc, dtype="u8")
        chk(lib.dml_maxpool3x3s2_fwd(xb.ptr, yb.ptr, ab.ptr, B, Hh, Ww, Cc, dt, st()))
        check_eq("max pool value " + what, yb.get(y.shape), y)
        got = ab.get(tap.shape)
        pinned = ~np.isnan(y)
        assert (got[pinned] == tap[pinned]).all(), "%s: %d argmax bytes are not the first maximum" % (what, int((got != tap)[pinned].sum()))
        yb.untouched(), ab.untouched()
        y2 = Buf(B * Ho * Wo, Cc, dtype=dtype)                      # argmax is optional
        chk(lib.dml_maxpool3x3s2_fwd(xb.ptr, y2.ptr, None, B, Hh, Ww, Cc, dt, st()))
        check_eq("max pool value without argmax " + what, y2.get(y.shape), y)
        g = PC.maxpool_grad(B, Hh, Ww, Cc)
        gb, tb, dxb = Buf(B * Ho * Wo, Cc, dtype=dtype, data=g), Buf(B * Ho * Wo, Cc, dtype="u8", data=tap), Buf(B * Hh * Ww, Cc, dtype=dtype)
        chk(lib.dml_maxpool3x3s2_bwd(gb.ptr, tb.ptr, dxb.ptr, B, Hh, Ww, Cc, dt, st()))
        check_eq("max pool gradient " + what, dxb.get(x.shape), PC.store(PC.maxpool_bwd(g, tap, Hh, Ww), dtype))
        dxb.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# sums over HW
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", PC.RED_HW)
def test_sums_over_hw(lib, HW, dtype):
    """dml_reduce_hw, dml_global_avgpool_fwd and dml_reduce_hw_f32 where reduce_hw_kernel's two loops hand over, one vector column
    either side of a workgroup's eight, dense and in a slice; the float32 form must not round to bfloat16 (channel 0 sums to 257)"""
    V, dt, B = PC.vec(dtype), DT[dtype][0], PC.RED_B
    inv = float(F32(1) / F32(HW))
    for cv in PC.RED_CV:
        Cc = cv * V
        for lay in PC.layouts(Cc, V):
            for kind in ("exact", "real"):
                what = "%s %s HW=%d C=%d ld=%d" % (kind, dtype, HW, Cc, lay[0])
                x = PC.reduce_input(kind, B, HW, Cc, dtype)
                xb = sliced(B * HW, Cc, lay, dtype, x)
                exact1, exacth = kind == "exact", kind == "exact" and PC.pow2(HW)

                def check(name, ob, scale, is_exact, odt):
                    ref = PC.sum_hw(x, scale)
                    if is_exact:
                        check_eq(name + " " + what, ob.get(), PC.store(ref, odt))
                    else:
                        check_le(name + " " + what, np.abs(ob.get().astype(F64) - ref), PC.stored_bar(PC.sum_bar(x, scale, True), ref, odt))
                    ob.untouched()

                o = Buf(B, Cc, dtype=dtype)
                chk(lib.dml_reduce_hw(xb.ptr, o.ptr, B, HW, Cc, lay[0], dt, st()))
                check("reduce_hw", o, 1.0, exact1, dtype)
                o = Buf(B, Cc, dtype=dtype)
                chk(lib.dml_global_avgpool_fwd(xb.ptr, o.ptr, B, HW, Cc, lay[0], dt, st()))
                check("global_avgpool", o, inv, exacth, dtype)
                for scale, ex in ((1.0, exact1), (inv, exacth)):
                    o = Buf(B, Cc, dtype="f32")
                    chk(lib.dml_reduce_hw_f32(xb.ptr, o.ptr, B, HW, Cc, lay[0], dt, scale, st()))
                    check("reduce_hw_f32 scale=%g" % scale, o, scale, ex, "f32")
                    if exact1 and HW >= 2 and scale == 1.0:
                        assert (o.get()[:, 0] == 257).all(), "the float32 sum was rounded to bfloat16"


# ---------------------------------------------------------------------------------------------------------------------
# broadcasts
# ---------------------------------------------------------------------------------------------------------------------
def check_broadcasts(lib, dtype, kind, B, HW, Cc, lay):
    dt = DT[dtype][0]
    what = "%s %s HW=%d C=%d ld=%d" % (kind, dtype, HW, Cc, lay[0])
    v, dx0 = PC.broadcast_input(kind, B, HW, Cc, dtype)
    vb = Buf(B, Cc, dtype=dtype, data=v)
    z = sliced(B * HW, Cc, lay, dtype)
    chk(lib.dml_broadcast_hw(vb.ptr, z.ptr, B, HW, Cc, lay[0], dt, st()))
    check_eq("broadcast_hw " + what, z.get((B, HW, Cc)), PC.broadcast_hw(v, HW))
    z.untouched()
    exact = kind == "exact" and PC.pow2(HW)
    for name, fn, old in (("avgpool_bwd_set", lib.dml_avgpool_bwd_set, None), ("avgpool_bwd_add", lib.dml_avgpool_bwd_add, dx0)):
        # set: the slice holds NaN beforehand -- the result cannot depend on it
        d = sliced(B * HW, Cc, lay, dtype, np.full((B, HW, Cc), np.nan, F32) if old is None else old)
        chk(fn(vb.ptr, d.ptr, B, HW, Cc, lay[0], dt, st()))
        ref = PC.avgpool_bwd(v, HW, old)
        if exact:
            check_eq(name + " " + what, d.get((B, HW, Cc)), PC.store(ref, dtype))
        else:
            check_le(name + " " + what, np.abs(d.get((B, HW, Cc)).astype(F64) - ref), PC.stored_bar(PC.avgpool_bwd_bar(v, HW, old), ref, dtype))
        d.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_broadcasts_over_hw(lib, dtype):
    V = PC.vec(dtype)
    for HW in PC.BC_HW:
        for cv in PC.RED_CV:
            for lay in PC.layouts(cv * V, V):
                for kind in ("exact", "real"):
                    check_broadcasts(lib, dtype, kind, PC.RED_B, HW, cv * V, lay)


@pytest.mark.parametrize("dtype", DTYPES)
def test_broadcasts_above_the_grid_cap(lib, dtype):
    """532 480 vector items: the grid-stride loop of broadcast_hw_kernel takes a second trip"""
    B, HW, cv = PC.BC_BIG
    check_broadcasts(lib, dtype, "exact", B, HW, cv * PC.vec(dtype), PC.layouts(cv * PC.vec(dtype), PC.vec(dtype))[1])


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize
# ---------------------------------------------------------------------------------------------------------------------
def run_bilinear(lib, bwd, geom, B, Cc, flags, layout, cache):
    """one dml_bilinear_fwd / dml_bilinear_bwd call checked against the definition"""
    h, w, Hh, Ww = geom
    bf, in32, out32 = flags
    idt = "f32" if (in32 or not bf) else "bf16"
    odt = "f32" if (out32 or not bf) else "bf16"
    exact = geom in PC.BILINEAR_EXACT or geom == PC.BILINEAR_BIG_BWD[1:5]
    ishape, oshape = ((B, Hh, Ww, Cc), (B, h, w, Cc)) if bwd else ((B, h, w, Cc), (B, Hh, Ww, Cc))
    key = (Cc, idt)
    if key not in cache:
        a = PC.bilinear_input(ishape, exact, idt, seed=1 if bwd else 0)
        ref = PC.bilinear_bwd(a, h, w) if bwd else PC.bilinear_fwd(a, Hh, Ww)
        cache[key] = (a, ref, None if exact else PC.bilinear_bar(a, h, w, Hh, Ww, bwd))
    a, ref, bar = cache[key]
    (ps, os_), (pd, od) = PC.BILINEAR_LAYOUTS[layout]
    sb = Buf(int(np.prod(ishape[:3])), Cc, Cc + ps, os_, idt, a)
    db = Buf(int(np.prod(oshape[:3])), Cc, Cc + pd, od, odt)
    fn = lib.dml_bilinear_bwd if bwd else lib.dml_bilinear_fwd
    chk(fn(sb.ptr, db.ptr, B, h, w, Hh, Ww, Cc, Cc + ps, Cc + pd, 1 if bf else 0, in32, out32, st()))
    what = "%s %s C=%d %s->%s %s" % ("bilinear_bwd" if bwd else "bilinear_fwd", geom, Cc, idt, odt, layout)
    got = db.get(oshape)
    if exact:
        check_eq(what, got, PC.store(ref, odt))
    else:
        check_le(what, np.abs(got.astype(F64) - ref), PC.stored_bar(bar, ref, odt))
    db.untouched()


@pytest.mark.parametrize("geom", PC.BILINEAR_GEOMS)
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_bilinear_geometries_dtypes_and_slices(lib, bwd, geom):
    """enlarging, identity, shrinking and an output extent of 1, each way; all four in_f32 / out_f32 combinations; the scalar kernels
    (C = 4, 12) and the bf16 16-byte ones (C = 8, 24) with their fall-back for a slice that starts 8 bytes into a vector"""
    cache = {}
    for flags in PC.BILINEAR_FLAGS:
        for Cc in PC.BILINEAR_C:
            for layout in PC.BILINEAR_LAYOUTS:
                run_bilinear(lib, bwd, geom, PC.BILINEAR_B, Cc, flags, layout, cache)


def test_bilinear_forward_above_the_grid_cap(lib):
    B, h, w, Hh, Ww, Cc = PC.BILINEAR_BIG_FWD
    run_bilinear(lib, False, (h, w, Hh, Ww), B, Cc, (0, 0, 0), "dense", {})


def test_bilinear_backward_above_the_grid_cap(lib):
    B, h, w, Hh, Ww, Cc = PC.BILINEAR_BIG_BWD
    run_bilinear(lib, True, (h, w, Hh, Ww), B, Cc, (0, 0, 0), "dense", {})


# ---------------------------------------------------------------------------------------------------------------------
# adaptive average pool, NHWC -> NCHW upsample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PC.ADAPTIVE_CASES)
def test_adaptive_avgpool(lib, case, dtype):
    B, Hh, Ww, Cc, ld = case
    x = PC.adaptive_input(B, Hh, Ww, Cc, dtype)
    xb = Buf(B * Hh * Ww, Cc, ld, 0, dtype, x)
    for S in PC.ADAPTIVE_S:
        y, mag, cnt = PC.adaptive_avgpool(x, S)
        n = int(lib.dml_adaptive_avgpool_ws_elems(B, Hh, Ww, Cc, S))
        ws = Buf(1, n, dtype="f32")
        yb = Buf(B * S * S, Cc, dtype=dtype)
        chk(lib.dml_adaptive_avgpool_fwd(xb.ptr, yb.ptr, ws.ptr, B, Hh, Ww, Cc, ld, S, DT[dtype][0], st()))
        check_le("adaptive_avgpool %s %s S=%d" % (case, dtype, S), np.abs(yb.get(y.shape).astype(F64) - y),
                 PC.stored_bar(PC.adaptive_bar(mag, cnt), y, dtype))
        yb.untouched(), ws.untouched()


def run_upsample(lib, src, dst0, Hh, Ww, alpha, ld, lead, accumulate, exact, what):
    B, h, w, Cc = src.shape
    sb = Buf(B * h * w, Cc, ld, 0, "f32", src)
    db = Buf(1, B * Cc * Hh * Ww, dtype="f32", data=dst0 if accumulate else None, lead=lead)
    chk(lib.dml_upsample_nhwc_to_nchw(sb.ptr, db.ptr, B, h, w, ld, Cc, Hh, Ww, alpha, accumulate, st()))
    old = dst0 if accumulate else None
    ref = PC.upsample_nchw(src, Hh, Ww, alpha, old)
    got = db.get(ref.shape)
    if exact:
        check_eq(what, got, ref)
    else:
        check_le(what, np.abs(got.astype(F64) - ref), PC.upsample_bar(src, Hh, Ww, alpha, old))
    db.untouched()


@pytest.mark.parametrize("kind", list(PC.UPSAMPLE_KINDS))
def test_upsample_nhwc_to_nchw(lib, kind):
    """W = 1, 3, 7: the scalar tail; W = 4, 8: float4 stores, and their scalar fall-back when the destination is one float off"""
    for Ww in PC.UPSAMPLE_W:
        src, dst0, Hh, alpha = PC.upsample_input(kind, Ww)
        for lead in (0, 1):
            for acc in (0, 1):
                run_upsample(lib, src, dst0, Hh, Ww, alpha, PC.UPSAMPLE_LD, lead, acc, kind == "exact",
                             "upsample %s W=%d lead=%d accumulate=%d" % (kind, Ww, lead, acc))


def test_upsample_above_the_grid_cap(lib):
    B, h, w, Cc, Hh, Ww = PC.UPSAMPLE_BIG
    src = PC.bilinear_input((B, h, w, Cc), True, "f32")
    run_upsample(lib, src, None, Hh, Ww, 0.5, Cc, 0, 0, True, "upsample above the cap")


# ---------------------------------------------------------------------------------------------------------------------
# SGD, fill, convert
# ---------------------------------------------------------------------------------------------------------------------
def run_sgd(lib, kind, n, prm):
    lr, mu, wd, gs = prm
    p0, v0, grads = PC.sgd_input(kind, n)
    pb, vb = Buf(1, n, dtype="f32", data=p0), Buf(1, n, dtype="f32", data=v0)
    for step, g in enumerate(grads):
        p_in, v_in = pb.get()[0], vb.get()[0]                      # the state the kernel itself had before this step
        gb = Buf(1, n, dtype="f32", data=g)
        chk(lib.dml_sgd_step(pb.ptr, gb.ptr, vb.ptr, n, lr, mu, wd, gs, st()))
        rp, rv, bp, bv = PC.sgd_step(p_in, g, v_in, lr, mu, wd, gs)
        what = "%s n=%d lr=%g mu=%g wd=%g gscale=%g step %d" % (kind, n, lr, mu, wd, gs, step)
        if kind == "exact":
            check_eq("sgd v " + what, vb.get()[0], rv)
            check_eq("sgd p " + what, pb.get()[0], rp)
        else:
            check_le("sgd v " + what, np.abs(vb.get()[0].astype(F64) - rv), bv)
            check_le("sgd p " + what, np.abs(pb.get()[0].astype(F64) - rp), bp)
        assert (gb.get()[0] == g).all()
        pb.untouched(), vb.untouched(), gb.untouched()


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_sgd_steps(lib, kind):
    """n < 4 is the scalar tail alone; gscale != 1, wd = 0 and mu = 0; three steps, each against the float64 step from the kernel's
    own previous state"""
    for n in PC.SGD_NS[:-1]:
        for prm in (PC.SGD_EXACT if kind == "exact" else PC.SGD_REAL):
            run_sgd(lib, kind, n, prm)


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_sgd_above_the_grid_cap(lib, kind):
    """524 588 float4 items and a tail of three: the stride of the second trip and the tail's index must not mix"""
    run_sgd(lib, kind, PC.SGD_NS[-1], PC.SGD_EXACT[0] if kind == "exact" else PC.SGD_REAL[1])


def test_fill(lib):
    for n in PC.FILL_NS:
        for val in PC.FILL_VALUES:
            b = Buf(1, n, dtype="f32")
            chk(lib.dml_fill_f32(b.ptr, n, val, st()))
            got = b.bits()
            if val != val:
                assert np.isnan(got.view(F32)).all()
            else:
                assert (got == np.array([val], F32).view(np.uint32)[0]).all(), "fill %r n=%d" % (val, n)
            b.untouched()


@pytest.mark.parametrize("src,dst", PC.CONVERT_DIRS)
def test_convert_bit_for_bit(lib, src, dst):
    """round to nearest even at exact ties, the overflow to inf, denormals, signed zeros, infinities and NaN -- in every block of an
    array longer than one trip of the grid"""
    for n in PC.FILL_NS:
        bits = PC.convert_input(n, src)
        sb, db = Buf(1, n, dtype=src, data=bits), Buf(1, n, dtype=dst)
        chk(lib.dml_convert_dtype(sb.ptr, db.ptr, n, DT[src][0], DT[dst][0], st()))
        ok = PC.bits_same(db.bits(), PC.convert_ref(bits, src, dst), dst)
        assert ok.all(), "convert %s -> %s n=%d: %d elements differ, the first at %d" % (src, dst, n, int((~ok).sum()), int(np.argmin(ok)))
        db.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# refusals (all before any launch: the output stays untouched)
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    x, y, a = Buf(64, 16, dtype="f32"), Buf(64, 16, dtype="f32"), Buf(64, 16, dtype="u8")
    for dtype, bad in (("f32", 6), ("bf16", 12)):
        dt = DT[dtype][0]
        assert lib.dml_maxpool3x3s2_fwd(x.ptr, y.ptr, a.ptr, 1, 2, 2, bad, dt, st()) == EALIGN
        assert lib.dml_maxpool3x3s2_bwd(y.ptr, a.ptr, x.ptr, 1, 2, 2, bad, dt, st()) == EALIGN
        for fn in (lib.dml_reduce_hw, lib.dml_global_avgpool_fwd, lib.dml_broadcast_hw, lib.dml_avgpool_bwd_add, lib.dml_avgpool_bwd_set):
            assert fn(x.ptr, y.ptr, 1, 2, bad, 16, dt, st()) == EALIGN
            assert fn(x.ptr, y.ptr, 1, 2, 8, bad, dt, st()) == EALIGN        # the leading dimension as well
        assert lib.dml_reduce_hw_f32(x.ptr, y.ptr, 1, 2, bad, 16, dt, 1.0, st()) == EALIGN
        ws = Buf(1, 1024, dtype="f32")
        assert lib.dml_adaptive_avgpool_fwd(x.ptr, y.ptr, ws.ptr, 1, 2, 2, bad, 16, 1, dt, st()) == EALIGN
    for fn in (lib.dml_bilinear_fwd, lib.dml_bilinear_bwd):
        assert fn(x.ptr, y.ptr, 1, 2, 2, 4, 4, 6, 6, 6, 0, 0, 0, st()) == EALIGN
    for B, Hh, Ww in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2), (1, -3, 2), (1, 2, -3)):
        assert lib.dml_maxpool3x3s2_fwd(x.ptr, y.ptr, a.ptr, B, Hh, Ww, 4, 0, st()) == EINVAL
        assert lib.dml_maxpool3x3s2_bwd(y.ptr, a.ptr, x.ptr, B, Hh, Ww, 4, 0, st()) == EINVAL
    p, g, v = (Buf(1, 64, dtype="f32") for _ in range(3))
    for k in range(3):
        ptrs = [p.ptr, g.ptr, v.ptr]
        ptrs[k] += 4
        assert lib.dml_sgd_step(ptrs[0], ptrs[1], ptrs[2], 8, 0.1, 0.9, 0.0, 1.0, st()) == EALIGN
    for sd, dd in ((2, 0), (0, 2), (-1, 1), (1, 7)):
        assert lib.dml_convert_dtype(x.ptr, y.ptr, 8, sd, dd, st()) == EINVAL
    torch.cuda.synchronize()
    for b in (x, y, a, p, g, v):
        assert bool((b.raw == 0xAA).all()), "a refused call wrote something"
