"""GPU: the weight-layout, input-packing, space-to-depth, tap-gather and bias-gradient kernels of csrc/optim_layout.hip at their
edges, through the C ABI -- every case of tests/layout_cases.py.

Layouts are compared bit for bit with the reshape / transpose definitions of tests/layout_cases.py (proved right, without a GPU,
by tests/test_layout_refs.py); the bias gradient must EQUAL the float64 sum on integer inputs and stay inside the counted bar
c * 2^-24 * (|db before| + sum |dy|) on real ones (layout_cases.bias_chain counts c from the code).  Every output sits between two
guard regions of 0xAA bytes, and a slice beside guard columns: all of that must be bitwise unchanged afterwards.  Each float
check prints "MEASURE <what> err=<largest share of its bar> bar=<that bar>" before it asserts (run with -s to see the figures).

Measured on the MI355X (the whole file, 37 tests, takes about 2.5 s there; the slowest test, the table launch with its first-use
set-up, 0.4 s):
  every layout, copy and accumulating copy; every bias gradient on integer inputs; the workspace form run three times   all equal
  bias gradient on real inputs, largest share of its counted bar (error of bar), all at the shortest chains, where one
  rounding of the sum is most of the bar:
    float32  scalar kernel  atomics 0.56 (2.2e-7 of 3.9e-7, M = 2, N = 255, c = 3)     workspace 0.27 (M = 2, N = 255)
    float32  vector kernel  atomics 0.27 (3.0e-7 of 1.1e-6, M = 3, N = 256, c = 8)     workspace 0.14 (M = 3, N = 256)
    bfloat16 scalar kernel  atomics 0.50 (1.2e-7 of 2.4e-7, M = 1, N = 255, c = 2)     workspace 0.25 (M = 1, N = 255)
    bfloat16 vector kernel  atomics 0.10 (2.4e-7 of 2.4e-6, M = 1, N = 256, c = 10)    workspace 0.08 (M = 1, N = 256)
  every guard byte intact.  No kernel had to be changed.

Tried on a scratch copy, one single-line change at a time, each caught by this file: tile[tx][ty + j * 8] read un-transposed in
prep_weights_kernel (the table and the above-the-cap case, both types); k >> 5 -> k >> 6 in the tile-major index of wt, and the
same in that of w (the table: the shapes with a tiled copy); off = 0 in s2d_weights_kernel (k = 3, 7, 11); rows_per_block rounded
down in bias_grad_impl, M / 1024 with 1 for M < 1024 (M = 1025 and 2049 then need 1025 workgroups: the workspace of exactly
1024 * N floats is refused; the atomics form stays right, which is why the exact-size workspace is part of the case);
`db[n] = t` for `+=` in bias_grad_fold_kernel; `=` for `+=` in unpad_wgrad_kernel and in the scatter of s2d_weights_kernel.
NOT caught, and not catchable: dropping the `rl < rt` guard of bias_grad_fold_kernel's walk.  The threads it lets in (256 % N of
them) read partial rows that exist (r < rows) and leave their sums in sh[rt * N ..], which the fold over r < rt never reads: the
kernel without the guard computes the same numbers.  A grid cap of 511 for 512 in the scalar path passes too, as it must: the cap
is a launch size, not part of the contract, and every sum stays inside the bar counted for 512.

One shape of the issue's table is run in two of its four layout combinations only: (N, RS, Cm, Cp) = (64, 1, 32, 32) with a
tile-major wt.  The header requires Cp % 64 == 0 for it (the engine asks for the same), and prep_weights_kernel would write a
32-row wt into the first half of 64-row blocks, up to element 3071 of a 2048-element buffer.  The two legal combinations of that
shape run, and (64, 1, 64, 64) beside it runs all four.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import layout_cases as LC
from test_gpu_pool_resize_edges import DT, EALIGN, EINVAL, Buf, check_le, chk, st

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = ("f32", "bf16")


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def check_bits(what, buf, ref):
    got = buf.bits()
    ref = np.asarray(ref).reshape(-1)
    assert got.dtype == ref.dtype and got.size == ref.size, what
    bad = got != ref
    assert not bad.any(), "%s: %d of %d elements differ bitwise, the first at %d (%#x, expected %#x)" % (
        what, int(bad.sum()), ref.size, int(np.argmax(bad)), int(got[np.argmax(bad)]), int(ref[np.argmax(bad)]))
    buf.untouched()


def fbuf(a, dtype="f32"):
    """a guarded flat buffer holding the float32 array a bit for bit"""
    a = np.ascontiguousarray(a, F32)
    return Buf(1, a.size, dtype=dtype, data=a.view(np.uint32).reshape(-1) if dtype == "f32" else a.reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------
# dml_prep_weights / dml_prep_weight / dml_unpad_wgrad
# ---------------------------------------------------------------------------------------------------------------------
def prep_table(descs, dtype):
    """(masters, device buffers, ctypes descriptors) of a table"""
    from dmlnet._lib import PrepDesc
    ent = []
    for i, (N, RS, Cm, Cp, has_wt, wtl, wttl) in enumerate(descs):
        master = LC.prep_master(N, RS, Cm, dtype, 10 + i)
        mb = fbuf(master)
        wb = Buf(1, N * RS * Cp, dtype=dtype)
        tb = Buf(1, Cp * RS * N, dtype=dtype) if has_wt else None
        ent.append((master, mb, wb, tb, PrepDesc(mb.ptr, wb.ptr, tb.ptr if tb is not None else None, N, RS, Cm, Cp, wtl, wttl)))
    return ent


def launch_table(lib, ent, dtype):
    from dmlnet._lib import PrepDesc
    arr = (PrepDesc * len(ent))(*[e[4] for e in ent])
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    chk(lib.dml_prep_weights(tab.data_ptr(), len(ent), DT[dtype][0], st()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_weights_heterogeneous_table(lib, dtype):
    """one launch over the whole table: blockIdx.y picks the descriptor; ragged 32 x 32 tiles, 441 tiles on 256 workgroups,
    wt = NULL, a 1 x 1 x 1 weight, the tile-major layouts in every combination the header allows; then every descriptor alone and
    dml_prep_weight on the same shapes give the same bytes"""
    descs = LC.prep_descs()
    ent = prep_table(descs, dtype)
    launch_table(lib, ent, dtype)
    refs = []
    for d, (master, mb, wb, tb, _) in zip(descs, ent):
        N, RS, Cm, Cp, has_wt, wtl, wttl = d
        rw, rwt = LC.prep_ref(master, Cp, dtype, wtl, wttl)
        refs.append((rw, rwt))
        check_bits("prep_weights w %s %s" % (d, dtype), wb, rw)
        if has_wt:
            check_bits("prep_weights wt %s %s" % (d, dtype), tb, rwt)
        mb.untouched()
    for i, d in enumerate(descs):
        N, RS, Cm, Cp, has_wt, wtl, wttl = d
        one = prep_table([d], dtype)
        one[0][1].set(ent[i][0].view(np.uint32).reshape(-1))                      # the same master
        launch_table(lib, one, dtype)
        check_bits("prep_weights alone w %s %s" % (d, dtype), one[0][2], refs[i][0])
        if has_wt:
            check_bits("prep_weights alone wt %s %s" % (d, dtype), one[0][3], refs[i][1])
        if not wtl and not wttl:
            wb, tb = Buf(1, N * RS * Cp, dtype=dtype), (Buf(1, Cp * RS * N, dtype=dtype) if has_wt else None)
            chk(lib.dml_prep_weight(ent[i][1].ptr, wb.ptr, tb.ptr if has_wt else None, N, RS, Cm, Cp, DT[dtype][0], st()))
            check_bits("prep_weight w %s %s" % (d, dtype), wb, refs[i][0])
            if has_wt:
                check_bits("prep_weight wt %s %s" % (d, dtype), tb, refs[i][1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_weight_above_the_grid_cap(lib, dtype):
    """533 520 elements: prep_weight_kernel's grid-stride loop takes a second trip; the table launch agrees"""
    N, RS, Cm, Cp = LC.PREP_BIG
    master = LC.prep_master(N, RS, Cm, dtype, 40)
    rw, rwt = LC.prep_ref(master, Cp, dtype)
    mb, wb, tb = fbuf(master), Buf(1, N * RS * Cp, dtype=dtype), Buf(1, Cp * RS * N, dtype=dtype)
    chk(lib.dml_prep_weight(mb.ptr, wb.ptr, tb.ptr, N, RS, Cm, Cp, DT[dtype][0], st()))
    check_bits("prep_weight big w", wb, rw)
    check_bits("prep_weight big wt", tb, rwt)
    ent = prep_table([(N, RS, Cm, Cp, True, 0, 0)], dtype)
    ent[0][1].set(master.view(np.uint32).reshape(-1))
    launch_table(lib, ent, dtype)
    check_bits("prep_weights big w", ent[0][2], rw)
    check_bits("prep_weights big wt", ent[0][3], rwt)


@pytest.mark.parametrize("case", LC.UNPAD_CASES)
def test_unpad_wgrad_accumulates(lib, case):
    """dst += src without the padding channels, Cm < Cp and Cm == Cp, above the grid cap of 524 288 elements as well"""
    N, RS, Cm, Cp = case
    src, dst0 = LC.values((N, RS, Cp), 50 + N), LC.values((N, RS, Cm), 51 + N)
    sb, db = fbuf(src), fbuf(dst0)
    chk(lib.dml_unpad_wgrad(sb.ptr, db.ptr, N, RS, Cm, Cp, st()))
    check_bits("unpad_wgrad %s" % (case,), db, LC.unpad_ref(src, dst0, Cm).view(np.uint32))
    check_bits("unpad_wgrad source %s" % (case,), sb, src.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# dml_pack_input / dml_pack_input_s2d
# ---------------------------------------------------------------------------------------------------------------------
def run_pack(lib, B, C, Hh, Ww, Cp, dtype):
    x = LC.values((B, C, Hh, Ww), 60 + C + Hh, special=dtype == "f32")
    xb, yb = fbuf(x), Buf(1, B * Hh * Ww * Cp, dtype=dtype)
    chk(lib.dml_pack_input(xb.ptr, yb.ptr, B, C, Hh, Ww, Cp, DT[dtype][0], st()))
    check_bits("pack_input B=%d C=%d %dx%d Cp=%d %s" % (B, C, Hh, Ww, Cp, dtype), yb, LC.pack_input_ref(x, Cp, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_input(lib, dtype):
    for C, Cp in LC.PACK_CCP:
        for B, Hh, Ww in LC.PACK_MAPS:
            run_pack(lib, B, C, Hh, Ww, Cp, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_input_above_the_grid_cap(lib, dtype):
    B, Hh, Ww = LC.PACK_BIG
    run_pack(lib, B, 3, Hh, Ww, 8, dtype)


def run_pack_s2d(lib, B, C, Hh, Ww):
    x = LC.values((B, C, Hh, Ww), 70 + C + Hh, special=True)
    xb, yb = fbuf(x), Buf(1, B * Hh * Ww * C, dtype="f32")
    chk(lib.dml_pack_input_s2d(xb.ptr, yb.ptr, B, C, Hh, Ww, st()))
    check_bits("pack_input_s2d B=%d C=%d %dx%d" % (B, C, Hh, Ww), yb, LC.pack_s2d_ref(x.view(np.uint32)))
    return xb, yb


def test_pack_input_s2d(lib):
    for B, C, Hh, Ww in LC.S2D_PACK:
        xb, yb = run_pack_s2d(lib, B, C, Hh, Ww)
    for Hh, Ww in ((3, 2), (2, 3), (1, 1)):
        assert lib.dml_pack_input_s2d(xb.ptr, yb.ptr, 1, 1, Hh, Ww, st()) == EALIGN
    torch.cuda.synchronize()
    yb.untouched()


def test_pack_input_s2d_above_the_grid_cap(lib):
    run_pack_s2d(lib, *LC.S2D_PACK_BIG)


# ---------------------------------------------------------------------------------------------------------------------
# dml_s2d_weights / dml_s2d_wgrad / dml_gather_taps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", LC.S2D_K)
def test_s2d_weights_and_wgrad(lib, k):
    """the regrouped filter bit for bit (zero taps are +0), and the gradient scatter ADDS into a non-zero dw"""
    k2 = (k + 1) // 2
    for N in LC.S2D_N:
        for C in LC.S2D_C:
            what = "k=%d N=%d C=%d" % (k, N, C)
            w = LC.values((N, k, k, C), 80 + k + N + C, special=True)
            wb, w2b = fbuf(w), Buf(1, N * k2 * k2 * 4 * C, dtype="f32")
            chk(lib.dml_s2d_weights(wb.ptr, w2b.ptr, N, k, C, st()))
            check_bits("s2d_weights " + what, w2b, LC.s2d_weights_ref(w.view(np.uint32)))
            check_bits("s2d_weights source " + what, wb, w.view(np.uint32))
            dw2, dw0 = LC.values((N, k2, k2, 4 * C), 81 + k + N + C), LC.values((N, k, k, C), 82 + k + N + C)
            gb, db = fbuf(dw2), fbuf(dw0)
            chk(lib.dml_s2d_wgrad(gb.ptr, db.ptr, N, k, C, st()))
            check_bits("s2d_wgrad " + what, db, LC.s2d_wgrad_ref(dw2, dw0, k).view(np.uint32))
            check_bits("s2d_wgrad source " + what, gb, dw2.view(np.uint32))


def test_s2d_refusals(lib):
    a, b = Buf(1, 4096, dtype="f32"), Buf(1, 4096, dtype="f32")
    for k in LC.S2D_BAD_K:
        assert lib.dml_s2d_weights(a.ptr, b.ptr, 1, k, 1, st()) == EINVAL
        assert lib.dml_s2d_wgrad(a.ptr, b.ptr, 1, k, 1, st()) == EINVAL
    torch.cuda.synchronize()
    assert bool((a.raw == 0xAA).all()) and bool((b.raw == 0xAA).all()), "a refused call wrote something"


@pytest.mark.parametrize("case", LC.GATHER_CASES + [LC.GATHER_BIG])
def test_gather_taps(lib, case):
    """1 to 4 taps, repeated and descending ones, n = 4, one case above the cap of 1 048 576 float4"""
    rows, taps_src, n, taps = case
    src = LC.values((rows, taps_src, n), 90 + rows, special=True)
    sb, db = fbuf(src), Buf(1, rows * len(taps) * n, dtype="f32")
    t4 = list(taps) + [0] * (4 - len(taps))
    chk(lib.dml_gather_taps(sb.ptr, db.ptr, rows, taps_src, n, len(taps), t4[0], t4[1], t4[2], t4[3], st()))
    check_bits("gather_taps %s" % (case[:3] + (taps,),), db, LC.gather_ref(src.view(np.uint32), taps))


def test_gather_taps_refusals(lib):
    s, d = Buf(1, 1024, dtype="f32"), Buf(1, 1024, dtype="f32")
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 4, 1, 9, 0, 0, 0, st()) == EINVAL          # tap out of range
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 4, 2, 0, -1, 0, 0, st()) == EINVAL
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 4, 5, 0, 0, 0, 0, st()) == EINVAL          # five taps
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 4, 0, 0, 0, 0, 0, st()) == EINVAL
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 6, 1, 0, 0, 0, 0, st()) == EALIGN          # n % 4
    assert lib.dml_gather_taps(s.ptr + 4, d.ptr, 2, 9, 4, 1, 0, 0, 0, 0, st()) == EALIGN
    assert lib.dml_gather_taps(s.ptr, d.ptr + 8, 2, 9, 4, 1, 0, 0, 0, 0, st()) == EALIGN
    assert lib.dml_gather_taps(None, d.ptr, 2, 9, 4, 1, 0, 0, 0, 0, st()) == EINVAL
    # a tap beyond ntaps is not looked at
    assert lib.dml_gather_taps(s.ptr, d.ptr, 2, 9, 4, 1, 0, 99, -5, 1000, st()) == 0
    torch.cuda.synchronize()
    assert bool((s.raw == 0xAA).all()), "a refused call wrote something"
    d.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# dml_bias_grad / dml_bias_grad_ws
# ---------------------------------------------------------------------------------------------------------------------
def run_bias(lib, kind, dtype, M, N, ld=None, off=0, lead=0, ws_rows=None, ws_elems=None, expect=None):
    """one accumulating call on db pre-filled with non-zero values; ws_rows: the workspace form with that many rows of N floats
    (pre-filled with NaN, three runs that must agree bitwise)"""
    ld = ld or N
    kern = expect or LC.bias_kernel(N, ld, dtype)
    dy, db0 = LC.bias_input(kind, M, N, dtype)
    yb = Buf(M, N, ld, off, dtype, dy, lead=lead)
    ref = LC.bias_ref(dy, db0)
    what = "%s %s %s M=%d N=%d ld=%d off=%d lead=%d ws=%s" % (kind, dtype, kern, M, N, ld, off, lead, ws_rows)
    outs = []
    for _ in range(1 if ws_rows is None else 3):
        db = Buf(1, N, dtype="f32", data=db0)
        if ws_rows is None:
            chk(lib.dml_bias_grad(yb.ptr, db.ptr, M, N, ld, DT[dtype][0], st()))
            elems = None
        else:
            elems = ws_rows * N if ws_elems is None else ws_elems
            ws = Buf(1, elems, dtype="f32", data=np.full(elems, np.nan, F32))
            chk(lib.dml_bias_grad_ws(yb.ptr, db.ptr, M, N, ld, DT[dtype][0], ws.ptr, elems, st()))
            ws.untouched()
        db.untouched()
        outs.append(db.bits())
        got = db.get()[0].astype(F64)
        if kind == "exact":
            assert (got == ref).all(), "%s: %d of %d columns differ from the exact sum" % (what, int((got != ref).sum()), N)
        else:
            check_le("bias_grad " + what, np.abs(got - ref), LC.bias_bar(dy, db0, LC.bias_chain(M, N, dtype, kern, elems)))
    for o in outs[1:]:
        assert (o == outs[0]).all(), what + ": the workspace form is not reproducible"
    yb.untouched()
    return outs[0]


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_grad_row_lanes_and_grid_edges(lib, dtype, kind):
    """every N of the table (vector and scalar kernels, idle row lanes at N = 24, N = 1 and 256) with M = 1, rt - 1, rt, rt + 1;
    1023 .. 2049 on the vector kernel (rows per workgroup goes from 1 to 2 at 1025); 512 rt + 1 on the scalar one (the grid cap);
    the atomics form and the workspace form with exactly 1024 * N floats"""
    for N in LC.BIAS_N:
        for M in LC.bias_ms(N, dtype):
            run_bias(lib, kind, dtype, M, N)
            run_bias(lib, kind, dtype, M, N, ws_rows=LC.WS_ROWS)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_grad_slices_and_alignment(lib, dtype, kind):
    """a slice of a wider matrix beside guard columns: ldy a multiple of the vector (vector kernel), an odd ldy (scalar kernel),
    dy one element off (scalar kernel) -- all the same sum"""
    V = LC.vec(dtype)
    for N in (2 * V, 3 * V):
        for M in (77, 1025):
            a = run_bias(lib, kind, dtype, M, N, ld=N + 2 * V, off=V)
            assert LC.bias_kernel(N, N + 2 * V, dtype) == "vec"
            b = run_bias(lib, kind, dtype, M, N, ld=N + 2 * V + 1, off=V, expect="scalar")
            c = run_bias(lib, kind, dtype, M, N, ld=N + 2 * V, off=V + 1, expect="scalar")
            d = run_bias(lib, kind, dtype, M, N, lead=1, expect="scalar")
            e = run_bias(lib, kind, dtype, M, N, ld=N + 2 * V, off=V, ws_rows=LC.WS_ROWS)
            f = run_bias(lib, kind, dtype, M, N, ld=N + 2 * V + 1, off=V, ws_rows=LC.WS_ROWS, expect="scalar")
            g = run_bias(lib, kind, dtype, M, N, lead=1, ws_rows=LC.WS_ROWS, expect="scalar")
            if kind == "exact":
                for o in (b, c, d, e, f, g):
                    assert (o == a).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_grad_workspace_sizes(lib, dtype):
    """a scalar-path workspace with room for 3 workgroups only shrinks the grid and the sum is still right; the vector path with
    too little room, ws_elems < N and ws = NULL are refused and leave db unchanged"""
    V = LC.vec(dtype)
    for kind in ("exact", "real"):
        for N in (13, 1, 255):
            rt = 256 // N
            run_bias(lib, kind, dtype, 40 * rt + 3, N, ws_rows=3 * rt)
            run_bias(lib, kind, dtype, 40 * rt + 3, N, ws_rows=3 * rt, ws_elems=3 * rt * N + N - 1 if N > 1 else 3 * rt)
            run_bias(lib, kind, dtype, 3, N, ws_rows=rt)
    N, M = 2 * V, 1500
    dy, db0 = LC.bias_input("exact", M, N, dtype)
    yb, db = Buf(M, N, dtype=dtype, data=dy), Buf(1, N, dtype="f32", data=db0)
    g, _ = LC.bias_grid(M, N, dtype, "vec")
    ws = Buf(1, 1024 * N, dtype="f32")
    dt = DT[dtype][0]
    assert lib.dml_bias_grad_ws(yb.ptr, db.ptr, M, N, N, dt, ws.ptr, g * N - 1, st()) == EINVAL
    assert lib.dml_bias_grad_ws(yb.ptr, db.ptr, M, N, N, dt, ws.ptr, N - 1, st()) == EINVAL
    assert lib.dml_bias_grad_ws(yb.ptr, db.ptr, M, N, N, dt, None, 1024 * N, st()) == EINVAL
    for fn_args in ((None, db.ptr, M, N), (yb.ptr, None, M, N), (yb.ptr, db.ptr, 0, N), (yb.ptr, db.ptr, M, 0), (yb.ptr, db.ptr, M, 257)):
        assert lib.dml_bias_grad(fn_args[0], fn_args[1], fn_args[2], fn_args[3], N, dt, st()) == EINVAL
    torch.cuda.synchronize()
    assert (db.get()[0] == db0).all(), "a refused call changed db"
    db.untouched()
    assert bool((ws.raw == 0xAA).all()), "a refused call wrote to the workspace"
    chk(lib.dml_bias_grad_ws(yb.ptr, db.ptr, M, N, N, dt, ws.ptr, g * N, st()))     # exactly enough
    assert (db.get()[0].astype(F64) == LC.bias_ref(dy, db0)).all()
    db.untouched(), ws.untouched()
