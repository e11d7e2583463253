"""CPU: the numpy definitions of tests/layout_cases.py are right -- the tile-major layout is the header's wording element by
element, the space-to-depth regrouping of image and filter gives the stride-2 convolution (float64, small integers: exactly), the
weight-gradient scatter is its adjoint -- and the bias-gradient bars hold for plain float32 evaluations in the kernels' orders."""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import layout_cases as LC

F32, F64 = np.float32, np.float64


def test_tile_major_is_the_headers_layout():
    """[rows][K] stored as [rows / 64][K / 32][64][32]: element (r, k) sits in block (r / 64, k / 32) at row r % 64, column k % 32"""
    rows, K = 128, 96
    m = np.arange(rows * K, dtype=np.int64).reshape(rows, K)
    t = LC.tile_major(m).reshape(rows // 64, K // 32, 64, 32)
    for r in range(rows):
        for k in range(K):
            assert t[r // 64, k // 32, r % 64, k % 32] == m[r, k]
    assert sorted(LC.tile_major(m).tolist()) == list(range(rows * K))


def test_prep_reference_pads_transposes_and_rounds_once():
    master = LC.prep_master(5, 3, 6, "f32", 1)
    w, wt = LC.prep_ref(master, 8, "f32")
    w, wt = w.reshape(5, 3, 8), wt.reshape(8, 3, 5)
    mb = master.view(np.uint32)
    for n in range(5):
        for rs in range(3):
            for c in range(8):
                want = mb[n, rs, c] if c < 6 else 0             # padding: +0
                assert w[n, rs, c] == want and wt[c, rs, n] == want
    assert set(LC.SPECIAL_BITS.tolist()) <= set(w.reshape(-1).tolist())          # the specials survive as bits
    m2 = LC.prep_master(4, 2, 3, "bf16", 2)
    wb, _ = LC.prep_ref(m2, 3, "bf16")
    back = (wb.astype(np.uint32) << 16).view(F32).astype(F64).reshape(m2.shape)
    ulp = 2.0 ** (np.floor(np.log2(np.abs(m2.astype(F64)))) - 7)
    assert (np.abs(back - m2) <= ulp / 2).all()                                   # nearest
    tie = np.array([[[1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]]], F32)                # ties go to the even bfloat16
    tb, _ = LC.prep_ref(tie, 2, "bf16")
    assert tb.tolist() == [0x3F80, 0x3F82]
    for N, RS, Cm, Cp, has_wt, wtl, wttl in LC.prep_descs():
        okw, okt = LC.tiled_ok(N, RS, Cp)
        assert (okw or not wtl) and (okt or not wttl)
    assert any(d[5] and d[6] for d in LC.prep_descs()) and any(d[5] and not d[6] for d in LC.prep_descs())
    assert any(d[6] and not d[5] for d in LC.prep_descs())
    N, RS, _, Cp = LC.PREP_TABLE[4][:4]
    assert ((N + 31) // 32) * ((Cp + 31) // 32) * RS == 441 > 256
    assert np.prod(LC.PREP_BIG[:2]) * LC.PREP_BIG[3] > LC.CAP_2048
    assert any(n * rs * cm > LC.CAP_2048 and cm < cp for n, rs, cm, cp in LC.UNPAD_CASES)
    assert any(n * rs * cm > LC.CAP_2048 and cm == cp for n, rs, cm, cp in LC.UNPAD_CASES)


def test_pack_input_reference():
    x = LC.values((2, 3, 5, 7), 3, special=True)
    y = LC.pack_input_ref(x, 8, "f32").reshape(2, 5, 7, 8)
    xb = x.view(np.uint32)
    for b in range(2):
        for c in range(8):
            for h in range(5):
                for w in range(7):
                    assert y[b, h, w, c] == (xb[b, c, h, w] if c < 3 else 0)
    B, Hh, Ww = LC.PACK_BIG
    assert B * Hh * Ww > LC.CAP_4096
    B, _, Hh, Ww = LC.S2D_PACK_BIG
    assert B * (Hh // 2) * (Ww // 2) > LC.CAP_4096
    rows, _, n, taps = LC.GATHER_BIG
    assert rows * len(taps) * (n // 4) > LC.CAP_4096


def test_pack_s2d_reference_is_the_headers_channel_order():
    x = np.arange(2 * 3 * 6 * 4, dtype=F32).reshape(2, 3, 6, 4)
    x2 = LC.pack_s2d_ref(x)
    assert x2.shape == (2, 3, 2, 12)
    for b in range(2):
        for y2 in range(3):
            for xx in range(2):
                for dy in range(2):
                    for dx in range(2):
                        for c in range(3):
                            assert x2[b, y2, xx, (dy * 2 + dx) * 3 + c] == x[b, c, 2 * y2 + dy, 2 * xx + dx]


@pytest.mark.parametrize("k", LC.S2D_K)
def test_space_to_depth_is_the_stride_2_convolution(k):
    """conv2d(x, w, stride 2, padding p) == conv2d(x2, w2, stride 1, padding (p + 1) / 2) on its H/2 x W/2 outputs (the regrouped
    filter's zero taps reach one row and column further: that extra output row and column is not part of the contract), in
    float64 on small integers: exactly"""
    p = (k - 1) // 2
    for N in LC.S2D_N:
        for C in LC.S2D_C:
            for B, Hh, Ww in ((2, 6, 4), (1, 2, 2), (1, 14, 26)):
                x = LC.ints((B, C, Hh, Ww), k + N + C)
                w = LC.ints((N, k, k, C), k * N + C)
                y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double().permute(0, 3, 1, 2), stride=2, padding=p)
                x2, w2 = LC.pack_s2d_ref(x), LC.s2d_weights_ref(w)
                assert w2.shape == (N, (k + 1) // 2, (k + 1) // 2, 4 * C)
                y2 = torch.nn.functional.conv2d(torch.from_numpy(x2).double().permute(0, 3, 1, 2), torch.from_numpy(w2).double().permute(0, 3, 1, 2),
                                                stride=1, padding=(p + 1) // 2)
                assert tuple(y.shape) == (B, N, Hh // 2, Ww // 2)
                assert torch.equal(y, y2[:, :, :Hh // 2, :Ww // 2])
                assert y.abs().sum() > 0 or Hh == 2
                # the adjoint: sum(w2(w) g2) == sum(w scatter(g2)), and scatter o gather is the identity on w
                g2 = LC.ints(w2.shape, 9 + k + N + C)
                assert (w2.astype(F64) * g2).sum() == (w.astype(F64) * LC.s2d_scatter(g2, k)).sum()
                assert np.array_equal(LC.s2d_scatter(w2, k), w)
                assert (w2 == 0).sum() >= w2.size - w.size


def test_gather_reference():
    src = np.arange(3 * 9 * 4).reshape(3, 9, 4)
    d = LC.gather_ref(src, (7, 7, 2))
    for r in range(3):
        for j, t in enumerate((7, 7, 2)):
            assert (d[r, j] == src[r, t]).all()


def f32_sum_in_order(rows, N):
    """float32 sum of the rows [n, N] in order, all columns at once"""
    acc = np.zeros(N, F32)
    for t in rows:
        acc = (acc + t.astype(F32)).astype(F32)
    return acc


def emulate_bias(dy, db0, N, dtype, kern, ws_rows=None):
    """float32 evaluation in the kernels' orders (the atomics in launch order)"""
    M = dy.shape[0]
    g, rows = LC.bias_grid(M, N, dtype, kern, None if ws_rows is None else ws_rows * N)
    parts = np.zeros((rows, N), F32)
    if kern == "vec":
        rt = LC.bias_rt(N, dtype, kern)
        rpb = LC.ceil_div(M, 1024)
        for b in range(g):
            blk = dy[b * rpb:min(M, (b + 1) * rpb)]
            parts[b] = f32_sum_in_order([f32_sum_in_order(blk[r::rt], N) for r in range(rt)], N)
    else:
        for r in range(rows):
            parts[r] = f32_sum_in_order(dy[r::rows], N)
    if ws_rows is None:
        acc = np.asarray(db0, F32)
        for r in range(rows):
            acc = (acc + parts[r]).astype(F32)
        return acc
    rf = 256 // N
    return (np.asarray(db0, F32) + f32_sum_in_order([f32_sum_in_order(parts[l::rf], N) for l in range(rf)], N)).astype(F32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bias_gradient_cases_and_bars(dtype):
    """every N has its M around the row lanes; the kernels named in the case table are the ones the entry point picks; float32
    evaluations in the kernels' orders equal the float64 sum on the exact inputs and stay inside the counted bar on the real ones"""
    V = LC.vec(dtype)
    for N in LC.BIAS_N:
        kern = LC.bias_kernel(N, N, dtype)
        assert kern == ("vec" if N % V == 0 else "scalar")
        rt = LC.bias_rt(N, dtype, kern)
        ms = LC.bias_ms(N, dtype)
        assert {m for m in (1, rt - 1, rt, rt + 1) if m >= 1} <= set(ms)
        assert (set(LC.BIAS_VEC_M) <= set(ms)) if kern == "vec" else (max(ms) > 512 * rt)
    assert LC.bias_kernel(12, 12, "f32") == "vec" and LC.bias_kernel(12, 12, "bf16") == "scalar"
    assert LC.bias_kernel(8, 24, dtype, aligned=False) == "scalar" and LC.bias_kernel(8, 27, dtype) == "scalar"
    assert 256 % (24 // V) != 0                                                    # N = 24 leaves idle row lanes
    assert LC.bias_grid(1024, 16, dtype, "vec")[0] == 1024 and LC.bias_grid(1025, 16, dtype, "vec")[0] == 513
    assert LC.bias_grid(2049, 16, dtype, "vec")[0] == 683
    assert LC.bias_grid(10 ** 6, 13, dtype, "scalar") == (512, 512 * 19)
    assert LC.bias_grid(10 ** 6, 13, dtype, "scalar", 3 * 19 * 13 + 5) == (3, 57)
    for N, M in ((13, 40), (24, 85 if dtype == "bf16" else 43), (16, 1025), (1, 300), (256, 5)):
        kern = LC.bias_kernel(N, N, dtype)
        for ws_rows in (None, LC.WS_ROWS):
            for kind in ("exact", "real"):
                dy, db0 = LC.bias_input(kind, M, N, dtype)
                got = emulate_bias(dy, db0, N, dtype, kern, ws_rows).astype(F64)
                ref = LC.bias_ref(dy, db0)
                if kind == "exact":
                    assert (got == ref).all() and (np.abs(ref) < 2 ** 24).all()
                else:
                    c = LC.bias_chain(M, N, dtype, kern, None if ws_rows is None else ws_rows * N)
                    assert (np.abs(got - ref) <= LC.bias_bar(dy, db0, c)).all()
    for N in LC.BIAS_N:                                                             # the exact inputs stay below 2^24 everywhere
        for M in LC.bias_ms(N, dtype):
            assert 3 * M + 17 < 2 ** 24
