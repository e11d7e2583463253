"""CPU: the float64 definitions, input generators and error bars of tests/pool_cases.py are right on exactly the inputs
tests/test_gpu_pool_resize_edges.py uses -- so that a failure there is the kernel's.

  * the definitions equal float64 F.max_pool2d(return_indices=True) and its autograd gradient (ties, -inf windows and the NaN
    included), F.interpolate with autograd, F.adaptive_avg_pool2d, torch.optim.SGD, and Tensor.to(torch.bfloat16) bit for bit;
  * the exact cases are exact: every intermediate of the contract is a float32 value (and the float32 source coordinates of the
    dyadic resizes are the float64 ones);
  * a plain float32 evaluation of each formula, contracted (FMA) and not, summed in sequence and pairwise, stays inside its bar
    on every real-valued case;
  * every tie-heavy max pool case has at least 40 % of its windows tied, the ReLU data at least 40 % zeros;
  * every "above the cap" case exceeds grid_for's cap times 256 of the kernel it is meant for.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as PC

F32, F64 = np.float32, np.float64
DTYPES = ("f32", "bf16")


def is32(x):
    x = np.asarray(x, F64)
    return bool((x.astype(F32).astype(F64) == x).all())


def fma32(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact, the sum is rounded once"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


def nchw(a, grad=False):
    return t64(np.asarray(a, F64).transpose(0, 3, 1, 2), grad)


def nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def inside(got, ref, bar, what):
    err = np.abs(np.asarray(got, F64) - ref)
    assert np.isfinite(err).all() and (err <= bar).all(), "%s: %.3e above %.3e" % (what, (err - bar).max(), bar.flat[np.argmax(err - bar)])


# ---------------------------------------------------------------------------------------------------------------------
# definitions against torch, float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", PC.MAXPOOL_KINDS)
def test_maxpool_definitions_equal_float64_torch(kind, dtype):
    for B, H, W, C in PC.maxpool_cases(dtype):
        x = PC.maxpool_input(kind, B, H, W, C, dtype)
        y, tap = PC.maxpool_fwd(x)
        xt = nchw(x, True)
        yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
        assert PC.same(y, nhwc(yt)).all(), (kind, B, H, W, C)
        # torch's flat index into the H x W image -> tap r * 3 + s of its window
        idx = it.numpy().transpose(0, 2, 3, 1)
        yo, xo = np.arange(y.shape[1])[None, :, None, None], np.arange(y.shape[2])[None, None, :, None]
        assert (tap == (idx // W - (2 * yo - 1)) * 3 + (idx % W - (2 * xo - 1))).all(), (kind, B, H, W, C)
        g = PC.maxpool_grad(B, H, W, C)
        yt.backward(nchw(g))
        assert (PC.maxpool_bwd(g, tap, H, W) == nhwc(xt.grad)).all(), (kind, B, H, W, C)
        if kind == "special":
            assert np.isinf(y[0, :, :, 0]).all() and np.isnan(y[B - 1, :, :, 1]).any() and (y[0, 0, 0, 2] == -np.inf)
            assert tap[0, 0, 0, 0] == 4 and tap[0, 0, 0, 2] == 4          # the first in-bounds tap of the corner window: r = s = 1


@pytest.mark.parametrize("geom", PC.BILINEAR_GEOMS + [PC.BILINEAR_BIG_BWD[1:5]])
def test_bilinear_definitions_equal_float64_torch(geom):
    h, w, H, W = geom
    for C in (4, 24):
        x = PC.bilinear_input((PC.BILINEAR_B, h, w, C), geom in PC.BILINEAR_EXACT, "f32")
        g = PC.bilinear_input((PC.BILINEAR_B, H, W, C), geom in PC.BILINEAR_EXACT, "f32", seed=1)
        xt = nchw(x, True)
        yt = F.interpolate(xt, size=(H, W), mode="bilinear", align_corners=False)
        yt.backward(nchw(g))
        y, dx = PC.bilinear_fwd(x, H, W), PC.bilinear_bwd(g, h, w)
        assert (np.abs(y - nhwc(yt)) <= 1e-13 * np.abs(x).max()).all()
        assert (np.abs(dx - nhwc(xt.grad)) <= 1e-12 * np.abs(g).max()).all()
        # the gather form and the matrix form are the same operator
        assert (np.abs(y - PC._sep(PC.lerp_matrix(H, h), PC.lerp_matrix(W, w), x.astype(F64), False)) <= 1e-13 * np.abs(x).max()).all()


@pytest.mark.parametrize("case", PC.ADAPTIVE_CASES)
def test_adaptive_avgpool_definition_equals_float64_torch(case):
    B, H, W, C, _ = case
    x = PC.adaptive_input(B, H, W, C, "f32")
    for S in PC.ADAPTIVE_S:
        y, mag, cnt = PC.adaptive_avgpool(x, S)
        ref = nhwc(F.adaptive_avg_pool2d(nchw(x), S))
        assert (np.abs(y - ref) <= 1e-13 * mag / cnt[None, :, :, None] + 1e-300).all()
    assert PC.bins(53, 3) == [(0, 18), (17, 36), (35, 53)] and PC.bins(11, 2) == [(0, 6), (5, 11)]


def test_upsample_definition_equals_float64_torch():
    for kind in PC.UPSAMPLE_KINDS:
        for W in PC.UPSAMPLE_W:
            src, dst0, H, alpha = PC.upsample_input(kind, W)
            ref = float(F32(alpha)) * F.interpolate(nchw(src), size=(H, W), mode="bilinear", align_corners=False).numpy()
            assert (np.abs(PC.upsample_nchw(src, H, W, alpha) - ref) <= 1e-13).all()
            assert (np.abs(PC.upsample_nchw(src, H, W, alpha, dst0) - (ref + dst0)) <= 1e-13).all()


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_sgd_definition_equals_float64_torch_optim(kind):
    for lr, mu, wd, gs in (PC.SGD_EXACT if kind == "exact" else PC.SGD_REAL):
        lr, mu, wd, gs = (float(F32(a)) for a in (lr, mu, wd, gs))
        p0, v0, gs_ = PC.sgd_input(kind, 1027)
        pt = torch.nn.Parameter(t64(p0))
        opt = torch.optim.SGD([pt], lr=lr, momentum=mu, weight_decay=wd)
        opt.state[pt]["momentum_buffer"] = t64(v0)
        p, v = p0.astype(F64), v0.astype(F64)
        for g in gs_:
            pt.grad = t64(g) * gs
            opt.step()
            p, v, _, _ = PC.sgd_step(p, g, v, lr, mu, wd, gs)
            assert (np.abs(p - pt.detach().numpy()) <= 1e-14 * (1 + np.abs(p))).all()
            if mu != 0:
                assert (np.abs(v - opt.state[pt]["momentum_buffer"].numpy()) <= 1e-14 * (1 + np.abs(v))).all()


def test_conversion_equals_torch_bit_for_bit():
    for n in PC.FILL_NS:
        bits = PC.convert_input(n, "f32")
        x = torch.from_numpy(bits.view(F32).copy())
        ref = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = PC.convert_ref(bits, "f32", "bf16")
        assert PC.bits_same(got, ref, "bf16").all()
        assert (np.isnan(PC.from_bf16_bits(got)) == np.isnan(bits.view(F32))).all()
        b16 = PC.convert_input(n, "bf16")
        back = torch.from_numpy(b16.view(np.int16).copy()).view(torch.bfloat16).float().numpy().view(np.uint32)
        assert PC.bits_same(PC.convert_ref(b16, "bf16", "f32"), back, "f32").all()
    # what the special patterns must become
    sp = PC.to_bf16_bits(PC.SPECIAL_BITS.view(F32))
    want = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F82, 0x3F81, 0x7F7F, 0x7F7F, 0x7F80, 0x7F80, 0xFF80, 0xFF7F,
            0x0000, 0x0000, 0x0002, 0x0080, 0x8000, 0x8002, 0x0000, 0x8000, 0x7F80, 0xFF80]
    assert sp[:len(want)].tolist() == want
    assert np.isnan(PC.from_bf16_bits(sp[len(want):])).all()
    # bn_cases.store agrees on the finite ones
    fin = np.isfinite(PC.SPECIAL_BITS.view(F32))
    assert (PC.bf16_round(PC.SPECIAL_BITS.view(F32)[fin]).view(np.uint32) >> 16 == sp[fin]).all()
    # every block of a long array carries the special patterns: also beyond the first trip of the grid-stride loop
    big = PC.convert_input(PC.BIG_N, "f32")
    assert (big[-len(PC.SPECIAL_BITS):] == PC.SPECIAL_BITS).all() and (big[PC.CAP_2048:PC.CAP_2048 + 5] == PC.SPECIAL_BITS[:5]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the exact cases are exact
# ---------------------------------------------------------------------------------------------------------------------
def on_grid(terms, k, what):
    """every term a multiple of 2^-k and the sum of their magnitudes below 2^(24 - k): every partial sum, in any order, with or
    without contraction, is then a float32 value"""
    t = np.asarray(terms, F64) * 2.0 ** k
    assert (t == np.rint(t)).all(), what + ": not on the 2^-%d grid" % k
    assert np.abs(t).sum(0).max() < 2.0 ** 24, what + ": a partial sum can leave float32"


def test_exact_maxpool_gradients_and_sums_are_exact():
    for dtype in DTYPES:
        for B, H, W, C in PC.maxpool_cases(dtype):
            g = PC.maxpool_grad(B, H, W, C)
            assert (PC.bf16_round(g.astype(F32)) == g).all()
            on_grid(np.stack([g] * 4), 2, "max pool gradient")               # at most four windows meet in a pixel
        for HW in PC.RED_HW:
            for cv in PC.RED_CV:
                C = cv * PC.vec(dtype)
                x = PC.reduce_input("exact", PC.RED_B, HW, C, dtype)
                assert (PC.bf16_round(x) == x).all()
                on_grid(x.transpose(1, 0, 2), 0, "sum over HW")
                s = PC.sum_hw(x)
                if HW >= 2:
                    assert (s[:, 0] == 257).all() and (PC.store(s, "bf16")[:, 0] != 257).all()
                if PC.pow2(HW):
                    assert is32(s * float(F32(1) / F32(HW))) and float(F32(1) / F32(HW)) == 1.0 / HW
        for B, HW, C in [(PC.RED_B, 1, 9 * PC.vec(dtype)), (PC.BC_BIG[0], PC.BC_BIG[1], PC.BC_BIG[2] * PC.vec(dtype))]:
            v, dx0 = PC.broadcast_input("exact", B, HW, C, dtype)
            assert PC.pow2(HW) and is32(v.astype(F64) / HW) and is32(PC.avgpool_bwd(v, HW, dx0))
            assert (PC.bf16_round(v) == v).all() and (PC.bf16_round(dx0) == dx0).all()


def src_index32(out, inn, fma):
    """the kernels' float32 source index: scale = (float) in / (float) out"""
    sc = F32(inn) / F32(out)
    d = np.arange(out, dtype=F32) + F32(0.5)
    s = fma32(sc, d, -0.5) if fma else sc * d - F32(0.5)
    s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = s - i0.astype(F32)
    return i0, i1, F32(1) - l1, l1, s


@pytest.mark.parametrize("geom", PC.BILINEAR_EXACT + [PC.BILINEAR_BIG_BWD[1:5], (512, 1368, 1024, 2736), (2, 7, 4, 7)])
def test_exact_resizes_are_exact(geom):
    h, w, H, W = geom
    for out, inn in ((H, h), (W, w)):
        ref = PC.src_index(out, inn)
        for fma in (False, True):
            got = src_index32(out, inn, fma)
            assert all((np.asarray(a, F64) == b).all() for a, b in zip(got, ref)), "float32 source index differs"
        t = ref[2] * 8
        assert (t == np.rint(t)).all()                                     # weights are multiples of 1/8
    Wy, Wx = PC.lerp_matrix(H, h), PC.lerp_matrix(W, w)
    # every weight product is a multiple of 1/64; data: multiples of 1/4 of magnitude <= 8, times alpha = 1/2 in the NCHW
    # upsample: terms on the 2^-9 grid, and the magnitudes a destination (a source, in the transpose) sums stay below 2^15
    for M in (Wy, Wx):
        assert (M * 8 == np.rint(M * 8)).all() and (M >= 0).all() and np.abs(M.sum(1) - 1).max() == 0
    assert 8.0 * 2.0 ** 9 * Wy.sum(0).max() * Wx.sum(0).max() < 2.0 ** 24
    x = PC.bilinear_input((1, h, w, 4), True, "bf16")
    assert np.abs(x).max() <= 8 and (x * 4 == np.rint(x * 4)).all()


def test_exact_sgd_steps_are_exact():
    for lr, mu, wd, gs in PC.SGD_EXACT:
        p, v, gs_ = PC.sgd_input("exact", 1027)
        p, v = p.astype(F64), v.astype(F64)
        for g in gs_:
            terms = [mu * v, gs * g, wd * p, gs * g + wd * p]
            p0 = p
            p, v, _, _ = PC.sgd_step(p, g, v, lr, mu, wd, gs)
            assert all(is32(t) for t in terms) and is32(v) and is32(lr * v) and is32(p)
            on_grid(np.stack(terms[:3] + [p0, lr * v]), 12, "SGD terms")       # ... so that contraction cannot change a sum


# ---------------------------------------------------------------------------------------------------------------------
# plain float32 evaluations stay inside the bars
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_float32_sums_inside_their_bars(dtype):
    V = PC.vec(dtype)
    for HW in PC.RED_HW:
        for cv in PC.RED_CV:
            x = PC.reduce_input("real", PC.RED_B, HW, cv * V, dtype)
            for scale in (1.0, float(F32(1) / F32(HW))):
                ref, bar = PC.sum_hw(x, scale), PC.sum_bar(x, scale, True)
                for s in (x.cumsum(1, dtype=F32)[:, -1], x.sum(1, dtype=F32), x[:, ::-1].cumsum(1, dtype=F32)[:, -1]):
                    inside(s * F32(scale), ref, bar, "sum HW=%d" % HW)
            if HW > 1:
                assert np.abs(x[:, :, 0].mean(1)).min() > 5e3 * x[:, :, 0].astype(F64).std(1).max() or dtype == "bf16"
    for HW in PC.BC_HW:
        v, dx0 = PC.broadcast_input("real", PC.RED_B, HW, 9 * V, dtype)
        a = F32(1) / F32(HW)
        inside((v * a)[:, None, :] + np.zeros_like(dx0), PC.avgpool_bwd(v, HW), PC.avgpool_bwd_bar(v, HW), "avgpool set")
        for got in ((v * a)[:, None, :] + dx0, fma32(v[:, None, :], a, dx0)):
            inside(got, PC.avgpool_bwd(v, HW, dx0), PC.avgpool_bwd_bar(v, HW, dx0), "avgpool add")


def fwd32(x, H, W, fma):
    x = np.asarray(x, F32)
    _, h, w, _ = x.shape
    y0, y1, ly0, ly1, _ = src_index32(H, h, fma)
    x0, x1, lx0, lx1, _ = src_index32(W, w, fma)
    a0, a1 = lx0[None, None, :, None], lx1[None, None, :, None]
    b0, b1 = ly0[None, :, None, None], ly1[None, :, None, None]
    r0, r1 = x[:, y0], x[:, y1]
    if fma:
        i0, i1 = fma32(a1, r0[:, :, x1], a0 * r0[:, :, x0]), fma32(a1, r1[:, :, x1], a0 * r1[:, :, x0])
        return fma32(b1, i1, b0 * i0)
    return b0 * (a0 * r0[:, :, x0] + a1 * r0[:, :, x1]) + b1 * (a0 * r1[:, :, x0] + a1 * r1[:, :, x1])


def wmat32(out, inn, fma):
    i0, i1, l0, l1, _ = src_index32(out, inn, fma)
    src = np.arange(inn)[None, :]
    return np.where(i0[:, None] == src, l0[:, None], F32(0)) + np.where(i1[:, None] == src, l1[:, None], F32(0))


def bwd32(g, h, w, fma):
    """the gather of bilinear_bwd_kernel: per source pixel the destination pixels in row-major order, acc += (wy wx) g"""
    g = np.asarray(g, F32)
    B, H, W, C = g.shape
    Wy, Wx = wmat32(H, h, fma), wmat32(W, w, fma)
    ys, xs = np.argmax(Wy != 0, 0), np.argmax(Wx != 0, 0)
    acc = np.zeros((B, h, w, C), F32)
    for a in range(int((Wy != 0).sum(0).max())):
        Y = np.minimum(ys + a, H - 1)
        wy = np.where(ys + a < H, Wy[Y, np.arange(h)], F32(0))
        for b in range(int((Wx != 0).sum(0).max())):
            X = np.minimum(xs + b, W - 1)
            wx = np.where(xs + b < W, Wx[X, np.arange(w)], F32(0))
            ww = (wy[:, None] * wx[None, :])[None, :, :, None]
            gs = g[:, Y][:, :, X]
            acc = fma32(ww, gs, acc) if fma else acc + ww * gs
    return acc


@pytest.mark.parametrize("geom", [g for g in PC.BILINEAR_GEOMS if g not in PC.BILINEAR_EXACT])
def test_float32_resizes_inside_their_bars(geom):
    h, w, H, W = geom
    for dtype in DTYPES:
        for C in PC.BILINEAR_C:
            x = PC.bilinear_input((PC.BILINEAR_B, h, w, C), False, dtype)
            g = PC.bilinear_input((PC.BILINEAR_B, H, W, C), False, dtype, seed=1)
            y, ybar = PC.bilinear_fwd(x, H, W), PC.bilinear_bar(x, h, w, H, W, False)
            dx, dbar = PC.bilinear_bwd(g, h, w), PC.bilinear_bar(g, h, w, H, W, True)
            for fma in (False, True):
                inside(fwd32(x, H, W, fma), y, ybar, "forward %s" % (geom,))
                inside(bwd32(g, h, w, fma), dx, dbar, "transpose %s" % (geom,))
            # the bars are no licence: a few float32 units of the magnitudes that enter
            mag = PC._sep(PC.lerp_matrix(H, h), PC.lerp_matrix(W, w), np.abs(x.astype(F64)), False)
            assert (ybar <= 8 * max(h, w) * PC.EPS32 * np.abs(x).max() * 4).all() and (ybar >= 5 * PC.EPS32 * mag).all()


def test_float32_big_forward_resize_inside_its_bar():
    B, h, w, H, W, C = PC.BILINEAR_BIG_FWD
    x = PC.bilinear_input((B, h, w, C), False, "f32")
    inside(fwd32(x, H, W, False), PC.bilinear_fwd(x, H, W), PC.bilinear_bar(x, h, w, H, W, False), "big forward")


def test_float32_upsample_inside_its_bar():
    for W in PC.UPSAMPLE_W:
        src, dst0, H, alpha = PC.upsample_input("real", W)
        a = F32(alpha)
        val = fwd32(src, H, W, False).transpose(0, 3, 1, 2)
        inside(a * val, PC.upsample_nchw(src, H, W, alpha), PC.upsample_bar(src, H, W, alpha), "upsample set")
        for got in (dst0 + a * val, fma32(a, fwd32(src, H, W, True).transpose(0, 3, 1, 2), dst0)):
            inside(got, PC.upsample_nchw(src, H, W, alpha, dst0), PC.upsample_bar(src, H, W, alpha, dst0), "upsample add")


@pytest.mark.parametrize("case", PC.ADAPTIVE_CASES)
def test_float32_adaptive_avgpool_inside_its_bar(case):
    B, H, W, C, _ = case
    for dtype in DTYPES:
        x = PC.adaptive_input(B, H, W, C, dtype)
        for S in PC.ADAPTIVE_S:
            y, mag, cnt = PC.adaptive_avgpool(x, S)
            bar = PC.adaptive_bar(mag, cnt)
            for i, (y0, y1) in enumerate(PC.bins(H, S)):
                for j, (x0, x1) in enumerate(PC.bins(W, S)):
                    blk = x[:, y0:y1, x0:x1].reshape(B, -1, C)
                    for s in (blk.cumsum(1, dtype=F32)[:, -1], blk.sum(1, dtype=F32)):
                        inside(s / F32(cnt[i, j]), y[:, i, j], bar[:, i, j], "adaptive pool S=%d" % S)


def test_float32_sgd_inside_its_bars():
    for lr, mu, wd, gs in PC.SGD_REAL:
        p, v, gs_ = PC.sgd_input("real", 1027)
        lr32, mu32, wd32, gs32 = (F32(a) for a in (lr, mu, wd, gs))
        for fma in (False, True):
            pp, vv = p.copy(), v.copy()
            for g in gs_:
                rp, rv, bp, bv = PC.sgd_step(pp, g, vv, lr, mu, wd, gs)
                if fma:
                    nv = fma32(mu32, vv, fma32(wd32, pp, gs32 * g))
                    np_ = fma32(-lr32, nv, pp)
                else:
                    nv = mu32 * vv + (gs32 * g + wd32 * pp)
                    np_ = pp - lr32 * nv
                # p's reference takes the float32 v the evaluation itself stored, as the GPU test does
                inside(nv, rv, bv, "v")
                inside(np_, pp.astype(F64) - float(lr32) * nv.astype(F64), 3 * PC.EPS32 * (np.abs(pp) + np.abs(float(lr32) * nv)), "p from its own v")
                inside(np_, rp, bp, "p")
                pp, vv = np_, nv


# ---------------------------------------------------------------------------------------------------------------------
# the inputs are what they are meant to be
# ---------------------------------------------------------------------------------------------------------------------
def test_tie_heavy_maxpool_cases_are_tie_heavy():
    for dtype in DTYPES:
        for B, H, W, C in PC.maxpool_cases(dtype):
            x = PC.maxpool_input("relu", B, H, W, C, dtype)
            assert (x == 0).mean() >= 0.4, (B, H, W, C)
            for kind in PC.TIE_HEAVY:
                if H * W > 1:                                              # a window of one tap cannot tie
                    share = PC.tied_share(PC.maxpool_input(kind, B, H, W, C, dtype))
                    assert share >= 0.4, (kind, B, H, W, C, share)
            assert PC.tied_share(PC.maxpool_input("gauss", B, H, W, C, dtype)) <= (0.0 if dtype == "f32" else 0.2)
    assert (PC.window_taps(7, 9) == np.outer([2, 3, 3, 2], [2, 3, 3, 3, 2])).all()
    assert (PC.window_taps(4, 2) == [[4], [6]]).all()


def test_above_the_cap_cases_exceed_the_cap():
    # grid_for(..., 256) defaults to 2048 workgroups: sgd_kernel (n / 4 + 4 items), fill_kernel, convert_kernel,
    # broadcast_hw_kernel (vector items), adaptive_pool_finish_kernel (bins * C)
    assert PC.CAP_2048 == 524288
    assert PC.SGD_NS[-1] // 4 > 524288 and PC.SGD_NS[-1] % 4 == 3 and PC.SGD_NS[-1] // 4 - 524288 == 300
    assert PC.FILL_NS[-1] > 524288
    B, HW, cv = PC.BC_BIG
    assert B * HW * cv == 532480 > 524288
    assert max(B * S * S * C for (B, H, W, C, _) in PC.ADAPTIVE_CASES for S in PC.ADAPTIVE_S if S <= min(H, W)) == 589824 > 524288
    # grid_for(items, 256, 256 * 16) = 4096 workgroups: bilinear_fwd_kernel / bilinear_bwd_kernel, four channels per item
    assert PC.CAP_4096 == 1048576
    B, h, w, H, W, C = PC.BILINEAR_BIG_FWD
    assert B * H * W * (C // 4) == 1065024 > 1048576
    B, h, w, H, W, C = PC.BILINEAR_BIG_BWD
    assert B * h * w * (C // 4) == 1052672 > 1048576
    # grid_for(items, 256, 256 * 32) = 8192 workgroups: upsample_to_nchw_kernel, four destination pixels of a row per item
    assert PC.CAP_8192 == 2097152
    B, h, w, C, H, W = PC.UPSAMPLE_BIG
    assert B * C * H * ((W + 3) // 4) == 2101248 > 2097152
    # every row of 53 at S = 3 has more than the 16 row slices, and 53 is no multiple of 3
    assert all(y1 - y0 > 16 for y0, y1 in PC.bins(53, 3)) and 53 % 3


def test_bilinear_bwd_window_encloses_every_contributing_row():
    """the gather window of the bilinear_bwd kernels, Y0 = floor((ys - 0.5) / s - 0.5) - 1 .. Y1 = ceil((ys + 1.5) / s - 0.5) + 1 in
    float32, holds every destination row that reads source row ys -- at the geometries of the table, enlarging, identity, shrinking
    and an extent of 1; it does so without its margin of one row too (the margin is slack, so no test can tell it is there)"""
    pairs = {(o, i) for h, w, Hh, Ww in PC.BILINEAR_GEOMS + [PC.BILINEAR_BIG_BWD[1:5]] for o, i in ((Hh, h), (Ww, w))}
    for out, inn in sorted(pairs):
        i0, i1, l0, l1, _ = src_index32(out, inn, False)
        sc = F32(inn) / F32(out)
        ys = np.arange(inn)
        Wm = np.where(i0[:, None] == ys, l0[:, None], F32(0)) + np.where(i1[:, None] == ys, l1[:, None], F32(0))
        lo = np.floor((ys.astype(F32) - F32(0.5)) / sc - F32(0.5)).astype(np.int64)
        hi = np.ceil((ys.astype(F32) + F32(1.5)) / sc - F32(0.5)).astype(np.int64)
        Y = np.arange(out)[:, None]
        for margin in (1, 0):
            outside = (Y < np.maximum(0, lo - margin)) | (Y > np.minimum(out - 1, hi + margin))
            assert not (outside & (Wm != 0)).any(), (out, inn, margin)
        assert (Wm.sum(1) == 1).all()
