"""GPU: the fused stem passes (dml_bn_relu_maxpool3x3s2_fwd, dml_stem_bn_bwd_reduce / _apply), the decoder unit's BatchNorm backward
that forms the embedding conv's data gradient itself (dml_head_bn_bwd_reduce / _apply), and the plans that use them.

Stem, through the C ABI, against the entry points they replace run one after the other on the same inputs (fp32, C = 64, B = 2,
H x W = 5 x 7, 6 x 6, 9 x 12: odd and even sizes clip windows at every border): p0, the argmax bytes, the ReLU mask and -- given the
same `coef` -- dy must be EQUAL, and so must the backward reduce's partial rows and the amax words (max |p0|); the fp16 planes of p0, scaled from the BatchNorm's bound (dml_h2_bound_bn), reproduce p0 to 2^-22
relative (two 11-bit roundings; the inputs keep every positive pooled value above 2^-3 of the scaled unit, below which the lo plane is
subnormal); the sums, d(gamma), d(beta) and coef behind dml_bn_bwd_finalize lie within the bars of tests/bn_cases.py of a float64
evaluation.  That evaluation takes the forward's argmax bytes and mask bits as given (they were just compared) and adds a pixel's
window terms in float64; the kernel adds up to four of them in float32 before the sums, three roundings more on the terms'
magnitudes than the g of bn_cases.reduce_bars, which the bars here add.  The inputs hold channels with gamma < 0 and gamma = 0 (beta
> 0: every window of that channel ties; beta < 0: every output dead), a constant window and a window whose z is all <= 0.

Head (M = 2 x 6 x 5, Kp = 16; K = 16 and 13; N = 256, and N = 20, which is no multiple of 8, for the four-channel plane stores): the
reference materialises dz with a float32 matmul on the host; sums and dy are compared with the float64 result at the same bars plus
the float32 dot product's own error, Kp roundings on sum_k |de_k w_kc| (the host matmul is held to the same bar).

Plans: one f16x2 train step at 2 x 3 x 64 x 64 and at 2 x 3 x 80 x 96 with each switch off against both on: loss, logits, running
statistics and every parameter gradient to 1e-5 of the tensor's largest magnitude -- and, since the plan scales p0's planes from
max |p0| as the unfused plan does and every sum keeps its order, equal.

The stem's backward gates a pixel's gradient with the stem's ReLU mask byte (38 MB, written by the fused forward for the 2 x 2
pixels a pooled pixel owns) instead of "p0 of the window > 0": the same bit -- a window's argmax element equals its pooled value --
and the mask of every unit stays where tests/test_gpu_model.py reads and imposes it.  The window terms are added in
dml_maxpool3x3s2_bwd's own order (its 2 x 2 block kernel), the order bit-equality with that entry point needs.

Each float check prints "MEASURE <what> err=<largest error> bar=<bar>" before it asserts (-s shows them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import bn_cases as CS

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS32 = CS.EPS32


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
    err = np.asarray(err, F64)
    bar = np.asarray(bar, F64) * np.ones_like(err)
    assert np.isfinite(err).all(), "%s: non-finite error" % what
    k = int(np.argmax(np.where(err > bar, np.inf, err / np.maximum(bar, 1e-300)))) if err.size else 0
    print("MEASURE %s err=%.3e bar=%.3e" % (what, err.flat[k] if err.size else 0.0, bar.flat[k] if err.size else 0.0))
    assert (err <= bar).all(), "%s: error %.3e above the bar %.3e" % (what, err.flat[k], bar.flat[k])


class Out:
    """an output buffer of n elements with a sentinel-filled guard of `tail` elements behind it"""

    def __init__(self, n, dtype, tail=64):
        self.n, self.dtype = n, dtype
        self.t = torch.empty(n + tail, dtype=dtype, device="cuda")
        self.t.view(torch.uint8).fill_(0xAA)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.t[self.n:].view(torch.uint8) == 0xAA).all()), "written behind the end of the buffer"
        return self.t[:self.n].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------
STEM_SHAPES = [(5, 7), (6, 6), (9, 12)]
CH = 64


def stem_inputs(Hh, Ww, seed=0):
    B = 2
    rs = np.random.default_rng(1000 + 31 * Hh + Ww + seed)
    y = rs.standard_normal((B, Hh, Ww, CH)).astype(F32)
    y[0, 0:3, 0:3, 0] = F32(0.75)                      # a constant window (ties) in an ordinary channel
    y[1, Hh - 3:Hh, Ww - 3:Ww, 5] = F32(-40.0)         # a window whose z is all <= 0 (gamma[5] > 0)
    gamma = rs.uniform(0.5, 1.5, CH).astype(F32)
    beta = (0.1 * rs.standard_normal(CH)).astype(F32)
    gamma[1], gamma[7] = F32(-1.25), F32(-0.5)          # "pool y, then normalise" is wrong here
    gamma[2], beta[2] = F32(0.0), F32(0.3)              # z constant and positive: every window ties
    gamma[3], beta[3] = F32(0.0), F32(-0.3)             # z constant and negative: every output dead
    mean64, var64 = CS.batch_stats(y.reshape(-1, CH))
    invstd = (1.0 / np.sqrt(var64 + CS.BN_EPS)).astype(F32)
    mean = mean64.astype(F32)
    scale = (gamma * invstd).astype(F32)
    Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    dp = rs.standard_normal((B, Ho, Wo, CH)).astype(F32)
    return dict(B=B, H=Hh, W=Ww, Ho=Ho, Wo=Wo, y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=beta, dp=dp)


def stem_reference(lib, d):
    """dml_bn_apply -> dml_maxpool3x3s2_fwd, and dml_maxpool3x3s2_bwd -> dml_bn_bwd_reduce -> dml_bn_bwd_finalize -> dml_bn_bwd_apply"""
    B, Hh, Ww, Ho, Wo = d["B"], d["H"], d["W"], d["Ho"], d["Wo"]
    M, Mp = B * Hh * Ww, B * Ho * Wo
    y, sc, sh, mu, inv, gam = (dev(d[k]) for k in ("y", "scale", "shift", "mean", "invstd", "gamma"))
    z, mask = Out(M * CH, torch.float32), Out(M * CH // 4, torch.uint8)
    chk(lib.dml_bn_apply(y.data_ptr(), None, z.ptr, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), mask.ptr, M, CH, CH, 0, CH, 1, 0,
                         0.0, 0, None, None, 0, 0, None, 0, None, st()))
    p, am = Out(Mp * CH, torch.float32), Out(Mp * CH, torch.uint8)
    chk(lib.dml_maxpool3x3s2_fwd(z.ptr, p.ptr, am.ptr, B, Hh, Ww, CH, 0, st()))
    dp = dev(d["dp"])
    dz = Out(M * CH, torch.float32)
    chk(lib.dml_maxpool3x3s2_bwd(dp.data_ptr(), am.ptr, dz.ptr, B, Hh, Ww, CH, 0, st()))
    part = torch.full((1100, CH, 2), float("nan"), device="cuda")
    nb = C.c_int(-1)
    chk(lib.dml_bn_bwd_reduce(dz.ptr, y.data_ptr(), None, mask.ptr, mu.data_ptr(), inv.data_ptr(), part.data_ptr(), M, CH, CH, CH, CH, 1,
                              1.0, 0, C.byref(nb), None, st()))
    torch.cuda.synchronize()
    partials = part[:nb.value].cpu().numpy()
    dg, db, coef = torch.zeros(CH, device="cuda"), torch.zeros(CH, device="cuda"), torch.zeros(4 * CH, device="cuda")
    chk(lib.dml_bn_bwd_finalize(part.data_ptr(), nb.value, M, CH, gam.data_ptr(), mu.data_ptr(), inv.data_ptr(), dg.data_ptr(),
                                db.data_ptr(), coef.data_ptr(), st()))
    dy = Out(M * CH, torch.float32)
    chk(lib.dml_bn_bwd_apply(dz.ptr, y.data_ptr(), None, mask.ptr, coef.data_ptr(), dy.ptr, None, M, CH, CH, CH, CH, CH, 0, 1, 1.0, 0, 0,
                             None, None, 0, 0, None, st()))
    return dict(z=z.get(), mask=mask.get(), p=p.get(), argmax=am.get(), dz=dz.get(), dy=dy.get(), coef=coef, partials=partials,
                dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())


_STEM = {}


def stem_case(lib, shape):
    """inputs and the reference's outputs of one shape, computed once and shared"""
    if shape not in _STEM:
        d = stem_inputs(*shape)
        _STEM[shape] = (d, stem_reference(lib, d))
    return _STEM[shape]


def stem_forward(lib, d, want_p=True, want_planes=True):
    B, Hh, Ww, Ho, Wo = d["B"], d["H"], d["W"], d["Ho"], d["Wo"]
    M, Mp = B * Hh * Ww, B * Ho * Wo
    y, sc, sh, mu, gam, bet = (dev(d[k]) for k in ("y", "scale", "shift", "mean", "gamma", "beta"))
    work = torch.zeros(1025, device="cuda")
    chk(lib.dml_h2_bound_bn(gam.data_ptr(), bet.data_ptr(), CH, M, 1.0, None, work.data_ptr(), st()))
    p = Out(Mp * CH, torch.float32) if want_p else None
    am, mask = Out(Mp * CH, torch.uint8), Out(M * CH // 4, torch.uint8)
    pl = Out(2 * Mp * CH, torch.float16) if want_planes else None
    amax = torch.zeros(1024 + 3, device="cuda")
    chk(lib.dml_bn_relu_maxpool3x3s2_fwd(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), p.ptr if p else None, am.ptr,
                                         mask.ptr, pl.ptr if pl else None, Mp * CH, work.data_ptr() + 4096,
                                         amax.data_ptr() if want_p else None, B, Hh, Ww, CH, CH, st()))
    torch.cuda.synchronize()
    assert bool((amax[1024:] == 0).all())
    return dict(p=p.get() if p else None, argmax=am.get(), mask=mask.get(), planes=pl.get().reshape(2, -1) if pl else None,
                unscale=float(work[1024].item()), amax=float(amax.max().item()))


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_forward_equals_apply_then_pool(lib, shape):
    d, ref = stem_case(lib, shape)
    # the inputs are what the docstring promises
    z = ref["z"].reshape(d["B"], d["H"], d["W"], CH)
    assert (z[:, :, :, 2] == z[0, 0, 0, 2]).all() and z[0, 0, 0, 2] > 0 and (z[:, :, :, 3] == 0).all()
    assert (z[0, 0:3, 0:3, 0] == z[0, 0, 0, 0]).all() and (z[1, d["H"] - 3:, d["W"] - 3:, 5] == 0).all()
    pr = ref["p"].reshape(d["B"], d["Ho"], d["Wo"], CH)
    assert (pr[:, :, :, 3] == 0).all() and pr[1, -1, -1, 5] == 0 and (ref["argmax"].reshape(pr.shape)[:, 1:, 1:, 2] == 0).all()
    out = stem_forward(lib, d)
    assert (out["p"].view(np.int32) == ref["p"].view(np.int32)).all(), "p0 differs at %d elements" % int((out["p"] != ref["p"]).sum())
    assert (out["argmax"] == ref["argmax"]).all(), "argmax bytes"
    assert (out["mask"] == ref["mask"]).all(), "ReLU mask bytes"
    assert out["amax"] == ref["p"].max(), "the amax words hold max |p0|"
    # planes: the scale is the bound's, nothing overflows, hi + lo reproduces p0 to 2^-22
    un = out["unscale"]
    assert un == CS.unscale_of_bound(CS.fwd_bound(d["gamma"], d["beta"], CH, d["B"] * d["H"] * d["W"]))
    hi, lo = out["planes"][0].astype(F64), out["planes"][1].astype(F64)
    assert np.isfinite(hi).all() and np.isfinite(lo).all() and np.abs(hi).max() < 2.0 ** 15
    p64 = ref["p"].astype(F64)
    pos = p64[p64 > 0]
    assert pos.size and pos.min() / un >= 0.125, "a pooled value below the range in which the lo plane is a normal number"
    check_le("planes of p0 %dx%d" % shape, np.abs((hi + lo) * un - p64), 2.0 ** -22 * np.abs(p64))
    eh, el = CS.h2_planes(ref["p"], un)
    assert (out["planes"][0].view(np.int16) == eh.view(np.int16)).all() and (out["planes"][1].view(np.int16) == el.view(np.int16)).all()
    # each output alone: planes only (what the plan asks for), fp32 only
    only = stem_forward(lib, d, want_p=False)
    assert (only["planes"].view(np.int16) == out["planes"].view(np.int16)).all() and (only["argmax"] == ref["argmax"]).all()
    only = stem_forward(lib, d, want_planes=False)
    assert (only["p"].view(np.int32) == ref["p"].view(np.int32)).all() and (only["mask"] == ref["mask"]).all()


def stem_g64(d, ref):
    """float64: g = d(z0) (.) mask and sum |terms| per input pixel, from the forward's argmax bytes and mask bits"""
    B, Hh, Ww, Ho, Wo = d["B"], d["H"], d["W"], d["Ho"], d["Wo"]
    am = ref["argmax"].reshape(B, Ho, Wo, CH).astype(np.int64)
    b, yo, xo, c = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), np.arange(CH), indexing="ij")
    yi, xi = 2 * yo - 1 + am // 3, 2 * xo - 1 + am % 3
    assert (yi >= 0).all() and (yi < Hh).all() and (xi >= 0).all() and (xi < Ww).all()
    g, ga = np.zeros((B, Hh, Ww, CH)), np.zeros((B, Hh, Ww, CH))
    np.add.at(g, (b, yi, xi, c), d["dp"].astype(F64))
    np.add.at(ga, (b, yi, xi, c), np.abs(d["dp"].astype(F64)))
    on = CS.unpack_mask(ref["mask"].reshape(B * Hh * Ww, CH // 4), 4)
    return np.where(on, g.reshape(-1, CH), 0.0), np.where(on, ga.reshape(-1, CH), 0.0)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_backward_equals_pool_then_bn_backward(lib, shape):
    d, ref = stem_case(lib, shape)
    B, Hh, Ww = d["B"], d["H"], d["W"]
    M = B * Hh * Ww
    y, mu, inv, gam, dp = (dev(d[k]) for k in ("y", "mean", "invstd", "gamma", "dp"))
    am, mask = dev(ref["argmax"]), dev(ref["mask"])
    g64, gabs = stem_g64(d, ref)
    on = CS.unpack_mask(ref["mask"].reshape(M, CH // 4), 4)
    check_le("pooling backward of the reference %dx%d" % shape, np.abs(np.where(on, ref["dz"].reshape(M, CH).astype(F64), 0.0) - g64),
             3 * EPS32 * gabs)
    y2 = d["y"].reshape(M, CH)
    sums = CS.bwd_sums(g64, y2, d["mean"], d["invstd"])
    # reduce
    part = torch.full((2100, CH, 2), float("nan"), device="cuda")
    gmax = torch.zeros(1024 + 3, device="cuda")
    nb = C.c_int(-1)
    chk(lib.dml_stem_bn_bwd_reduce(dp.data_ptr(), am.data_ptr(), mask.data_ptr(), y.data_ptr(), mu.data_ptr(), inv.data_ptr(),
                                   part.data_ptr(), B, Hh, Ww, CH, CH, C.byref(nb), gmax.data_ptr(), st()))
    torch.cuda.synchronize()
    nb = nb.value
    assert nb == ref["partials"].shape[0] and bool(torch.isnan(part[nb:]).all()) and bool((gmax[1024:] == 0).all())
    # the geometry and the order of additions of dml_bn_bwd_reduce: the same partial rows, bit for bit
    assert (part[:nb].cpu().numpy().view(np.int32) == ref["partials"].view(np.int32)).all(), "partial rows differ from dml_bn_bwd_reduce's"
    got = part[:nb].cpu().numpy().astype(F64).sum(0).T
    n = CS.partial_rows_bound(M, nb)                   # pixels one partial row covers, at most
    xhat = (y2.astype(F64) - d["mean"].astype(F64)) * d["invstd"].astype(F64)
    bars = CS.reduce_bars(gabs, y2, d["mean"], d["invstd"], n) + 3 * EPS32 * np.stack([gabs.sum(0), (gabs * np.abs(xhat)).sum(0)])
    tag = "%dx%d" % shape
    check_le("stem reduce sum g %s" % tag, np.abs(got[0] - sums[0]), bars[0])
    check_le("stem reduce sum g xhat %s" % tag, np.abs(got[1] - sums[1]), bars[1])
    g32 = np.where(on, ref["dz"].reshape(M, CH), F32(0))
    assert float(gmax.max().item()) == np.abs(g32).max(), "gmax is max |g|"
    # finalize: parameter gradients and coefficients against float64
    dg, db, coef = torch.zeros(CH, device="cuda"), torch.zeros(CH, device="cuda"), torch.zeros(4 * CH, device="cuda")
    chk(lib.dml_bn_bwd_finalize(part.data_ptr(), nb, M, CH, gam.data_ptr(), mu.data_ptr(), inv.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                coef.data_ptr(), st()))
    torch.cuda.synchronize()
    cref = CS.bwd_coef(sums, d["gamma"], d["mean"], d["invstd"], M)
    A = np.abs(cref[0])
    cbar = EPS32 * np.abs(cref) + np.stack([0 * A, A * d["invstd"].astype(F64) * bars[1] / M, A * bars[0] / M, 0 * A])
    check_le("stem d(beta) %s" % tag, np.abs(db.cpu().numpy().astype(F64) - sums[0]), bars[0] + EPS32 * np.abs(sums[0]))
    check_le("stem d(gamma) %s" % tag, np.abs(dg.cpu().numpy().astype(F64) - sums[1]), bars[1] + EPS32 * np.abs(sums[1]))
    check_le("stem coef %s" % tag, np.abs(coef.cpu().numpy().astype(F64).reshape(4, CH) - cref), cbar)
    # apply with the reference's coefficients: dy equal, alone and beside its planes
    un = dev(np.array([2.0 ** -9], F32))
    for want_dy, want_pl in ((True, False), (True, True), (False, True)):
        dy = Out(M * CH, torch.float32) if want_dy else None
        pl = Out(2 * M * CH, torch.float16) if want_pl else None
        chk(lib.dml_stem_bn_bwd_apply(dp.data_ptr(), am.data_ptr(), mask.data_ptr(), y.data_ptr(), ref["coef"].data_ptr(),
                                      dy.ptr if dy else None, B, Hh, Ww, CH, CH, CH, pl.ptr if pl else None, M * CH, CH,
                                      un.data_ptr() if pl else None, st()))
        if dy:
            o = dy.get()
            assert (o.view(np.int32) == ref["dy"].view(np.int32)).all(), "dy differs at %d elements" % int((o != ref["dy"]).sum())
        if pl:
            hi, lo = CS.h2_planes(ref["dy"], 2.0 ** -9)
            o = pl.get().reshape(2, -1)
            assert (o[0].view(np.int16) == hi.view(np.int16)).all() and (o[1].view(np.int16) == lo.view(np.int16)).all(), "dy planes"
    # and against float64 at the apply kernels' bar
    dy64 = CS.bwd_apply_ref(g64, y2, cref)
    c32 = ref["coef"].cpu().numpy().astype(F64).reshape(4, CH)
    bar = CS.bwd_apply_bar(g64, y2, c32, 1.0) + 3 * EPS32 * np.abs(c32[0]) * gabs
    slack = np.abs(c32[0] - cref[0]) * np.abs(g64) + np.abs(c32[1] - cref[1]) * np.abs(y2.astype(F64) - cref[3]) + np.abs(c32[2] - cref[2])
    check_le("stem dy against float64 %s" % tag, np.abs(ref["dy"].reshape(M, CH).astype(F64) - dy64), bar + slack)


def test_stem_entry_points_refuse_what_they_cannot_take(lib):
    d, ref = stem_case(lib, (5, 7))
    y, v = dev(d["y"]), dev(d["scale"])
    o, am = Out(2 * 3 * 4 * CH, torch.float32), Out(2 * 3 * 4 * CH, torch.uint8)
    f = lib.dml_bn_relu_maxpool3x3s2_fwd
    assert f(y.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), None, am.ptr, None, None, 0, None, None, 2, 5, 7, CH, CH, st()) == -1
    assert f(y.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), o.ptr, am.ptr, None, None, 0, None, None, 2, 5, 7, 60, 60, st()) == -2
    assert f(y.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), o.ptr, am.ptr, None, o.ptr, 8, None, None, 2, 5, 7, CH, CH, st()) == -1
    nb = C.c_int(0)
    assert lib.dml_stem_bn_bwd_reduce(y.data_ptr(), am.ptr, None, y.data_ptr(), v.data_ptr(), v.data_ptr(), o.ptr, 2, 5, 7, CH, CH,
                                      C.byref(nb), None, st()) == -1
    assert lib.dml_stem_bn_bwd_apply(y.data_ptr(), am.ptr, am.ptr, y.data_ptr(), v.data_ptr(), None, 2, 5, 7, CH, CH, CH, None, 0, 0, None,
                                     st()) == -1
    assert lib.dml_stem_bn_bwd_apply(y.data_ptr(), am.ptr, am.ptr, y.data_ptr(), v.data_ptr(), o.ptr, 2, 5, 7, 6, 6, 6, None, 0, 0, None,
                                     st()) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
HEAD_M, HEAD_KP = 2 * 6 * 5, 16


@pytest.mark.parametrize("N,K", [(256, 16), (256, 13), (20, 16)])
def test_head_bn_backward_forms_the_data_gradient(lib, N, K):
    M, Kp = HEAD_M, HEAD_KP
    rs = np.random.default_rng(77 + N + K)
    de = rs.standard_normal((M, Kp)).astype(F32)
    de[:, K:] = 0                                      # the embedding's pad channels carry no gradient
    w = (rs.standard_normal((K, N)) / 16).astype(F32)
    y = rs.standard_normal((M, N)).astype(F32)
    on = rs.random((M, N)) < 0.6
    gamma = rs.uniform(0.5, 1.5, N).astype(F32)
    mean64, var64 = CS.batch_stats(y)
    mean, invstd = mean64.astype(F32), (1.0 / np.sqrt(var64 + CS.BN_EPS)).astype(F32)
    # reference: dz materialised by a float32 matmul on the host; truth: the float64 product of the same float32 inputs
    dz32 = de[:, :K] @ w
    dz64 = de[:, :K].astype(F64) @ w.astype(F64)
    dabs = np.abs(de[:, :K]).astype(F64) @ np.abs(w).astype(F64)
    gerr = np.where(on, Kp * EPS32 * dabs, 0.0)         # a float32 dot product of Kp terms, in any order, with or without FMA
    check_le("host float32 matmul N=%d K=%d" % (N, K), np.where(on, np.abs(dz32.astype(F64) - dz64), 0.0), gerr)
    g64 = np.where(on, dz64, 0.0)
    sums = CS.bwd_sums(g64, y, mean, invstd)
    xhat = (y.astype(F64) - mean.astype(F64)) * invstd.astype(F64)
    d_de, d_w, d_y, d_mask, d_mu, d_inv, d_gam = (dev(a) for a in (de, w, y, CS.pack_mask(on, 4), mean, invstd, gamma))
    tag = "N=%d K=%d" % (N, K)
    for relu in (1, 0):
        gg, ge = (g64, gerr) if relu else (dz64, Kp * EPS32 * dabs)
        ss = sums if relu else CS.bwd_sums(dz64, y, mean, invstd)
        part = torch.full((1100, N, 2), float("nan"), device="cuda")
        gmax = torch.zeros(1024 + 3, device="cuda")
        nb = C.c_int(-1)
        chk(lib.dml_head_bn_bwd_reduce(d_de.data_ptr(), d_w.data_ptr(), d_y.data_ptr(), d_mask.data_ptr() if relu else None,
                                       d_mu.data_ptr(), d_inv.data_ptr(), part.data_ptr(), M, N, K, Kp, Kp, N, N, relu, C.byref(nb),
                                       gmax.data_ptr(), st()))
        torch.cuda.synchronize()
        nb = nb.value
        assert 1 <= nb <= 1100 and bool(torch.isnan(part[nb:]).all()) and bool((gmax[1024:] == 0).all())
        got = part[:nb].cpu().numpy().astype(F64).sum(0).T
        bars = CS.reduce_bars(gg, y, mean, invstd, CS.partial_rows_bound(M, nb)) + np.stack([ge.sum(0), (ge * np.abs(xhat)).sum(0)])
        check_le("head reduce sum g %s relu=%d" % (tag, relu), np.abs(got[0] - ss[0]), bars[0])
        check_le("head reduce sum g xhat %s relu=%d" % (tag, relu), np.abs(got[1] - ss[1]), bars[1])
        check_le("head reduce gmax %s relu=%d" % (tag, relu), abs(float(gmax.max().item()) - np.abs(gg).max()), ge.max() + EPS32 * np.abs(gg).max())
    # apply, with the float64 coefficients rounded to float32
    coef = CS.bwd_coef(sums, gamma, mean, invstd, M).astype(F32)
    d_coef = dev(coef.reshape(-1))
    dy64 = CS.bwd_apply_ref(g64, y, coef)
    bar = CS.bwd_apply_bar(g64, y, coef, 1.0) + np.abs(coef[0].astype(F64)) * gerr
    un = dev(np.array([2.0 ** -9], F32))
    outs = {}
    for want_dy, want_pl in ((True, False), (True, True), (False, True)):
        dy = Out(M * N, torch.float32) if want_dy else None
        pl = Out(2 * M * N, torch.float16) if want_pl else None
        chk(lib.dml_head_bn_bwd_apply(d_de.data_ptr(), d_w.data_ptr(), d_y.data_ptr(), d_mask.data_ptr(), d_coef.data_ptr(),
                                      dy.ptr if dy else None, M, N, K, Kp, Kp, N, N, N, 1, pl.ptr if pl else None, M * N, N,
                                      un.data_ptr() if pl else None, st()))
        outs[(want_dy, want_pl)] = (dy.get().reshape(M, N) if dy else None, pl.get().reshape(2, M, N) if pl else None)
    o = outs[(True, False)][0]
    check_le("head apply dy %s" % tag, np.abs(o.astype(F64) - dy64), bar)
    assert (outs[(True, True)][0].view(np.int32) == o.view(np.int32)).all()
    hi, lo = CS.h2_planes(o, 2.0 ** -9)
    for key in ((True, True), (False, True)):            # (False, True): the 16-byte plane stores of lane pairs where N % 8 == 0
        p = outs[key][1]
        assert (p[0].view(np.int16) == hi.view(np.int16)).all() and (p[1].view(np.int16) == lo.view(np.int16)).all(), "dy planes %s" % (key,)


def test_head_entry_points_refuse_what_they_cannot_take(lib):
    t = torch.zeros(4096, device="cuda")
    nb = C.c_int(0)
    p = t.data_ptr()
    r = lambda Kp, K, N: lib.dml_head_bn_bwd_reduce(p, p, p, p, p, p, p, 4, N, K, Kp, Kp, N, N, 1, C.byref(nb), None, st())
    assert r(12, 12, 8) == -1 and r(16, 17, 8) == -1 and r(16, 16, 6) == -2
    assert lib.dml_head_bn_bwd_reduce(p, p, p, None, p, p, p, 4, 8, 16, 16, 16, 8, 8, 1, C.byref(nb), None, st()) == -1
    assert lib.dml_head_bn_bwd_apply(p, p, p, p, p, None, 4, 8, 16, 16, 16, 8, 8, 8, 1, None, 0, 0, None, st()) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------
SWITCHES = ("DML_FUSE_STEM", "DML_FUSE_HEAD_DGRAD")
NEW = {"DML_FUSE_STEM": {"dml_bn_relu_maxpool3x3s2_fwd", "dml_stem_bn_bwd_reduce", "dml_stem_bn_bwd_apply"},
       "DML_FUSE_HEAD_DGRAD": {"dml_head_bn_bwd_reduce", "dml_head_bn_bwd_apply"}}


def train_step(shape, monkeypatch, off=None):
    import network
    import utils
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    if off is not None:
        monkeypatch.setenv(off, "0")
    m = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
    m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=1))
    m.cuda()
    m.set_compute_dtype(torch.float32, fp32_products="f16x2")
    m.train()
    m.classifier.aspp.project[3].eval()
    utils.set_bn_momentum(m.backbone, 0.01)
    img = H.synth_tensor(41, "fusion.img", (2, 3) + shape).cuda()
    lab = H.synth_labels(41, "fusion.lab", (2,) + shape, 16, 255, ignore_rows=3).cuda()
    lg, _, ft = m(img)
    loss = utils.CrossEntropyLoss(ignore_index=255, alpha=0, beta=0, gamma=0)(lg, lab, ft)
    loss.backward()
    torch.cuda.synchronize()
    plan = next(p for p in m._engine.plans.values() if p.training)
    names = {getattr(fn, "__name__", "") for fn, _ in plan.fwd + plan.bwd}
    out = {"loss": loss.detach().reshape(1).double().cpu(), "logits": lg.detach().double().cpu()}
    for k, b in m.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["state " + k] = b.detach().double().cpu()
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        out["grad " + k] = p.grad.detach().double().cpu()
    return out, names


@pytest.mark.parametrize("shape", [(64, 64), (80, 96)])
def test_train_step_with_each_fusion_off_agrees(shape, monkeypatch):
    on, names = train_step(shape, monkeypatch)
    assert NEW["DML_FUSE_STEM"] <= names and NEW["DML_FUSE_HEAD_DGRAD"] <= names and "dml_maxpool3x3s2_fwd" not in names
    for sw in SWITCHES:
        off, names_off = train_step(shape, monkeypatch, off=sw)
        assert not (NEW[sw] & names_off) and NEW[[s for s in SWITCHES if s != sw][0]] <= names_off
        assert ("dml_maxpool3x3s2_bwd" in names_off) == (sw == "DML_FUSE_STEM")
        worst, where = 0.0, None
        for k in on:
            e = (on[k] - off[k]).abs().max().item() / (off[k].abs().max().item() + 1e-30)
            if e > worst:
                worst, where = e, k
        print("MEASURE %s=0 against on at %dx%d err=%.3e bar=%.3e (%s)" % ((sw,) + shape + (worst, 1e-5, where)))
        assert set(on) == set(off) and worst <= 1e-5, "%s: %s differs by %.3e of its largest magnitude" % (sw, where, worst)
        # (the bar the fusions were asked to meet; built as they are -- same plane scales, same order of every sum -- nothing moves)
        assert worst == 0.0, "%s: %s differs by %.3e: the fused plan no longer computes the unfused plan's numbers" % (sw, where, worst)
