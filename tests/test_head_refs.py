"""CPU: the float64 definitions, input generators, case tables, error bars and comparison functions of tests/head_cases.py are right
on exactly the inputs tests/test_gpu_head_edges.py uses -- so that a failure there is the kernel's.

  * the definitions equal float64 torch: the broadcast distance, F.interpolate(align_corners=False), autograd for the backward, and
    torch.argmax's first maximum on the exact tie cases;
  * the exact cases are exact: features on the 2^-6 grid, squared differences on the 2^-12 grid, the magnitudes a pixel sums below
    2^24 grid units, and four plain float32 evaluations (contracted or not, channels in sequence or pairwise) equal the float64 result;
  * those float32 evaluations stay inside the bars on every real case;
  * the argmax near-tie share of the reference is at most 0.1 % on every real case, and the exact tie cases do tie;
  * an inf and a NaN in the upsampled head's embedding reach, in the definition and in float32, exactly the pixels the case says;
  * every instantiation head.hip's and pool_resize.hip's entry points can launch is reached by a case, and every above-the-cap
    case exceeds grid_for's cap times 256;
  * the comparison has teeth: six deliberately wrong float32 evaluators are each rejected by the comparison functions the GPU
    tests use;
  * the four entry points refuse bad arguments on the host, before any launch (the library loads without a GPU).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as HC
import pool_cases as PC

F32, F64 = np.float32, np.float64
KINDS = ("exact", "real")
SMALL_PLAIN = [c for c in HC.plain_cases() if c not in (HC.BIG_PX1, HC.BIG_PX4)]
SMALL_UP = HC.upsample_cases()[:-2]


def pkinds(kind):
    return HC.PROTO_KINDS if kind == "exact" else ("real",)


def fma32(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact, the sum is rounded once"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


def psum(a):
    """float32 pairwise sum over the last axis"""
    a = np.asarray(a, F32)
    while a.shape[-1] > 1:
        if a.shape[-1] % 2:
            a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), F32)], -1)
        a = a[..., ::2] + a[..., 1::2]
    return a[..., 0]


def ssum(a):
    """float32 sum over the last axis in sequence"""
    a = np.asarray(a, F32)
    acc = np.zeros(a.shape[:-1], F32)
    for i in range(a.shape[-1]):
        acc = acc + a[..., i]
    return acc


def rejected(fn):
    """fn() fails one of the comparison's assertions"""
    try:
        fn()
    except AssertionError:
        return True
    return False


VARIANTS = [(False, False), (False, True), (True, False), (True, True)]        # (contracted, pairwise)


def head32(f, P, fma, pairwise, drop_last=False, last_max=False):
    """a plain float32 evaluation of the head on f[B, H, W, C]: dict of logits NCHW, dissum, argmax"""
    f, P = np.asarray(f, F32), np.asarray(P, F32)
    C, K = f.shape[-1], P.shape[0]
    Cu = C - 1 if (drop_last and C % 4) else C
    with np.errstate(invalid="ignore", over="ignore"):
        t = f[..., None, :Cu] - P[:, :Cu]
        if fma and not pairwise:
            d = np.zeros(t.shape[:-1], F32)
            for c in range(Cu):
                d = fma32(t[..., c], t[..., c], d)
        elif fma:                                                              # pairs contracted, then summed pairwise
            if Cu % 2:
                t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), F32)], -1)
            d = psum(fma32(t[..., 1::2], t[..., 1::2], t[..., ::2] * t[..., ::2]))
        else:
            d = psum(t * t) if pairwise else ssum(t * t)
        lg = -d
        ds = -(psum(lg) if pairwise else ssum(lg))
    L = np.where(np.isnan(lg), -np.inf, lg)
    am = (K - 1 - np.argmax(L[..., ::-1], -1)) if last_max else np.argmax(L, -1)
    return {"logits": np.moveaxis(lg, -1, 1), "dissum": ds, "argmax": am.astype(np.uint8), "feats": f}


def src_index32(out, inn, fma, offset=True):
    """the kernels' float32 source index: scale = (float) in / (float) out"""
    sc = F32(inn) / F32(out)
    d = np.arange(out, dtype=F32) + F32(0.5 if offset else 0.0)
    s = fma32(sc, d, -0.5 if offset else 0.0) if fma else sc * d - F32(0.5 if offset else 0.0)
    s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = s - i0.astype(F32)
    return i0, i1, F32(1) - l1, l1, s


def up32(e, H, W, fma, offset=True):
    e = np.asarray(e, F32)
    _, h, w, _ = e.shape
    y0, y1, ly0, ly1, _ = src_index32(H, h, fma, offset)
    x0, x1, lx0, lx1, _ = src_index32(W, w, fma, offset)
    a0, a1 = lx0[None, None, :, None], lx1[None, None, :, None]
    b0, b1 = ly0[None, :, None, None], ly1[None, :, None, None]
    r0, r1 = e[:, y0], e[:, y1]
    if fma:
        i0, i1 = fma32(a1, r0[:, :, x1], a0 * r0[:, :, x0]), fma32(a1, r1[:, :, x1], a0 * r1[:, :, x0])
        return fma32(b1, i1, b0 * i0)
    return b0 * (a0 * r0[:, :, x0] + a1 * r0[:, :, x1]) + b1 * (a0 * r1[:, :, x0] + a1 * r1[:, :, x1])


def up32_staged(e, H, W):
    """the order of the staged x4 kernel: the two rows are blended first, then the columns"""
    e = np.asarray(e, F32)
    _, h, w, _ = e.shape
    y0, y1, ly0, ly1, _ = src_index32(H, h, False)
    x0, x1, lx0, lx1, _ = src_index32(W, w, False)
    T = ly0[None, :, None, None] * e[:, y0] + ly1[None, :, None, None] * e[:, y1]
    both = (x0 == x1)[None, None, :, None]
    two = lx0[None, None, :, None] * T[:, :, x0] + lx1[None, None, :, None] * T[:, :, x1]
    return np.where(both, (lx0 + lx1)[None, None, :, None] * T[:, :, x0], two)


def bwd32(g, f, P, gf, fma, pairwise, ignore_gf=False):
    g, f, P = np.asarray(g, F32).transpose(0, 2, 3, 1), np.asarray(f, F32), np.asarray(P, F32)
    K = P.shape[0]
    gs = (psum(g) if pairwise else ssum(g))[..., None]
    if pairwise:
        gm = psum(np.moveaxis(g[..., None] * P, -2, -1))
    else:
        gm = np.zeros(f.shape, F32)
        for k in range(K):
            gm = fma32(g[..., k, None], P[k], gm) if fma else gm + g[..., k, None] * P[k]
    v = F32(-2) * (fma32(gs, f, -gm) if fma else gs * f - gm)
    return v if (gf is None or ignore_gf) else v + np.asarray(gf, F32)


plain_inputs, up_inputs = HC.plain_input, HC.upsample_input


# ---------------------------------------------------------------------------------------------------------------------
# definitions against torch, float64
# ---------------------------------------------------------------------------------------------------------------------
def torch_head(x, P):
    """x[B, C, H, W] float64 tensor -> logits[B, K, H, W]"""
    return -((x[:, None] - t64(P)[None, :, :, None, None]) ** 2).sum(2)


@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_backward_definitions_equal_float64_torch(kind):
    for case in HC.plain_cases():
        big = case in (HC.BIG_PX1, HC.BIG_PX4)
        if big and kind == "real":
            continue                                                           # the above-the-cap cases are exact ones
        B, H, W, C, K = case
        for pkind in (pkinds(kind)[:1] if big else pkinds(kind)):
            f, P = plain_inputs(kind, pkind, case)
            ref = HC.head_fwd(f, P, bars=not big)
            x = t64(f.transpose(0, 3, 1, 2), not big)
            lg = torch_head(x, P)
            assert PC.same(ref["logits"], lg.detach().numpy()).all() if kind == "exact" else \
                HC.check_close("logits", ref["logits"], lg.detach().numpy(), 1e-13 * (1 + np.abs(ref["logits"])), False)
            if kind == "exact":
                assert (ref["argmax"] == torch.argmax(lg.detach(), 1).numpy()).all(), (case, pkind)
                assert PC.same(ref["dissum"], -lg.detach().sum(1).numpy()).all()
            if big:
                continue
            g, fb, gf = HC.gradients(kind, B, K, H, W, C, P)
            xb = t64(fb, True)
            lb = torch_head(xb.permute(0, 3, 1, 2), P)
            (lb * t64(g)).sum().backward()
            for gfeats, extra in ((None, 0.0), (gf, gf.astype(F64))):
                df, _ = HC.head_bwd(g, fb, P, gfeats)
                assert (np.abs(df - (xb.grad.numpy() + extra)) <= 1e-12 * (1 + np.abs(df))).all(), (case, pkind)


@pytest.mark.parametrize("kind", KINDS)
def test_upsampled_definition_equals_float64_torch(kind):
    for case in HC.upsample_cases():
        B, h, w, H, W, C, K, am, ds = case
        big = B * H * W > 10 ** 6
        if (big and kind == "real") or kind not in HC.upsample_kinds(case):
            continue
        for pkind in (pkinds(kind)[:1] if big else pkinds(kind)):
            e, P = up_inputs(kind, pkind, case)
            f, Df, ref = HC.upsample_head(e, P, H, W, big)
            x = F.interpolate(t64(e.transpose(0, 3, 1, 2)), size=(H, W), mode="bilinear", align_corners=False)
            lg = torch_head(x, P).numpy()
            assert (np.abs(f - x.numpy().transpose(0, 2, 3, 1)) <= 1e-13 * np.abs(e[np.isfinite(e)]).max()).all()
            assert (np.abs(ref["logits"] - lg) <= 1e-12 * (1 + np.abs(lg))).all(), case
            if kind == "exact":
                assert (ref["argmax"] == np.argmax(lg, 1)).all(), case


def test_nhwc_definition_equals_float64_torch():
    for kind in KINDS:
        for K, Kp in HC.NHWC_KKP:
            for pkind in pkinds(kind):
                e, P = HC.nhwc_inputs(kind, 257, K, Kp, pkind)
                out, bar = HC.nhwc_dist(e, P, K)
                assert (e[:, K:] == 0).all() and (P[:, K:] == 0).all() and (out[:, K:] == 0).all()
                ref = torch_head(t64(e.T[None, :, :, None]), P).numpy()[0, :, :, 0].T
                HC.check_close("nhwc", out[:, :K], ref, 1e-13 * (1 + np.abs(ref)), False)


def test_first_maximum_rules():
    lg = np.array([[1.0, 1.0, 0.0], [np.nan, 2.0, 2.0], [np.nan, np.nan, np.nan], [-np.inf, -np.inf, -np.inf], [np.nan, -np.inf, 3.0]]).T[None]
    assert HC.first_max(lg)[0].tolist() == [0, 1, 0, 0, 2]
    # every exact input carries a tie in pixel 0 and the definition names the first of the tied rows
    for pkind, K, C in (("eye", 16, 16), ("dup", 16, 16), ("dup", 5, 16), ("eye", 2, 3), ("dup", 33, 32)):
        P = HC.protos(pkind, K, C)
        f = HC.features("exact", (1, 1, 4, C), P, pkind)
        lg = HC.head_fwd(f, P)["logits"][0, :, 0, 0]
        tied = np.flatnonzero(lg == lg.max())
        assert len(tied) >= 2 and HC.head_fwd(f, P)["argmax"][0, 0, 0] == tied[0], (pkind, K, C)
        if pkind == "dup":
            assert K // 3 in tied and K - 1 in tied and (P[K - 1] == P[K // 3]).all()
        else:
            assert tied.tolist() == [0, 1] and not (P[0] == P[1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the exact cases are exact
# ---------------------------------------------------------------------------------------------------------------------
def on_grid(f, P, bits, what):
    """features on the 2^-bits grid, squared differences on the 2^-(2 bits) grid, and the squared differences of a pixel -- over every
    channel and prototype: the distances' and the dissum's partial sums in any order -- below 2^24 grid units"""
    f, P = np.asarray(f, F64), np.asarray(P, F64)
    assert (f * 2.0 ** bits == np.rint(f * 2.0 ** bits)).all(), what + ": features off the grid"
    assert (f.astype(F32) == f).all() and (P == np.rint(P)).all()
    tot = np.zeros(f.shape[:-1])
    for k in range(P.shape[0]):
        tot += ((f - P[k]) ** 2).sum(-1)
    assert tot.max() * 4.0 ** bits < 2.0 ** 24, what + ": a partial sum can leave float32"


def test_exact_forward_cases_are_exact():
    for case in HC.plain_cases():
        big = case in (HC.BIG_PX1, HC.BIG_PX4)
        for pkind in (HC.PROTO_KINDS[:1] if big else HC.PROTO_KINDS):
            f, P = plain_inputs("exact", pkind, case)
            on_grid(f, P, 0, "forward %s %s" % (case, pkind))
            if big:
                continue
            ref = HC.head_fwd(f, P)
            for fma, pw in VARIANTS:
                HC.check_head("float32 %s" % (case,), head32(f, P, fma, pw), ref, f, None, True)


def test_exact_upsampled_cases_are_exact():
    for case in HC.upsample_cases():
        B, h, w, H, W, C, K, am, ds = case
        if not HC.dyadic(h, w, H, W):
            continue
        big = B * H * W > 10 ** 6
        for out, inn in ((H, h), (W, w)):
            ref = PC.src_index(out, inn)
            for fma in (False, True):
                assert all((np.asarray(a, F64) == b).all() for a, b in zip(src_index32(out, inn, fma), ref)), "float32 source index differs"
            assert (ref[2] * 8 == np.rint(ref[2] * 8)).all() and (ref[3] * 8 == np.rint(ref[3] * 8)).all()
        for pkind in (HC.PROTO_KINDS[:1] if big else HC.PROTO_KINDS):
            e, P = up_inputs("exact", pkind, case)
            f, _, ref = HC.upsample_head(e, P, H, W, True)
            on_grid(f, P, 6, "upsampled %s %s" % (case, pkind))
            if big:
                continue
            evals = [up32(e, H, W, False), up32(e, H, W, True)] + ([up32_staged(e, H, W)] if (H, W) == (4 * h, 4 * w) else [])
            for f32v in evals:
                assert (f32v == f).all(), case
                for fma, pw in VARIANTS:
                    HC.check_head("float32 %s" % (case,), head32(f32v, P, fma, pw), ref, f, None, True)


def test_exact_backward_and_nhwc_cases_are_exact():
    for case in HC.plain_cases():
        B, H, W, C, K = case
        big = case in (HC.BIG_PX1, HC.BIG_PX4)
        for pkind in (HC.PROTO_KINDS[:1] if big else HC.PROTO_KINDS):
            P = HC.protos(pkind, K, C)
            g, f, gf = HC.gradients("exact", B, K, H, W, C, P)
            assert all((a == np.rint(a)).all() for a in (g, f, gf, P))
            mag = np.abs(g).sum(1).max() * (np.abs(f).max() + np.abs(P).max()) * 2 + np.abs(gf).max()
            assert mag < 2.0 ** 24
            if B * H * W >= 2:
                assert (g.transpose(0, 2, 3, 1).reshape(-1, K)[1] == 0).all()
            if big:
                continue
            for gfeats in (None, gf):
                df, _ = HC.head_bwd(g, f, P, gfeats, bars=False)
                for fma, pw in VARIANTS:
                    assert (bwd32(g, f, P, gfeats, fma, pw) == df).all(), case
    for M, K, Kp in [(257, K, Kp) for K, Kp in HC.NHWC_KKP] + [HC.NHWC_BIG]:
        for pkind in HC.PROTO_KINDS:
            e, P = HC.nhwc_inputs("exact", M, K, Kp, pkind)
            on_grid(e, P, 0, "nhwc")


# ---------------------------------------------------------------------------------------------------------------------
# plain float32 evaluations stay inside the bars; the argmax cap holds for the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_float32_forward_inside_its_bars_and_argmax_cap():
    worst = 0.0
    for case in SMALL_PLAIN:
        f, P = plain_inputs("real", "real", case)
        ref = HC.head_fwd(f, P)
        worst = max(worst, HC.argmax_excused(ref["logits"], ref["lbar"]).mean())
        for fma, pw in VARIANTS:
            got = head32(f, P, fma, pw)
            HC.check_head("float32 %s fma=%d pairwise=%d" % (case, fma, pw), got, ref, f, None, False)
            bits = np.ascontiguousarray(got["feats"]).view(np.uint32)
            assert (bits == np.ascontiguousarray(f).view(np.uint32)).all()
        n = case[0] * case[1] * case[2]
        if n >= 6:                                                             # the data that hurts is there and does what it should
            lg = ref["logits"].transpose(0, 2, 3, 1).reshape(n, -1)
            assert lg[0].max() == 0 and np.abs(lg[n // 2]).min() > 1e4
            assert (lg[n - 1] == -np.inf).all() and np.isnan(lg[n - 2]).all() and np.signbit(f.reshape(n, -1)[1, 0])
            assert ref["dissum"].reshape(n)[n - 1] == np.inf and np.isnan(ref["dissum"].reshape(n)[n - 2])
    assert worst <= HC.ARGMAX_EXCUSED_CAP


def test_float32_upsampled_inside_its_bars_and_argmax_cap():
    for case in SMALL_UP:
        B, h, w, H, W, C, K, am, ds = case
        assert HC.upsample_kinds(case) == (KINDS if HC.dyadic(h, w, H, W) else ("real",))       # (exact: compared for equality, above)
        e, P = up_inputs("real", "real", case)
        f, Df, ref = HC.upsample_head(e, P, H, W, False)
        assert HC.argmax_excused(ref["logits"], ref["lbar"]).mean() <= HC.ARGMAX_EXCUSED_CAP, case
        evals = [up32(e, H, W, False), up32(e, H, W, True)] + ([up32_staged(e, H, W)] if (H, W) == (4 * h, 4 * w) else [])
        for f32v in evals:
            for fma, pw in VARIANTS:
                HC.check_head("float32 %s" % (case,), head32(f32v, P, fma, pw), ref, f, Df, False)
        # the data that hurts is there: the corner pixel of image 0 sits on a prototype, the low-resolution pixel in the middle of the
        # flat order -- the corner of image 1 -- has magnitude 1e3, and so have the output pixels that copy it
        n = B * h * w
        assert B == 2 and n // 2 == h * w and (e[0, 0, 0] == P[min(1, K - 1)]).all()
        if n >= 3:                                                             # (1 x 1: two pixels, the second stays as drawn)
            assert np.abs(e.reshape(n, C)[n // 2]).max() > 1e3 and np.abs(ref["logits"]).max() > 1e4
        if H >= h and W >= w:                                                  # not shrinking: the corner output copies the corner input
            assert ref["logits"][0, :, 0, 0].max() == 0 and (f[:, 0, 0] == e[:, 0, 0]).all()
            assert n < 3 or np.abs(ref["logits"][1, :, 0, 0]).min() > 1e4


def test_upsampled_special_cases_propagate_in_the_definition_and_in_float32():
    for case in HC.UP_SPECIAL:
        B, h, w, H, W, C, K, am, ds = case
        assert HC.dyadic(h, w, H, W) and (case in HC.upsample_cases() or (h, w, H, W) in HC.UP_C16 + HC.UP_X4)
        bad, e, P, must, may = HC.upsample_special(case)
        assert np.isinf(bad).sum() == 1 and np.isnan(bad).sum() == 1 and (must <= may).all() and must.any() and not may.all()
        f, Df, ref = HC.upsample_head(e, P, H, W, False)
        with np.errstate(invalid="ignore"):
            fb = HC.upsample_head(bad, P, H, W, True)[2]                       # the definition itself
        assert (~np.isfinite(fb["logits"].transpose(0, 2, 3, 1)[must])).all() and (~np.isfinite(fb["dissum"][must])).all()
        assert PC.same(fb["logits"].transpose(0, 2, 3, 1)[~may], ref["logits"].transpose(0, 2, 3, 1)[~may]).all()
        with np.errstate(invalid="ignore"):                                    # a zero weight times inf
            evals = [up32(bad, H, W, False), up32(bad, H, W, True)] + ([up32_staged(bad, H, W)] if (H, W) == (4 * h, 4 * w) else [])
        for f32v in evals:
            HC.check_propagation("float32 %s" % (case,), head32(f32v, P, False, False), ref, f, Df, must, may)
        # teeth: an evaluator that cleans its input first is rejected
        clean = head32(up32(np.nan_to_num(bad, nan=0.0, posinf=0.0), H, W, False), P, False, False)
        assert rejected(lambda: HC.check_propagation("mutant", clean, ref, f, Df, must, may))


def test_float32_backward_and_nhwc_inside_their_bars():
    for case in SMALL_PLAIN:
        B, H, W, C, K = case
        P = HC.protos("real", K, C)
        g, f, gf = HC.gradients("real", B, K, H, W, C, P)
        for gfeats in (None, gf):
            df, bar = HC.head_bwd(g, f, P, gfeats)
            for fma, pw in VARIANTS:
                HC.check_close("float32 backward %s" % (case,), bwd32(g, f, P, gfeats, fma, pw), df, bar, False)
        # the cancelling channel: its result is far below the magnitudes that entered, and the bar does not shrink with it
        n = B * H * W
        gp = g.transpose(0, 2, 3, 1).reshape(n, K).astype(F64)
        df0, bar0 = HC.head_bwd(g, f, P)
        terms = np.abs(gp[n - 1].sum() * f.reshape(n, C)[n - 1, 0])
        if terms > 1e-3:
            assert abs(df0.reshape(n, C)[n - 1, 0]) <= 1e-5 * 2 * terms and bar0.reshape(n, C)[n - 1, 0] >= 2 * HC.EPS32 * terms
    for K, Kp in HC.NHWC_KKP:
        e, P = HC.nhwc_inputs("real", 257, K, Kp, "real")
        out, bar = HC.nhwc_dist(e, P, K)
        for fma, pw in VARIANTS:
            got = head32(e[:, None, None, :], P, fma, pw)["logits"][:, :, 0, 0]
            HC.check_close("float32 nhwc", got, out[:, :K], bar[:, :K], False)


# ---------------------------------------------------------------------------------------------------------------------
# the case table reaches everything
# ---------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_reached():
    hit = HC.covered()
    assert hit == set(HC.INSTANTIATIONS), sorted(set(HC.INSTANTIATIONS) - hit)
    D = HC.dispatch
    assert D("fwd", 16, 16, 4, 4) == "fwd_c16" and D("fwd", 16, 16, 5, 7) == "fwd<1,16>" and D("fwd", 16, 5, 4, 4) == "fwd<4,16>"
    assert D("fwd", 17, 16, 4, 4) == "fwd<4,32>" and D("bwd", 32, 33, 1, 3) == "bwd<1,32>" and D("bwd", 16, 16, 1, 4) == "bwd_c16"
    assert D("up", 16, 16, 12, 20, 3, 5) == "up_x4" and D("up", 16, 16, 12, 20, 3, 5, argmax=True) == "up<4,16>"
    assert D("up", 16, 16, 7, 12, 3, 5) == "up_c16" and D("up", 16, 16, 7, 12, 3, 5, dissum=True) == "up<4,16>"
    assert D("up", 16, 16, 7, 9, 3, 5) == "up<1,16>" and D("up", 24, 21, 7, 12, 3, 5) == "up<4,32>" and D("up", 5, 3, 12, 20, 3, 5) == "up<4,16>"
    # the ways into the generic four-pixel upsample kernel, and C % 4 != 0 / the named pairs among the generic cases
    ways = {(C, K, am, ds) for (_, _, _, _, W, C, K, am, ds) in HC.upsample_cases() if W % 4 == 0}
    assert {(16, 13, True, True), (24, 21, True, True), (5, 3, True, True), (16, 16, True, False), (16, 16, False, True)} <= ways
    assert {(16, 5), (32, 33), (24, 21)} <= set(HC.PAIRS) and any(C % 4 for C, _ in HC.PAIRS)
    assert {C for C, _ in HC.PAIRS} >= {1, 3, 4, 13, 16, 17, 20, 32} and {K for _, K in HC.PAIRS} >= {1, 2, 16, 17, 33}
    assert all(C <= HC.MAXC and K <= HC.MAXK for C, K in HC.PAIRS)
    assert {H * W for _, H, W in HC.PX1_SHAPES} >= {1, 3, 35} and all((H * W) % 4 for _, H, W in HC.PX1_SHAPES)
    assert all((H * W) % 4 == 0 for _, H, W in HC.PX4_SHAPES + HC.C16_SHAPES)
    assert [B * H * W // 4 for B, H, W in HC.C16_SHAPES] == [1, 15, 63, 64, 65, 257, 514]
    assert len(HC.NULL_COMBOS) == 16 and HC.NULL_SHAPE in HC.C16_SHAPES


def test_above_the_cap_cases_exceed_the_cap():
    assert HC.CAP_4096 == 1048576 and HC.CAP_2048 == 524288
    for B, H, W, C, K in (HC.BIG_PX1, HC.BIG_PX4):
        assert HC.items("fwd", B, H, W) > HC.CAP_4096 and HC.dispatch("fwd", C, K, H, W) == "fwd<%d,16>" % (1 if W % 4 else 4)
    assert HC.items("fwd", *HC.BIG_PX1[:3]) == 1050625 and HC.items("bwd", *HC.BIG_PX4[:3]) == 1050624
    for B, h, w, H, W, C, K in (HC.UP_BIG_PX4, HC.UP_BIG_PX1):
        assert HC.items("up", B, H, W) > HC.CAP_4096 and HC.dyadic(h, w, H, W)
        assert HC.dispatch("up", C, K, H, W, h, w, True, True) == "up<%d,16>" % (1 if W % 4 else 4)
    assert HC.NHWC_BIG[0] > HC.CAP_2048 and HC.NHWC_BIG[1:] == (2, 4)
    assert all(HC.items("fwd", B, H, W) < 1024 for B, H, W, _, _ in SMALL_PLAIN)


# ---------------------------------------------------------------------------------------------------------------------
# teeth: wrong evaluators are rejected by the comparison the GPU tests use
# ---------------------------------------------------------------------------------------------------------------------
def test_mutant_last_maximum_is_rejected():
    caught = 0
    for pkind in ("eye", "dup"):
        f, P = plain_inputs("exact", pkind, (3, 1, 20, 16, 16))
        ref = HC.head_fwd(f, P)
        HC.check_head("right", head32(f, P, False, False), ref, f, None, True)
        caught += rejected(lambda: HC.check_head("mutant", head32(f, P, False, False, last_max=True), ref, f, None, True))
    assert caught == 2


def test_mutant_dropped_last_channel_is_rejected():
    for kind, pkind in (("exact", "int"), ("real", "real")):
        f, P = plain_inputs(kind, pkind, (2, 3, 4, 13, 17))
        ref = HC.head_fwd(f, P)
        assert rejected(lambda: HC.check_head("mutant", head32(f, P, False, False, drop_last=True), ref, f, None, kind == "exact"))
    f, P = plain_inputs("real", "real", (2, 3, 4, 16, 5))                      # C % 4 == 0: the mutant is the right evaluator
    HC.check_head("right", head32(f, P, False, False, drop_last=True), HC.head_fwd(f, P), f, None, False)


def upsample_mutant(kind, case, mutate):
    B, h, w, H, W, C, K, am, ds = case
    e, P = up_inputs(kind, "eye" if kind == "exact" else "real", case)
    assert kind in HC.upsample_kinds(case)
    exact = kind == "exact"
    f, Df, ref = HC.upsample_head(e, P, H, W, exact)
    HC.check_head("right", head32(up32(e, H, W, False), P, False, False), ref, f, Df, exact)
    return rejected(lambda: HC.check_head("mutant", mutate(e, P, H, W), ref, f, Df, exact))


def test_mutant_low_resolution_width_in_the_pixel_index_is_rejected():
    def mutate(e, P, H, W):
        w = e.shape[2]
        got = head32(up32(e, H, W, False), P, False, False)
        Y, X = np.divmod(np.arange(H * W), W)
        for name in ("logits", "dissum"):
            a = got[name].reshape(got[name].shape[:-2] + (H * W,))
            out = np.full(a.shape, np.nan, F32)
            out[..., Y * w + X] = a                                            # pix = Y * w + X: rows overlap, the tail is never written
            got[name] = out.reshape(got[name].shape)
        got["feats"] = got["argmax"] = None
        return got
    assert upsample_mutant("real", (2, 3, 5, 7, 12, 16, 13, True, True), mutate)
    assert upsample_mutant("exact", (2, 3, 5, 12, 20, 16, 13, True, True), mutate)


def test_mutant_without_the_half_pixel_offset_is_rejected():
    def mutate(e, P, H, W):
        return head32(up32(e, H, W, False, offset=False), P, False, False)
    for kind in KINDS:
        assert upsample_mutant(kind, (2, 3, 5, 12, 20, 16, 16, False, False), mutate)
    assert upsample_mutant("real", (2, 3, 5, 7, 9, 24, 21, True, True), mutate)


def test_mutant_ignoring_gfeats_is_rejected():
    for kind, pkind in (("exact", "int"), ("real", "real")):
        B, H, W, C, K = 2, 3, 4, 16, 5
        P = HC.protos(pkind, K, C)
        g, f, gf = HC.gradients(kind, B, K, H, W, C, P)
        df, bar = HC.head_bwd(g, f, P, gf)
        HC.check_close("right", bwd32(g, f, P, gf, False, False), df, bar, kind == "exact")
        assert rejected(lambda: HC.check_close("mutant", bwd32(g, f, P, gf, False, False, ignore_gf=True), df, bar, kind == "exact"))


def test_mutant_image_index_of_the_first_lane_is_rejected():
    """b taken from lane 0 of the wave: in the 15-group case every lane then computes inside image 0's address range"""
    for kind, pkind in (("exact", "int"), ("real", "real")):
        B, H, W, C, K = 3, 1, 20, 16, 16
        f, P = plain_inputs(kind, pkind, (B, H, W, C, K), special=False)
        ref = HC.head_fwd(f, P)
        x = np.ascontiguousarray(f.transpose(0, 3, 1, 2)).reshape(-1)
        HW, gpi = H * W, H * W // 4
        out = np.full(B * K * HW, np.nan, F32)
        for i in range(B * gpi):
            b = ((i // 64) * 64) // gpi
            for p in range(4):
                pix = (i - b * gpi) * 4 + p
                v = x[(b * C + np.arange(C)) * HW + pix]
                out[(b * K + np.arange(K)) * HW + pix] = head32(v[None, None, None, :], P, False, False)["logits"][0, :, 0, 0]
        assert rejected(lambda: HC.check_close("mutant", out.reshape(B, K, H, W), ref["logits"], ref["lbar"], kind == "exact"))


# ---------------------------------------------------------------------------------------------------------------------
# refusals: argument validation happens on the host, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import helpers  # noqa: F401  (path setup)
    from dmlnet import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED = -1, -3
    p = 0x10000                                                               # never dereferenced: every call below is refused

    def fwd(x=p, pr=p, B=1, C=16, K=16, H=4, W=4):
        return lib.dml_proto_dist_fwd(x, pr, p, p, p, p, B, C, K, H, W, None)

    def up(e=p, pr=p, B=1, h=2, w=2, C=16, K=16, H=8, W=8):
        return lib.dml_upsample_dist_fwd(e, pr, p, p, p, p, B, h, w, C, K, H, W, None)

    def bwd(g=p, f=p, pr=p, df=p, B=1, C=16, K=16, H=4, W=4):
        return lib.dml_proto_dist_bwd(g, p, f, pr, df, B, C, K, H, W, None)

    def nhwc(e=p, pr=p, o=p, M=4, K=13, Kp=16, lde=16, ldo=16):
        return lib.dml_proto_dist_nhwc(e, pr, o, M, K, Kp, lde, ldo, None)

    for fn, ptrs in ((fwd, ("x", "pr")), (up, ("e", "pr")), (bwd, ("g", "f", "pr", "df")), (nhwc, ("e", "pr", "o"))):
        for name in ptrs:
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
    for fn in (fwd, up, bwd):
        for dim in ("B", "H", "W") + (("h", "w") if fn is up else ()):
            for bad in (0, -1):
                assert fn(**{dim: bad}) == EINVAL, (fn.__name__, dim, bad)
        assert fn(C=33) == EUNSUPPORTED and fn(K=34) == EUNSUPPORTED and fn(C=0) == EUNSUPPORTED and fn(K=0) == EUNSUPPORTED
        assert fn(C=-4) == EUNSUPPORTED and fn(K=-1) == EUNSUPPORTED
        assert fn(C=33, B=0) == EINVAL                                          # sizes are looked at first
    assert bwd(H=0, W=0) == EINVAL and bwd(B=-2, H=4, W=4) == EINVAL
    for bad in (0, -5):
        assert nhwc(M=bad) == EINVAL and nhwc(K=bad) == EINVAL
    assert nhwc(K=34, Kp=32, lde=32, ldo=32) == EINVAL and nhwc(Kp=0) == EINVAL and nhwc(K=16, Kp=33, lde=33, ldo=33) == EINVAL
    assert nhwc(K=17, Kp=16) == EUNSUPPORTED and nhwc(K=18, Kp=16) == EINVAL and nhwc(K=33, Kp=32, lde=32, ldo=32) == EUNSUPPORTED
    assert nhwc(lde=15) == EINVAL and nhwc(ldo=15) == EINVAL and nhwc(lde=15, ldo=15) == EINVAL
