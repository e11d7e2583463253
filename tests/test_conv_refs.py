"""CPU: what tests/conv_cases.py says is right -- the numpy forward convolution is torch's float64 F.conv2d and the numpy data gradient
its autograd input gradient on every distinct geometry of the table, the four parity-class launches assemble the stride-2 data gradient,
the exact inputs are exact in every operand format and sum below 2^24, every case reaches the kernel, grid, tiling, tail split and
statistics rows its row claims (asked of csrc/conv_choice.h itself, through tests/tools/conv_choice_dump.cpp), the table reaches every
instantiation of ALL_KERNELS, and the bars are neither vacuous (a float32 evaluation in the kernels' structure stays inside them) nor
slack (a kernel that drops a tap of a tile, the last K step, a tail part, a cross term of the split, forgets the batch boundary or reads
a channel past the slice leaves them, or changes an exact result)."""
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (path setup)
import conv_cases as CC
from test_conv_choice import DUMP_SRC, _fields, _host_compiler, case_line

F32, F64 = np.float32, np.float64
RUN = [c for c in CC.CASES if c.rc == 0]
EVERY = CC.CASES + [CC.SUB_PARENT] + CC.SUB_CASES
BIG = 2e10                                  # multiply-adds above which a case would be checked on the exact inputs only (none is)
_CACHE = {}


def data(case, kind):
    """(inputs, reference) of a case, computed once"""
    key = (case.id, kind)
    if key not in _CACHE:
        inp = CC.inputs(case, kind)
        _CACHE[key] = (inp, CC.reference(case, inp))
    return _CACHE[key]


def macs(c):
    return c.M * c.Ktot * c.N


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
def torch_conv(c, x, w):
    """the launch's convolution by torch in float64: F.conv2d, or the autograd input gradient of F.conv2d"""
    xt, wt = torch.from_numpy(np.asarray(x, F64)), torch.from_numpy(np.asarray(w, F64))
    if c.mode == 0:
        y = F.conv2d(xt.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), stride=c.stride, padding=c.pad, dilation=c.dil)
        assert tuple(y.shape) == (c.B, c.N, c.Ho, c.Wo), c.id
        return y.permute(0, 2, 3, 1).reshape(c.M, c.N).numpy()
    xin = torch.zeros((c.B, c.N, c.Ho, c.Wo), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xin, wt.permute(3, 0, 1, 2), stride=c.stride, padding=c.pad, dilation=c.dil)       # the forward weight [Cout][Cin][R][S]
    assert tuple(y.shape) == (c.B, c.C, c.Hi, c.Wi), c.id
    y.backward(xt.permute(0, 3, 1, 2))
    return xin.grad.permute(0, 2, 3, 1).reshape(c.M, c.N).numpy()


def test_reference_is_torchs_float64_convolution_and_input_gradient():
    seen = set()
    for c in CC.CASES + [CC.SUB_PARENT]:
        if c.geometry() in seen:
            continue
        seen.add(c.geometry())
        for kind in ("exact", "real") if macs(c) < BIG else ("exact",):
            inp = CC.inputs(c, kind)
            got, want = CC.conv_core(c, inp["x"], inp["w"]), torch_conv(c, inp["x"], inp["w"])
            if kind == "exact" and c.special is None:
                assert (got == want).all(), c.id
            else:
                mag = CC.conv_core(c, np.abs(inp["x"]), np.abs(inp["w"]))
                assert (np.abs(got - want) <= 1e-12 * mag).all(), c.id
    assert len(seen) >= 30 and {g[0] for g in seen} == {0, 1}


def test_parity_classes_assemble_the_stride2_gradient():
    """the four class launches (1, 2, 2 and 4 taps of the transposed weights, each on dY's grid) written through out_rows into one
    tensor are the 3 x 3 stride-2 data gradient, on the exact inputs exactly"""
    p = CC.SUB_PARENT
    for kind in ("exact", "real"):
        inp = CC.inputs(p, kind)
        want = CC.conv_core(p, inp["x"], inp["w"])
        got = np.full_like(want, np.nan)
        taps = 0
        for c, rs, ss in CC.parity_classes():
            assert (c.Hi, c.Wi, c.My) == (p.Hi, p.Wi, p.M)
            sub = inp["w"][:, rs][:, :, ss]
            taps += len(rs) * len(ss)
            rows = CC.out_rows(c)
            assert np.isnan(got[rows]).all()
            got[rows] = CC.conv_core(c, inp["x"], sub)
        assert taps == 9 and not np.isnan(got).any()
        if kind == "exact":
            assert (got == want).all()
        else:
            assert (np.abs(got - want) <= 1e-12 * CC.conv_core(p, np.abs(inp["x"]), np.abs(inp["w"]))).all()


def test_epilogues_of_the_reference():
    """the epilogue walk on hand-checkable properties: statistics partials sum to the column sums and merge to the variance; the
    BatchNorm-backward sums use the stored value under the mask; padding-only taps contribute nothing"""
    c = CC.BY_ID["ring_fwd_n64"]
    inp, ref = data(c, "real")
    assert np.allclose(ref["stats"][..., 0].sum(0), ref["conv"].sum(0), rtol=1e-12, atol=1e-9)
    g, ok = CC.groups(c, ref["conv"], c.stat_rows)
    cnt = ok.sum(1)[:, None]
    mean = ref["conv"].mean(0)
    var = (ref["stats"][..., 1].sum(0) + (cnt * (g.sum(1) / cnt - mean) ** 2).sum(0)) / c.M
    assert np.allclose(var, ref["conv"].var(0), rtol=1e-10)
    c = CC.BY_ID["ring_dg_n256"]
    inp, ref = data(c, "exact")
    on = inp["bnr_on"]
    assert (ref["bnr"][..., 0].sum(0) == np.where(on, ref["stored"], 0).sum(0)).all() and not on.all() and on.any()
    assert (ref["y"] == ref["conv"] + np.where(inp["res_on"], inp["res"], 0)).all()
    for cid in ("pl_fwd_pad_only", "ring_fwd_pad_only", "f32_pad_only", "x3_pad_only"):
        c = CC.BY_ID[cid]
        inp, ref = data(c, "real")
        centre = CC.conv_fwd(inp["x"], inp["w"][:, 1:2, 1:2], 1, 1, 0, 0, c.Ho, c.Wo).reshape(c.M, c.N)
        assert c.dil > max(c.Hi, c.Wi) and (ref["conv"] == centre).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. exactness
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_inputs_are_exact_in_every_format():
    for c in EVERY:
        if c.rc or c.special:
            continue
        inp, ref = data(c, "exact")
        x, w = inp["x"], inp["w"]
        assert (x == np.round(x)).all() and (w == np.round(w)).all() and np.abs(x).max() <= 3 and np.abs(w).max() <= 3
        for k, a in inp.items():
            if a.dtype == bool or k in ("x", "w"):
                continue
            if k in ("bnr_invstd", "post_scale"):
                assert set(np.unique(a)) <= {0.5, 1.0, 2.0}
            else:
                assert (a == np.round(a)).all() and np.abs(a).max() <= 8 and (CC.bf16_round(a) == a).all()
        assert (CC.bf16_round(x) == x).all() and (CC.bf16_round(w) == w).all()
        assert 9 * c.Ktot + CC.EXTRA_MAX < 2 ** 24, c.id
        if macs(c) < 2e9:               # (the walk over absolute values, where it is cheap: the bound is what the ranges above give)
            assert CC.reference(c, inp, mag=True)["y"].max() <= 9 * c.Ktot + CC.EXTRA_MAX, c.id
        assert (ref["y"] * 2 == np.round(ref["y"] * 2)).all() and (ref["y"].astype(F32).astype(F64) == ref["y"]).all()
        assert (ref["conv"] == np.round(ref["conv"])).all()
        for a in (x, w):
            hi, mid, lo = CC.x3_terms(a)
            assert (hi == a).all() and not mid.any() and not lo.any()
            h, l_, s = CC.h2_terms(a)
            assert s == 2.0 ** 13 and (h.astype(F64) == a.astype(F64) * s).all() and not l_.any() and np.isfinite(h).all()
        if "bnr" in c.epi:
            assert (ref["bnr"] * 4 == np.round(ref["bnr"] * 4)).all() and np.abs(ref["bnr"]).max() < 2 ** 22


def test_exact_inputs_with_a_second_split_term():
    """x3_mid: hi = a, mid = +-2^-8 on the channels below 24, lo = 0, every partial sum a multiple of 2^-16 below 2^8, and the mid mid
    products are there; h2_lo: hi = a 2^13, lo = 2 b, the kept products sum exactly in fp32, the dropped lo lo term is sum b b' 2^-24"""
    c = CC.BY_ID["x3_mid"]
    assert c.kernel == CC.X3K % (64, 0)
    inp, ref = data(c, "exact")
    terms = []
    for a in (inp["x"][..., :24], inp["w"][..., :24]):
        hi, mid, lo = CC.x3_terms(a)
        assert (np.abs(hi) >= 2).all() and (hi == np.round(hi)).all() and (np.abs(mid) == 2.0 ** -8).all() and not lo.any()
        assert (hi.astype(F64) + mid == a).all()
        terms.append(mid)
    assert not inp["x"][..., 24:].any()
    mag = CC.reference(c, inp, mag=True)["y"]
    assert (ref["y"] * 2.0 ** 16 == np.round(ref["y"] * 2.0 ** 16)).all() and mag.max() < 2.0 ** 8
    assert (ref["y"].astype(F32).astype(F64) == ref["y"]).all()
    midmid = np.tensordot(terms[0].reshape(c.M, 24).astype(F64), terms[1].reshape(c.N, 24).astype(F64), axes=([1], [1]))
    assert (midmid != 0).mean() > 0.5
    c = CC.BY_ID["pl_fwd_h2_lo"]
    assert c.kernel == CC.P_N64 % (0, 0) and c.Ktot <= 256
    inp, ref = data(c, "exact")
    planes = []
    for a in (inp["x"], inp["w"]):
        h, l_, s = CC.h2_terms(a)
        h, l_ = h.astype(F64), l_.astype(F64)
        assert s == 2.0 ** 13 and (h + l_ == a.astype(F64) * s).all() and (np.abs(l_) >= 2).all() and (np.abs(l_) <= 6).all()
        assert (h == np.round(a) * s).all()
        planes.append((h, l_))
    kept = sum(CC.conv_core(c, planes[0][i], planes[1][j]) for i, j in ((0, 0), (0, 1), (1, 0)))
    kmag = sum(CC.conv_core(c, np.abs(planes[0][i]), np.abs(planes[1][j])) for i, j in ((0, 0), (0, 1), (1, 0)))
    assert (kept % 2.0 ** 14 == 0).all() and kmag.max() < 2.0 ** 38                  # any partial sum: a multiple of 2^14 below 2^24 of them
    assert (kept * 2.0 ** -26 == ref["y"]).all() and (ref["y"].astype(F32).astype(F64) == ref["y"]).all()
    dropped = CC.h2_lo_dropped(c, inp)
    full = CC.conv_core(c, inp["x"], inp["w"])
    assert (full - dropped == ref["y"]).all() and (dropped != 0).mean() > 0.5 and np.abs(dropped).max() <= c.Ktot * 9 * 2.0 ** -24


def test_split_terms_of_the_real_inputs():
    """what r rests on, on the inputs used (as tests/test_wgrad_refs.py checks for the weight gradients)"""
    for c in RUN + [CC.SUB_PARENT] + CC.SUB_CASES:
        if CC.conv_r(c) == 0.0:
            continue
        inp = CC.inputs(c, "real")
        for a in (inp["x"], inp["w"]):
            a64 = a.astype(F64)
            if CC.conv_r(c) == CC.R_X3:
                hi, mid, lo = (t.astype(F64) for t in CC.x3_terms(a))
                assert (hi + mid + lo == a64).all(), c.id
                assert (np.abs(mid) <= 2.0 ** -8 * np.abs(a64)).all() and (np.abs(lo) <= 2.0 ** -16 * np.abs(a64)).all()
            else:
                h, l_, s = CC.h2_terms(a)
                h, l_ = h.astype(F64), l_.astype(F64)
                assert np.isfinite(h).all() and 2.0 ** 14 <= np.abs(a64).max() * s < 2.0 ** 15
                assert (np.abs(a64 * s - h - l_) <= np.maximum(2.0 ** -22 * np.abs(a64 * s), 2.0 ** -25)).all(), c.id
                assert (np.abs(l_) <= 2.0 ** -11 * np.abs(a64 * s)).all()


@pytest.mark.parametrize("case", [c for c in RUN + [CC.SUB_PARENT] + CC.SUB_CASES if CC.conv_r(c) == CC.R_H2 and not c.special], ids=lambda c: c.id)
def test_plane_representation_errors_fit_their_share_of_r(case):
    """the inputs' own representation errors e = |x - (hi + lo) / s| (elements with a subnormal lo plane included), carried through the
    sum -- sum e_x |w| + (|x| + e_x) e_w -- stay below the 2 * 2^-22 sum |x w| that R_H2 gives them, for every element of y (as
    tests/test_wgrad_refs.py asserts for the weight gradients)"""
    inp = CC.inputs(case, "real")

    def rep_err(a):
        h, l_, s = CC.h2_terms(a)
        return np.abs(a.astype(F64) - (h.astype(F64) + l_.astype(F64)) / s)
    ax, aw = np.abs(inp["x"]).astype(F64), np.abs(inp["w"]).astype(F64)
    ex, ew = rep_err(inp["x"]), rep_err(inp["w"])
    carried = CC.conv_core(case, ex, aw) + CC.conv_core(case, ax + ex, ew)
    share = 2 * 2.0 ** -22 * CC.conv_core(case, ax, aw)
    assert (carried <= share).all(), float((carried / np.maximum(share, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# 3. each case reaches what the table claims
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_cases") / "conv_choice_dump")
    r = subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", DUMP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [case_line({"kind": "C", "d": c.desc()}, c.id, (0, 1, 0)) for c in EVERY]
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        i, _, rest = ln.partition(" ")
        out[i] = _fields(rest)
    return out


def test_every_case_reaches_its_kernel(chosen):
    kernels = set()
    for c in EVERY:
        f = chosen[c.id]
        assert int(f["rc"]) == c.rc, (c.id, f)
        if c.rc:
            assert c.expect[0] is None
            continue
        got = (f["k"], int(f["grid"]), int(f["nblk_m"]), int(f["nblk_n"]), int(f["tail_q"]), int(f["rows"]))
        assert got == c.expect, (c.id, got)
        kernels.add(f["k"])
    assert kernels == CC.ALL_KERNELS, (sorted(CC.ALL_KERNELS - kernels), sorted(kernels - CC.ALL_KERNELS))
    assert len(CC.ALL_KERNELS) == 55


def test_table_rows_hold_their_properties(chosen):
    """the properties the rows are there for, from the header's answers"""
    by = CC.BY_ID

    def tiles(cid):
        return int(chosen[cid]["nblk_m"]) * int(chosen[cid]["nblk_n"])
    # more tiles than persistent workgroups: the second tile of a workgroup
    for cid, n, rows in (("pl_fwd_wrap48", 303, 48), ("pl_fwd_wrap144", 260, 144), ("pl_fwd_wrap192", 257, 192), ("pl_dg_wrap144", 260, 144),
                         ("ws_fwd_wrap144", 260, 144), ("ws_fwd_wrap288", 257, 288), ("ws_dg_wrap144", 260, 144)):
        assert int(chosen[cid]["grid"]) == 256 < tiles(cid) == n and by[cid].M % rows != 0, cid
    assert by["pl_fwd_wrap144"].Ktot == 32 and by["pl_dg_wrap144"].Ktot == 64
    # statistics groups that straddle M
    for cid in ("pl_fwd_wrap48", "pl_fwd_wrap144", "ws_fwd_wrap288", "pl_fwd_n320", "ring_fwd_n64", "ring_fwd_bn128"):
        assert by[cid].M % by[cid].stat_rows != 0 and "stats" in by[cid].epi, cid
    assert {by[c].stat_rows for c in ("pl_fwd_wrap48", "pl_fwd_wrap144", "ring_fwd_n64")} == {48, 144, 64}
    # a half-empty last 128-wide column block; a last channel group of 32
    assert by["pl_fwd_n320"].N % 128 == 64 and by["pl_fwd_n192"].N % 128 == 64 and by["pl_fwd_n320"].C % 64 == 32
    assert by["pl_fwd_5x5"].R * by["pl_fwd_5x5"].S == 25 and tiles("pl_fwd_5x5") == 1
    # grids that are no multiple of 8 (xcd_remap)
    assert [int(chosen[c]["grid"]) % 8 for c in ("ring_fwd_n64", "ring_fwd_n256", "ring_fwd_bn128")] == [3, 4, 2]
    assert by["ring_fwd_bn128"].M % 128 == 32 and by["ring_fwd_256rows"].M % 256 == 177
    # the K-split tail: 264 tiles, 8 beyond the round, 6 parts each
    for cid in ("ring_fwd_tail", "ring_dg_tail"):
        f = chosen[cid]
        assert tiles(cid) == 264 and int(f["tail_full"]) == 256 and int(f["tail_q"]) == 6 and int(f["grid"]) == 256 + 8 * 6
    # the four epilogue instantiations of the two-plane data gradient, on each tile configuration
    for base in (CC.P_N64, CC.P_NARROW, CC.P_W144):
        assert {base % (1, e) for e in range(4)} <= {c.kernel for c in RUN}
    # batch boundaries inside a tile; one-pixel-wide and one-pixel-high maps
    for cid in ("pl_fwd_w1", "ring_fwd_h1", "f32_w1", "x3_h1"):
        c = by[cid]
        assert min(c.Hi, c.Wi) == 1 and c.B == 3 and c.Ho * c.Wo == 50
    # one row past and one row short of a multiple of every row tile
    tile_of = {CC.P_W48: 48, CC.RING64: 128, CC.P_W144: 144, CC.P_N64: 192, CC.RING256: 256, CC.WS288: 288}
    for rows in (48, 128, 144, 192, 256, 288):
        ms = sorted(c.M for c in RUN if c.id.endswith("_tile%d" % rows))
        assert len(ms) == 2 and ms[0] % rows == rows - 1 and ms[1] % rows == 1, (rows, ms)
        for c in RUN:
            if c.id.endswith("_tile%d" % rows):
                fam = [k for k, v in tile_of.items() if v == rows][0]
                assert c.kernel.split("<")[0] == fam.split("<")[0] and int(chosen[c.id]["nblk_m"]) == -(-c.M // rows), c.id
    assert by["ring_dg_n96_bnr_res"].N % 64 == 32
    assert by["pl_dg_s2"].Ho % 2 == 1 and by["pl_dg_s2"].Wo % 2 == 1 and by["pl_dg_s2"].stride == 2
    assert by["pl_dg_k32_falls_to_x3"].Ktot == 32 and by["pl_dg_k32_planes_only"].rc == CC.EUNSUPPORTED
    assert by["planes_7x7"].R * by["planes_7x7"].S > 32 and by["planes_7x7"].kernel == CC.REG % ("f32", 64, 0, 0)
    assert {c.kernel for c in CC.SUB_CASES} == {CC.P_NARROW % (1, 1)} and [(c.R, c.S) for c in CC.SUB_CASES] == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert (CC.SUB_CASES[2].pad, CC.SUB_CASES[2].pad_x) == (1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the bars
# ---------------------------------------------------------------------------------------------------------------------
EMU = RUN + [CC.SUB_PARENT] + CC.SUB_CASES          # every case that launches, the stride-2 data gradients and the parity classes included
assert all(macs(c) < BIG for c in EMU)


def test_chain_counts_the_k_steps():
    by = CC.BY_ID
    assert CC.conv_chain(by["pl_fwd_wrap144"]) == 32 and CC.conv_chain(by["ring_fwd_tail"]) == 1152 + 6
    assert CC.conv_chain(by["reg_bf16_c40"]) == 32 * 12 and by["reg_bf16_c40"].Ktot == 360          # steps straddle taps: ceil(360 / 32)
    assert CC.conv_chain(by["pl_fwd_post"]) == 64 + 4 and CC.conv_chain(by["ring_dg_n256"]) == 576 + 1
    assert CC.conv_r(by["pl_dg_k32_falls_to_x3"]) == CC.R_X3 and CC.conv_r(by["planes_7x7"]) == 0.0 and CC.conv_r(by["pl_dg_s2"]) == CC.R_H2
    assert CC.conv_r(by["ws_fwd_wrap144"]) == 0.0 and CC.conv_r(by["x3_n64"]) == CC.R_X3


@pytest.mark.parametrize("case", [c for c in EMU if not c.special], ids=lambda c: c.id)
def test_float32_evaluation_stays_inside_the_bars(case):
    """not vacuous: float32 arithmetic in the kernels' structure -- K steps of 32 in tap order, the kept products of the emulated split
    terms, tail parts, the epilogue operands, the statistics by the kernel's formula -- meets every bar"""
    inp, ref = data(case, "real")
    acc, y = CC.emulate_f32(case, inp)
    err, bar = np.abs(y.astype(F64) - ref["y"]), CC.y_bar(case, inp, ref)
    assert (err <= bar).all(), (case.id, float((err / np.maximum(bar, 1e-300)).max()))
    assert err.max() > 0
    if "stats" in case.epi:
        g, ok = CC.groups(case, acc.astype(F64), case.stat_rows)
        g, okk = g.astype(F32), ok[:, :, None]
        s = np.where(okk, g, F32(0)).sum(1, dtype=F32)
        mean = s * (F32(1) / ok.sum(1).astype(F32))[:, None]
        m2 = (np.where(okk, g - mean[:, None, :], F32(0)) ** 2).sum(1, dtype=F32)
        got = np.stack([s, m2], -1).astype(F64)
        sb = CC.stats_bars(case, inp, ref)
        assert (np.abs(got - ref["stats"]) <= sb).all(), case.id


def _delta(case, inp, rows, cols, xt=None, wt=None):
    """what zeroing the K columns `cols` of the output rows `rows` takes out of the convolution, float64"""
    P = patches_of(case, inp) if xt is None else xt
    W = inp["w"].reshape(case.N, case.Ktot).astype(F64) if wt is None else wt
    return P[rows][:, cols] @ W[:, cols].T


def patches_of(case, inp):
    key = (case.id, "patches", id(inp))
    if key not in _CACHE:
        _CACHE[key] = CC.patches(case, inp["x"])
    return _CACHE[key]


def leaves(case, kind, delta, rows, ref, inp):
    """a mutation that changes the convolution by `delta` on `rows`: outside the bar on at least one element (real) / a changed
    result (exact)"""
    if kind == "exact":
        return bool((delta != 0).any())
    return bool((np.abs(delta) > CC.y_bar(case, inp, ref)[rows]).any())


# (the special cases differ from their base case on the exact inputs only)
@pytest.mark.parametrize("case,kind", [(c, k) for c in EMU for k in ("exact", "real") if not (c.special and k == "real")],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_mutations_leave_the_bars(case, kind):
    """not slack: each way a kernel can be subtly wrong moves at least one element out of its bar on the real inputs and changes the
    result on the exact ones.  Not applicable (and skipped in the loop, not as a test): the batch boundary where no tap crosses it -- one
    image, one filter row, and the stride-2 data gradients of an odd image (pl_dg_s2*: the rows of z next to the boundary are inserted
    zeros of the image's own pitch, which no dY row maps to; the even image pl_dg_s2_even and f32_stem_dg do cross it) --, the tail part
    where the launch has no tail, the cross term where the operands are used as stored -- and on the exact integer inputs, whose second
    split terms are zero: x3_mid and pl_fwd_h2_lo are there for that"""
    inp, ref = data(case, kind)
    P = patches_of(case, inp)
    tile_rows = {"conv_igemm_dma_kernel<128,0,3,2": 256}.get(case.kernel[:31], 128)
    t0 = np.arange(min(case.M, tile_rows))
    C = case.C
    done = []
    # one tap of one tile: the first tap that is not padding for every row of the first tile
    for tap in range(case.R * case.S):
        cols = np.arange(tap * C, (tap + 1) * C)
        if P[t0][:, cols].any():
            assert leaves(case, kind, _delta(case, inp, t0, cols), t0, ref, inp), "a dropped tap stays inside the bar"
            done.append("tap")
            break
    # the last K step (of a tap that is not padding for the rows looked at)
    ks = -(-case.Ktot // 32)
    for j in range(ks - 1, -1, -1):
        cols = np.arange(j * 32, min((j + 1) * 32, case.Ktot))
        if P[:, cols].any():
            allr = np.arange(case.M)
            assert leaves(case, kind, _delta(case, inp, allr, cols), allr, ref, inp), "a dropped K step stays inside the bar"
            done.append("kstep")
            break
    # a row of the neighbouring image at a batch boundary
    Pm = CC.patches(case, inp["x"], merge_batch=True) if case.B > 1 and case.R > 1 else P
    rows = np.nonzero((Pm != P).any(1))[0]
    if case.B > 1 and case.R > 1:
        assert rows.size or (case.mode == 1 and case.stride == 2 and case.Ho % 2 == 1), case.id
    if rows.size:
        delta = (Pm[rows] - P[rows]) @ inp["w"].reshape(case.N, case.Ktot).astype(F64).T
        assert leaves(case, kind, delta, rows, ref, inp), "a forgotten batch boundary stays inside the bar"
        done.append("batch")
    # one channel past the slice: the neighbouring channel holds NaN
    xs = np.concatenate([inp["x"][..., 1:], np.full(inp["x"].shape[:-1] + (1,), np.nan, F32)], -1)
    assert np.isnan(CC.conv_core(case, xs, inp["w"])).any()
    done.append("channel")
    # one tail part
    if case.tail_q > 1:
        q = case.tail_q
        cols = np.arange((q - 1) * ks // q * 32, case.Ktot)
        rows = np.arange(min(case.M, 128))
        assert leaves(case, kind, _delta(case, inp, rows, cols), rows, ref, inp), "an omitted tail part stays inside the bar"
        done.append("tail")
    # the hi lo cross term of the split
    if CC.conv_r(case) and (kind == "real" or case.special):
        Wm = inp["w"].reshape(case.N, case.Ktot)
        xt, wt = CC.operand_terms(case, P.astype(F32)), CC.operand_terms(case, Wm)
        delta = (xt[0][0] @ wt[1][0].T) / (xt[0][1] * wt[1][1])
        allr = np.arange(case.M)
        assert leaves(case, kind, delta, allr, ref, inp), "a dropped cross term stays inside the bar"
        done.append("cross")
    assert {"tap", "kstep", "channel"} <= set(done), done
