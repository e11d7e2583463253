"""CPU: what tests/wgrad_cases.py says is right -- the numpy weight gradient is torch's float64 autograd weight gradient of
F.conv2d on every case geometry, the exact inputs are exact in every operand format and sum to integers below 2^24, every case
reaches the kernel, split count, slab size, item count and fold launches its row claims (asked of csrc/conv_choice.h itself, through
tests/tools/conv_choice_dump.cpp), wgrad_chain counts what a brute-force walk over the pixel rows counts, and the bars are not
vacuous: a plain float32 evaluation of the reference in the kernels' structure stays inside them."""
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (path setup)
import wgrad_cases as WC
from test_conv_choice import DUMP_SRC, _fields, _host_compiler, case_line

F32, F64 = np.float32, np.float64
RUN = [c for c in WC.CASES if c.rc == 0]


def all_cases():
    return WC.CASES + [j for g in WC.GROUPS for j in WC.group_jobs(g)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_torchs_float64_weight_gradient():
    """every distinct geometry of the table, on the exact inputs (integers: both sides are exact, so they must be equal), and on the
    real inputs of the small ones; dropping c >= Cm and adding the value dw held"""
    seen = set()
    for c in all_cases():
        if c.shape() in seen:
            continue
        seen.add(c.shape())
        for kind in ("exact", "real") if c.M * c.plane < 5e7 else ("exact",):
            x, dy, dw0 = WC.inputs(c, kind)
            xt = torch.from_numpy(x.astype(F64)).permute(0, 3, 1, 2)
            w = torch.zeros((c.N, c.C, c.k, c.k), dtype=torch.float64, requires_grad=True)
            y = F.conv2d(xt, w, stride=c.stride, padding=c.pad, dilation=c.dil)
            assert tuple(y.shape) == (c.B, c.N, c.Ho, c.Wo), c.id
            y.backward(torch.from_numpy(dy.astype(F64)).permute(0, 3, 1, 2))
            want = w.grad.permute(0, 2, 3, 1).numpy()[..., :c.cm] + dw0.astype(F64)
            got = WC.wgrad_ref(c, x, dy, dw0)
            assert got.shape == (c.N, c.k, c.k, c.cm)
            if kind == "exact":
                assert (got == want).all(), c.id
            else:
                assert np.abs(got - want).max() <= 1e-12 * WC.wgrad_mag(c, x, dy, dw0).max(), c.id
    assert len(seen) >= 30


def test_padding_only_taps_keep_the_prior_value():
    """d6_on_5x5: 8 of the 9 taps only ever see padding -- those rows of dw are dw0; m33_3x3: 6 of 9"""
    for cid, live in (("d6_on_5x5", 1), ("m33_3x3", 3)):
        c = WC.BY_ID[cid]
        x, dy, dw0 = WC.inputs(c, "real")
        same = (WC.wgrad_ref(c, x, dy, dw0) == dw0).all(axis=(0, 3))
        assert int((~same).sum()) == live, (cid, same)
        assert (WC.wgrad_mag(c, x, dy, dw0)[:, same] == np.abs(dw0)[:, same]).all()      # the bar there: the rounding of nothing


# ---------------------------------------------------------------------------------------------------------------------
# 2. exactness
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_inputs_are_exact_in_every_format():
    for c in all_cases():
        if c.rc:
            continue
        x, dy, dw0 = WC.inputs(c, "exact")
        if c.mid:
            continue
        for a, lim in ((x, 3), (dy, 3), (dw0, 8)):
            assert (a == np.round(a)).all() and np.abs(a).max() <= lim
        assert (WC.bf16_round(x) == x).all() and (WC.bf16_round(dy) == dy).all()
        ref, mag = WC.wgrad_ref(c, x, dy, dw0), WC.wgrad_mag(c, x, dy, dw0)
        assert (ref == np.round(ref)).all() and mag.max() < 2 ** 24 and 9 * c.M + 8 < 2 ** 24, c.id
        assert (ref.astype(F32).astype(F64) == ref).all()
        for a in (x, dy):
            hi, mid, lo = WC.x3_terms(a)
            assert (hi == a).all() and not mid.any() and not lo.any()
            h, l_, s = WC.h2_terms(a)
            assert s == 2.0 ** 13 or not a.any()
            assert (h.astype(F64) == a.astype(F64) * s).all() and not l_.any() and np.isfinite(h).all()


def test_exact_inputs_with_a_mid_term():
    """x3_mid_terms: hi = a, mid = +-2^-8 everywhere, lo = 0; every product is a multiple of 2^-16 and sum |dy x| + |dw0| stays below
    2^8, so every partial sum in any order is a float32; without the mid mid products the result differs"""
    cases = [c for c in WC.CASES if c.mid]
    assert [c.id for c in cases] == ["x3_mid_terms"] and cases[0].kernel == WC.X3
    for c in cases:
        x, dy, dw0 = WC.inputs(c, "exact")
        terms = []
        for a in (x, dy):
            hi, mid, lo = WC.x3_terms(a)
            assert (np.abs(hi) >= 2).all() and (hi == np.round(hi)).all() and (np.abs(mid) == 2.0 ** -8).all() and not lo.any()
            assert (hi.astype(F64) + mid == a).all()
            terms.append((hi, mid))
        ref, mag = WC.wgrad_ref(c, x, dy, dw0), WC.wgrad_mag(c, x, dy, dw0)
        assert (ref * 2.0 ** 16 == np.round(ref * 2.0 ** 16)).all() and mag.max() < 2.0 ** 8
        assert (ref.astype(F32).astype(F64) == ref).all()
        g = (c.k, c.stride, c.dil, c.pad)
        midmid = WC.wgrad_sum(terms[0][1], terms[1][1], *g)[..., :c.cm]
        assert (midmid != 0).mean() > 0.5


def test_split_terms_of_the_real_inputs():
    """what the derivation of r uses: the three bfloat16 terms reproduce a float32 exactly, |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|; the two
    fp16 planes reproduce s x to 2^-22 of itself or, where lo is an fp16 subnormal, to 2^-25; |lo| <= 2^-11 |s x|"""
    for c in RUN:
        if c.kind not in ("x3", "planes"):
            continue
        for a in WC.inputs(c, "real")[:2]:
            a64 = a.astype(F64)
            if c.kind == "x3":
                hi, mid, lo = (t.astype(F64) for t in WC.x3_terms(a))
                assert (hi + mid + lo == a64).all(), c.id
                assert (np.abs(mid) <= 2.0 ** -8 * np.abs(a64)).all() and (np.abs(lo) <= 2.0 ** -16 * np.abs(a64)).all()
            else:
                h, l_, s = WC.h2_terms(a)
                h, l_ = h.astype(F64), l_.astype(F64)
                assert np.isfinite(h).all() and 2.0 ** 14 <= np.abs(a64).max() * s < 2.0 ** 15
                assert (np.abs(a64 * s - h - l_) <= np.maximum(2.0 ** -22 * np.abs(a64 * s), 2.0 ** -25)).all(), c.id
                assert (np.abs(l_) <= 2.0 ** -11 * np.abs(a64 * s)).all()


@pytest.mark.parametrize("case", [c for c in RUN if c.kind == "planes"], ids=lambda c: c.id)
def test_plane_representation_errors_fit_their_share_of_r(case):
    """the inputs' own representation errors e = |x - (hi + lo) / s| (elements with a subnormal lo plane included), carried through the
    sum -- sum |dy| e_x + e_dy |x| + e_dy e_x -- stay below the 2 * 2^-22 sum |dy x| that r gives them, for every element of dw"""
    x, dy, dw0 = WC.inputs(case, "real")

    def rep_err(a):
        h, l_, s = WC.h2_terms(a)
        return np.abs(a.astype(F64) - (h.astype(F64) + l_.astype(F64)) / s)
    ex, ey = rep_err(x), rep_err(dy)
    g = (case.k, case.stride, case.dil, case.pad)
    carried = WC.wgrad_sum(ex, np.abs(dy), *g) + WC.wgrad_sum(np.abs(x) + ex, ey, *g)
    share = 2 * 2.0 ** -22 * WC.wgrad_sum(np.abs(x), np.abs(dy), *g)
    assert (carried <= share).all(), float((carried / np.maximum(share, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# 3. each case reaches what the table claims
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_choice") / "conv_choice_dump")
    r = subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", DUMP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [case_line({"kind": "W", "d": c.desc()}, c.id, None) for c in WC.CASES]
    for gid in WC.GROUPS:
        jobs = [j.desc() for j in WC.group_jobs(gid)]
        for tag, elems in (("", WC.GROUP_WS[gid]), ("/short", WC.GROUP_WS[gid] - 1)):
            lines.append(case_line({"kind": "G", "ws": 16, "ws_elems": elems, "jobs": jobs}, gid + tag, None))
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        i, _, rest = ln.partition(" ")
        out[i] = _fields(rest)
    return out


def test_every_case_reaches_its_kernel(chosen):
    kernels, folds = set(), set()
    for c in WC.CASES:
        f = chosen[c.id]
        assert int(f["rc"]) == c.rc, (c.id, f)
        if c.rc:
            continue
        nred = sum(1 for k in f if k.startswith("reduce"))
        got = (f["k"], int(f["splitk"]), int(f["slab_tiles"]), int(f["nitems"]), nred)
        assert got == (c.kernel, c.x_splitk, c.x_slab, c.x_nitems, c.x_nreduce), (c.id, got)
        assert int(f["ws"]) == (0 if c.ws == "atomics" else 1) and int(f["planes"]) == (1 if c.kind == "planes" else 0), c.id
        assert c.ws == "atomics" or c.x_splitk * c.plane <= c.ws_elems
        kernels.add(f["k"])
        folds.add(nred)
    assert kernels == WC.ALL_KERNELS and folds == {0, 1, 2}


def test_table_rows_hold_their_properties(chosen):
    """the properties the rows are there for, from the header's answers"""
    by = WC.BY_ID

    def red(cid, i=0):
        gx, rest = chosen[cid]["reduce%d" % i].split("x", 1)
        t = rest.split("/")
        return dict(gx=int(gx), gy=int(t[0]), block=int(t[1]), splits=int(t[2]), nrs=int(t[3]), cm=int(t[4]), cp=int(t[5]),
                    stride=int(t[6]), fold_only=int(t[7]))
    c = by["plain_bf16_straddle"]
    assert (int(chosen[c.id]["nblk_n"]), int(chosen[c.id]["nblk_k"])) == (2, 3) and 128 % c.C and c.N % 128 and c.Ktot % 128 and c.M == 105
    assert by["plain_1x1_s2"].k == 1 and by["plain_1x1_s2"].stride == 2 and by["plain_1x1_s2"].Hi % 2 and by["plain_1x1_s2"].Wi % 2
    assert [by[i].M for i in ("m1", "m31", "m32", "m33")] == [1, 31, 32, 33]
    assert int(chosen["n64_n24"]["nblk_k"]) == 2 and by["n64_n24"].Ktot - 256 == 104
    assert by["stem_odd_bf16"].tiles == 15 and by["stem_odd_bf16"].k ** 2 == 49
    # the persistent kernel: more items than workgroups, K steps per item around the three-stage ring
    for cid, kt, items in (("ws_items_kt1", 1, 264), ("ws_items_kt2", 2, 264), ("ws_items_kt4", 4, 280)):
        assert int(chosen[cid]["grid"]) == 256 < int(chosen[cid]["nitems"]) == items and by[cid].x_slab == kt
    assert by["ws_items_kt4"].tiles - 13 * 4 == 3 and by["ws_n128_sk5"].tiles - 4 * 4 == 1 and by["big_c120_sk6"].tiles - 5 * 3 == 2
    assert int(chosen["ws_n128_auto"]["nitems"]) == 2 and int(chosen["ws_lin"]["nblk_k"]) == 2 and by["ws_lin"].Ktot - 256 == 8
    assert by["ws_items_kt4"].ws_elems * 4 < 34e6
    # the fold grid strides: more elements than threads
    for cid, block in (("ws_items_kt4", 64), ("big_fold_stride", 256)):
        r = red(cid)
        assert r["block"] == block and r["gx"] * block == WC.FOLD_CAP < r["nrs"] * r["cm"], cid
    assert int(chosen["big_c120_auto"]["nblk_k"]) == 5 and by["big_c120_auto"].Ktot - 4 * 256 == 56
    assert (int(chosen["big_1x1"]["nblk_n"]), int(chosen["big_1x1"]["nblk_k"])) == (2, 3) and by["big_s2_odd"].tiles == 20
    # the chunked fold: chunks of 16 splits, then the chunk sums at a slab stride of 16
    assert [by[i].tiles for i in ("fold_64", "fold_65", "fold_67")] == [64, 65, 67]
    for cid in ("fold_65", "fold_67", "fold_67_cm5", "fold_x3_67", "fold_h2_67", "fold_80_n64", "fold_auto"):
        r0, r1 = red(cid, 0), red(cid, 1)
        assert r0["fold_only"] == 1 and r0["gy"] == -(-by[cid].x_splitk // 16) == r1["splits"] and r1["stride"] == 16 and r1["gy"] == 1, cid
    assert red("fold_67_cm5")["cm"] == 5 != red("fold_67_cm5")["cp"] and red("fold_80_n64")["gy"] * 16 == 80
    assert by["ws_clamps"].ws_elems == 2 * by["ws_clamps"].plane < by["ws_clamps"].splitk * by["ws_clamps"].plane
    assert by["ws_too_small"].ws_elems == by["ws_too_small"].plane - 1


def test_groups_partition_exactly_their_workspace(chosen):
    for gid in WC.GROUPS:
        f, jobs = chosen[gid], WC.group_jobs(gid)
        assert int(f["rc"]) == 0 and f["k"] == "conv_wgrad_group_kernel<2>", gid
        off = 0
        for j, c in enumerate(jobs):
            t = f["job%d" % j].split("/")
            assert (int(t[2]), int(t[3])) == (c.x_splitk, c.x_slab) and int(t[7]) == off and int(t[8]) == c.cm, (gid, j, t)
            off += c.x_splitk * c.plane
        assert off == WC.GROUP_WS[gid]
        assert int(chosen[gid + "/short"]["rc"]) == WC.EINVAL
    assert len(WC.group_jobs("group_12")) == 12 and len({c.shape() for c in WC.group_jobs("group_12")}) == 4
    assert {c.Cm > 0 for c in WC.group_jobs("group_12")} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the bars
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["ws_n128_sk5", "plain_bf16_atomics_sk3"])
def test_chain_against_a_brute_force_count(cid):
    """walk the pixel rows the kernels walk -- 32 per K step, rows past M included as zeros -- into their slabs, then the slabs, then dw"""
    c = WC.BY_ID[cid]
    slab_rows = {}
    for row in range(-(-c.M // 32) * 32):
        s = (row // 32) // -(-c.tiles // c.splitk)
        slab_rows[s] = slab_rows.get(s, 0) + 1
    assert len(slab_rows) == c.x_splitk
    assert WC.wgrad_chain(c) == max(slab_rows.values()) + len(slab_rows) + 1


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.id)
def test_float32_evaluation_stays_inside_the_bar(case):
    """the bar is not vacuous the other way: float32 arithmetic in the kernels' structure (slab sums, then the slabs, then dw0) meets it"""
    x, dy, dw0 = WC.inputs(case, "real")
    err = np.abs(WC.wgrad_f32(case, x, dy, dw0).astype(F64) - WC.wgrad_ref(case, x, dy, dw0))
    bar = WC.wgrad_bar(case, x, dy, dw0)
    assert (err <= bar).all(), (case.id, float((err / np.maximum(bar, 1e-300)).max()))
    assert err.max() > 0 or case.M == 1
