"""CPU: the float64 definitions, inputs, case tables and bars of tests/loss_cases.py are right on exactly the inputs
tests/test_gpu_loss_edges.py uses -- so that a failure there is the kernel's.

  * loss_ref and head_bwd_ref equal float64 torch autograd through oracle/dmlnet_ref.py (F.interpolate(mode="bilinear",
    align_corners=False) -> distance_head -> dml_loss) on every real case, to 1e-12 of the magnitude sums the bars are made of; the
    number correct equals torch.argmax's first maximum, ties included;
  * the exact cases are exact: the dominant class leads by more than 200 in logit, every gradient is a multiple of 2^-14, every term
    of de a multiple of 2^-21 with the magnitudes below 2^24 units, and a float32 evaluation in another order (prototypes backwards,
    columns before rows) EQUALS the float64 result rounded once;
  * a plain float32 evaluation stays inside the bars on the real cases;
  * every case reaches what its name claims: the arithmetic path (head.hip's diagonal test restated), the tile counts, the halo
    situation, and -- the above-the-cap cases -- a second trip of the grid-stride loop, restating the launch arithmetic;
  * the references have teeth.  Each change, applied to the reference, is rejected by the bar of the cases marked x (all of them
    asserted below):
                                   no_wvar   swap_lr   clamp_x1   last_max
      fused exact, alpha on           x         x*        x*
      fused exact, alpha 0                      x*        x*
      fused real, alpha 0.01          x         x*        x*
      every_clamp_1x1 (w = 1)         x
      one_column_7x1  (w = 1)         x
      loss: gradient, alpha 0.01      x
      loss: ties_hw0 / ties_hw3                                      x (sums[3])
    (*: every geometry with w >= 2; with w = 1 both columns are the same one and neither change does anything.)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (path setup)
import head_cases as HC
import loss_cases as LC
import pool_cases as PC
from oracle import dmlnet_ref as O

F32, F64 = np.float32, np.float64
SMALL = [(c, r) for c in LC.LOSS_CASES for r in c[7] if c[0] != "hw1_513_grid_stride"]
FUSED = LC.fused_cases()


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


fused_scalars = LC.fused_scalars


def case_id(c):
    return "-".join(str(v) for v in c)


# ---------------------------------------------------------------------------------------------------------------------
# the definitions against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in FUSED if c[0] != "exact"], ids=case_id)
def test_head_bwd_ref_equals_float64_autograd(case):
    kind, pkind, gname, lkind, ignore = case
    f, lab, P = LC.fused_input(kind, pkind, gname, lkind, ignore)
    B, H_, W_, _ = f.shape
    h, w = H_ // 4, W_ // 4
    nv = float((lab != ignore).sum())
    e = torch.zeros(B, 16, h, w, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(e, size=(H_, W_), mode="bilinear", align_corners=False)
    feats = up + t64(f).permute(0, 3, 1, 2)                                    # the case's features, with the upsample's gradient path
    logits, _, _ = O.distance_head(feats, t64(P))
    loss = O.dml_loss(logits, torch.from_numpy(lab), alpha=float(F32(LC.REAL_ALPHA)), ignore_index=ignore) * float(F32(LC.REAL_GOUT))
    loss.backward()
    want = e.grad.permute(0, 2, 3, 1).numpy()
    de, bar, parts = LC.head_bwd_ref(f, lab, P, nv, float(B), ignore, LC.REAL_ALPHA, LC.REAL_GOUT, parts=True)
    if lkind == "all_ignored":
        assert (de == 0).all() and (np.nan_to_num(want) == 0).all()
        return
    mag = bar / (LC.C_HEAD * LC.EPS32)                                         # at least the magnitude sum
    assert (np.abs(de - want) <= 1e-12 * mag).all(), np.abs(de - want).max()
    assert np.allclose(parts["logits"], logits.detach().numpy(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("case,regime", SMALL, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_loss_ref_equals_float64_autograd(case, regime):
    name, B, K, H_, W_, ign = case[:6]
    lg, lab = LC.loss_input(case, regime)
    x = t64(lg, True)
    ref = O.dml_loss(x, torch.from_numpy(lab), alpha=float(F32(0.01)), ignore_index=ign)
    (ref * 0.5).backward()
    mine = LC.loss_ref(lg, lab, ign, 0.01, float(B), 0.5)
    want = x.grad.numpy()
    if regime == "nan":
        assert np.isnan(ref.item()) and np.isnan(mine["loss"])
        bad = LC.nonfinite_pixels(lg)
        assert bad.sum() == B and np.isnan(mine["grad"].transpose(0, 2, 3, 1)[bad]).all()
        keep = ~np.broadcast_to(bad[:, None], want.shape)
        # torch's mean-reduced cross-entropy sends the NaN loss back to every pixel; the definition is per pixel
        clean = lg.copy()
        clean[np.isnan(clean)] = -50.0
        other = LC.loss_ref(clean, lab, ign, 0.01, float(B), 0.5)["grad"]
        assert np.array_equal(mine["grad"][keep], other[keep])
        return
    assert np.isfinite(ref.item()) and abs(mine["loss"] - ref.item()) <= 1e-12 * abs(ref.item())
    scale = 0.5 / (mine["sums"][1] * B)
    assert (np.abs(mine["grad"] - want) <= 1e-12 * scale).all()
    valid = lab != ign
    pred = torch.from_numpy(lg.astype(F64)).argmax(1).numpy()
    if regime != "ties":                                                       # torch.argmax does not promise the first of a tie
        assert mine["sums"][3] == ((pred == lab) & valid).sum()
    assert mine["sums"][1] == valid.sum() and mine["sums"][4] == B
    if K == 1:
        assert mine["sums"][0] == 0 and abs(mine["loss"] - float(F32(0.01)) * mine["sums"][2] / B) < 1e-15 * abs(mine["loss"])
        assert np.abs(mine["grad"][np.broadcast_to(~valid[:, None], want.shape)]).max(initial=0) == 0
    if regime.startswith("neg_inf"):
        plane = 0 if regime.endswith("0") else K - 1
        hit = np.isneginf(lg[:, plane])
        assert hit.sum() == B and (mine["grad"][:, plane][hit] == 0).all() and np.isfinite(mine["grad"]).all()


@pytest.mark.parametrize("name", ["ties_hw0", "ties_hw3"])
def test_ties_count_the_first_maximum(name):
    """by hand: a tie pixel counts when its label is the lowest maximal plane"""
    case = [c for c in LC.LOSS_CASES if c[0] == name][0]
    lg, lab = LC.loss_input(case, "ties")
    B, K, H_, W_ = lg.shape
    flat, lf = lg.transpose(0, 2, 3, 1).reshape(-1, K), lab.reshape(-1)
    ntie = (flat == flat.max(1, keepdims=True)).sum(1)
    assert set(ntie.tolist()) == {2, K}
    want = sum(1 for row, y in zip(flat, lf) if y != case[5] and int(np.flatnonzero(row == row.max())[0]) == y)
    sums = LC.loss_ref(lg, lab, case[5], 0.01, float(B), None, bars=False)["sums"]
    assert sums[3] == want and 0 < want < (lf != case[5]).sum()
    assert LC.loss_ref(lg, lab, case[5], 0.01, float(B), None, bars=False, mut="last_max")["sums"][3] != want


# ---------------------------------------------------------------------------------------------------------------------
# exact cases are exact; float32 stays inside the bars
# ---------------------------------------------------------------------------------------------------------------------
def head32(f, lab, P, nv, n, ignore, alpha, gout):
    """float32 throughout, prototypes backwards, columns before rows"""
    f, P = np.asarray(f, F32), np.asarray(P, F32)
    B, H_, W_, Cc = f.shape
    h, w = H_ // 4, W_ // 4
    go = F32(1.0 if gout is None else gout)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w_ce = go / (F32(nv) * F32(n))
        w_var = go * F32(alpha) / (F32(H_ * W_) * F32(n))
        fl, lb = f.reshape(-1, Cc), lab.reshape(-1)
        lg = np.zeros((fl.shape[0], 16), F32)
        for k in range(15, -1, -1):
            for c in range(15, -1, -1):
                u = fl[:, c] - P[k, c]
                lg[:, k] -= u * u
        e = np.exp(lg - lg.max(1, keepdims=True))
        den = e[:, ::-1].sum(1, keepdims=True, dtype=F32)
        valid = (lb != ignore)[:, None]
        oh = (np.arange(16)[None, :] == lb[:, None]) & valid
        g = np.where(valid, e * (w_ce / den) - oh * (w_ce + w_var), F32(0)).astype(F32)
        gs = np.zeros((fl.shape[0], 1), F32)
        gm = np.zeros_like(fl)
        for k in range(15, -1, -1):
            gs[:, 0] += g[:, k]
            gm += g[:, k:k + 1] * P[k][None, :]
        df = (F32(-2) * (gs * fl - gm)).reshape(B, H_, W_, Cc)
        My, Mx = LC.lerp4(H_, h).astype(F32), LC.lerp4(W_, w).astype(F32)
        t = np.einsum("Xx,bYXc->bYxc", Mx, df).astype(F32)
        return np.einsum("Yy,bYxc->byxc", My, t).astype(F32)


@pytest.mark.parametrize("case", [c for c in FUSED if c[0] == "exact"], ids=case_id)
def test_exact_cases_are_exact(case):
    kind, pkind, gname, lkind, ignore = case
    f, lab, P = LC.fused_input(kind, pkind, gname, lkind, ignore)
    B, H_, W_, _ = f.shape
    for gout, alpha_on, _ in LC.SCALARS:
        nv, n, alpha, gout = fused_scalars(kind, lkind, lab, ignore, H_, W_, gout, alpha_on)
        de, _, parts = LC.head_bwd_ref(f, lab, P, nv, n, ignore, alpha, gout, bars=False, parts=True)
        lg = parts["logits"]
        top2 = np.sort(lg, 1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0] > 200).all(), "a class is not ahead by 200"
        assert (np.abs(lg) < 2 ** 14).all() and (lg * 16 == np.round(lg * 16)).all()
        go = 1.0 if gout is None else gout
        if nv > 0:
            w_ce, w_var = go / (nv * n), go * alpha / (H_ * W_ * n)
            assert w_ce in (2.0 ** -12, 2.0 ** -11) and w_var in (0.0, 2.0 ** -14, 2.0 ** -13)
            g = parts["glogits"] * 2.0 ** 14
            assert (g == np.round(g)).all() and set(np.unique(parts["glogits"])) <= {0.0, w_ce, -w_ce - w_var, -w_var}
            if alpha_on and lkind == "ten_percent":
                assert {w_ce, -w_ce - w_var, -w_var} <= set(np.unique(parts["glogits"])), "both label situations must occur"
        # every term wy wx df is a multiple of 2^-21 and the magnitudes a low-resolution element sums stay below 2^24 units
        df = parts["df"]
        unit = 2.0 ** -21
        assert (df * 2.0 ** 15 == np.round(df * 2.0 ** 15)).all()
        assert (PC.bilinear_bwd(np.abs(df), H_ // 4, W_ // 4) < 2 ** 24 * unit).all()
        assert (de / unit == np.round(de / unit)).all()
        got = head32(f, lab, P, nv, n, ignore, alpha, gout)
        assert PC.same(got, LC.store(de, "f32")).all(), "float32 in another order differs"
        assert (LC.store(de, "f32") == de).all()
        if lkind == "all_ignored":
            assert (de == 0).all()
        else:
            assert np.abs(de).max() > 2.0 ** -12 and (lab != ignore).any()
            if lkind == "image0_ignored":
                assert B >= 2 and (de[0] == 0).all() and (lab[0] == ignore).all()


@pytest.mark.parametrize("case", [c for c in FUSED if c[0] != "exact"], ids=case_id)
def test_float32_stays_inside_the_bars(case):
    kind, pkind, gname, lkind, ignore = case
    f, lab, P = LC.fused_input(kind, pkind, gname, lkind, ignore)
    B, H_, W_, _ = f.shape
    nv, n, alpha, gout = fused_scalars(kind, lkind, lab, ignore, H_, W_, 0.5, True)
    de, bar = LC.head_bwd_ref(f, lab, P, nv, n, ignore, alpha, gout)
    HC.check_close("float32 " + case_id(case), head32(f, lab, P, nv, n, ignore, alpha, gout), de, bar, False)


# ---------------------------------------------------------------------------------------------------------------------
# reach
# ---------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_what_its_name_claims():
    assert [LC.is_diagonal(LC.protos(k)) for k in ("eye", "diag", "gend", "general", "almost")] == [True, True, False, False, False]
    d = np.diag(LC.protos("diag"))
    assert (d < 0).any() and (d == 0).any() and np.signbit(LC.protos("diag")[0, 1])
    assert LC.protos("almost")[5, 9] == F32(2.0 ** -20)
    T = {g: LC.fused_tiles(*LC.GEOMS[g][1:]) for g in LC.GEOMS}
    assert T["every_clamp_1x1"] == T["one_row_1x14"] == T["one_column_7x1"] == T["one_tile_7x14"] == T["ragged_tile_6x13"] == (1, 1)
    assert T["second_tile_one_column_7x15"] == (1, 2) and LC.GEOMS["second_tile_one_column_7x15"][2] - LC.HB_TI == 1
    assert T["second_tile_one_row_8x14"] == (2, 1) and LC.GEOMS["second_tile_one_row_8x14"][1] - LC.HB_TJ == 1
    assert T["tiles_3x3_15x29"] == (3, 3) and T["exact_multiples_14x28_b3"] == (2, 2)
    B, h, w = LC.GEOMS["exact_multiples_14x28_b3"]
    assert B == 3 and h % LC.HB_TJ == 0 and w % LC.HB_TI == 0
    B, h, w = LC.GEOMS["one_tile_7x14"]
    assert 4 * 0 - 2 < 0 and 4 * h + 2 > 4 * h - 1 and (h, w) == (LC.HB_TJ, LC.HB_TI)    # the tile's halo rows and groups lie outside
    B, h, w = LC.GEOMS["ragged_tile_6x13"]
    assert h < LC.HB_TJ and w < LC.HB_TI
    for g, (B, h, w) in LC.GEOMS.items():
        i0, i1, _, _, _ = PC.src_index(4 * w, w)
        assert (i1 == i0).all() == (w == 1)
    trips = LC.cases_reach()
    assert set(trips) == set(LC.BIG_REACH) and all(t >= 2 for t in trips.values())
    for name, B, K, H_, W_ in [c[:5] for c in LC.BIG_CASES]:
        assert K == 2 and B * H_ * W_ * (K * 4 * 2 + 8) < 210e6
    assert {(c[3] * c[4]) % 4 for c in LC.LOSS_CASES if c[0].startswith("hw") and c[3] <= 6} == {0, 1, 2, 3}
    f, lab, ref_lab, P, must = LC.fused_nonfinite("eye", np.nan)
    assert must.sum() == 4 and (lab != ref_lab).sum() == 1
    f, _, _ = LC.fused_input("big", "eye", "tiles_3x3_15x29")
    _, _, parts = LC.head_bwd_ref(f, np.zeros(f.shape[:3], np.int64), P, 1.0, 1.0, 255, 0.0, None, bars=False, parts=True)
    lg = parts["logits"]
    assert (lg - lg.max(1, keepdims=True)).min() < -1000                         # exp underflows to exactly 0 in float32 below -104


# ---------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------
def mutant_rejected(case, mut, alpha_on=True):
    kind, pkind, gname, lkind, ignore = case
    f, lab, P = LC.fused_input(kind, pkind, gname, lkind, ignore)
    nv, n, alpha, gout = fused_scalars(kind, lkind, lab, ignore, f.shape[1], f.shape[2], 0.5, alpha_on)
    de, bar = LC.head_bwd_ref(f, lab, P, nv, n, ignore, alpha, gout, bars=kind != "exact")
    bad, _ = LC.head_bwd_ref(f, lab, P, nv, n, ignore, alpha, gout, bars=False, mut=mut)
    return rejected(lambda: HC.check_close(mut, LC.store(bad, "f32"), LC.store(de, "f32") if kind == "exact" else de, bar, kind == "exact"))


@pytest.mark.parametrize("gname", list(LC.GEOMS))
def test_the_fused_reference_has_teeth(gname):
    wide = LC.GEOMS[gname][2] >= 2
    for case in (("exact", "eye", gname, "ten_percent", 255), ("exact", "gend", gname, "ten_percent", 255),
                 ("real", "eye", gname, "ten_percent", 255), ("real", "general", gname, "ten_percent", 255)):
        assert mutant_rejected(case, "no_wvar"), case
        assert mutant_rejected(case, "swap_lr") == wide, case
        assert mutant_rejected(case, "clamp_x1") == wide, case
    exact = ("exact", "diag", gname, "ten_percent", 255)
    assert not mutant_rejected(exact, "no_wvar", alpha_on=False)                # alpha = 0: nothing to drop
    assert mutant_rejected(exact, "swap_lr", alpha_on=False) == wide


def test_the_loss_reference_has_teeth():
    case = [c for c in LC.LOSS_CASES if c[0] == "hw0_6x10"][0]
    lg, lab = LC.loss_input(case, "close")
    ref = LC.loss_ref(lg, lab, 255, 0.01, 2.0, 0.5)
    bad = LC.loss_ref(lg, lab, 255, 0.01, 2.0, 0.5, bars=False, mut="no_wvar")
    assert rejected(lambda: LC.compare("no_wvar", bad["grad"], ref["grad"], ref["gbar"]))
    LC.compare("itself", ref["grad"].astype(F32), ref["grad"], ref["gbar"])
