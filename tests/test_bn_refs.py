"""CPU: the float64 definitions, input generators and error bars of tests/bn_cases.py are right on exactly the inputs
tests/test_gpu_bn_edges.py uses -- so that a failure there is the kernel's.

  * the definitions equal float64 autograd of F.batch_norm (training, and training=False for the fixed-statistics backward);
  * the Chan merge of float64 group partials equals numpy's variance of the whole matrix;
  * the exact cases are exact: every intermediate of the contract is a float32 value and every partial sum stays below 2^24 units;
  * a plain float32 evaluation of each formula, contracted (FMA) and not, stays inside its bar on the real-valued inputs;
  * no more than 1 element in 10 000 has a ReLU / mask decision inside its bar;
  * every plane-scale bound the GPU tests expect a scale from is further than 1e-4 from a power of two.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as CS

F32, F64 = np.float32, np.float64


def is32(x):
    x = np.asarray(x, F64)
    return bool((x.astype(F32).astype(F64) == x).all())


def fma32(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 values is exact, the sum is rounded once"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------------
# definitions against autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,N", CS.REAL_SHAPES)
@pytest.mark.parametrize("relu,res", [(1, True), (1, False), (0, False)])
def test_definitions_equal_float64_autograd(M, N, dtype, relu, res):
    d = CS.real_inputs(M, N, dtype)
    y, r = t64(d["y"], True), t64(d["res"], True) if res else None
    gamma, beta = t64(d["gamma"], True), t64(d["beta"], True)
    o = F.batch_norm(y, None, None, gamma, beta, training=True, eps=CS.BN_EPS)
    if res:
        o = o + r
    if relu:
        o = F.relu(o)
    (o * t64(d["dz"])).sum().backward()
    mean, var = CS.batch_stats(d["y"])
    invstd = 1.0 / np.sqrt(var + CS.BN_EPS)
    z, pre = CS.fwd_ref(d["y"], d["res"] if res else None, mean, d["gamma"].astype(F64) * invstd, d["beta"], relu)
    g = CS.bwd_g(d["dz"], (z > 0) if relu else None, 1.0)
    sums = CS.bwd_sums(g, d["y"], mean, invstd)
    dy = CS.bwd_apply_ref(g, d["y"], CS.bwd_coef(sums, d["gamma"], mean, invstd, M))

    def close(got, ref, what):
        ref = ref.detach().numpy()
        tol = 1e-8 * np.abs(ref).max(0) + 1e-12
        assert (np.abs(got - ref) <= tol).all(), what

    close(z, o, "z")
    close(dy, y.grad, "dy")
    close(sums[1], gamma.grad, "dgamma")
    close(sums[0], beta.grad, "dbeta")
    if res:
        close(g, r.grad, "dres")


def test_fixed_statistics_backward_adds_the_parameter_gradients():
    """M = 0 of dml_bn_bwd_finalize: float64 autograd of F.batch_norm(training=False) has coef1 = coef2 = 0 and dgamma = sum g xhat,
    dbeta = sum g with xhat from the running statistics -- the sums ARE added (the kernel's behaviour, the header's corrected text)"""
    M, N = CS.REAL_SHAPES[0]
    d = CS.real_inputs(M, N, "f32")
    rs = np.random.RandomState(3)
    rm, rv = rs.standard_normal(N), rs.uniform(0.5, 2.0, N)
    y, gamma, beta = t64(d["y"], True), t64(d["gamma"], True), t64(d["beta"], True)
    o = F.relu(F.batch_norm(y, t64(rm), t64(rv), gamma, beta, training=False, eps=CS.BN_EPS))
    (o * t64(d["dz"])).sum().backward()
    invstd = 1.0 / np.sqrt(rv + CS.BN_EPS)
    z, _ = CS.fwd_ref(d["y"], None, rm, d["gamma"].astype(F64) * invstd, d["beta"], 1)
    g = CS.bwd_g(d["dz"], z > 0, 1.0)
    sums = CS.bwd_sums(g, d["y"], rm, invstd)
    coef = CS.bwd_coef(sums, d["gamma"], rm, invstd, 0)
    assert (coef[1] == 0).all() and (coef[2] == 0).all()
    for got, ref in ((CS.bwd_apply_ref(g, d["y"], coef), y.grad), (sums[1], gamma.grad), (sums[0], beta.grad)):
        ref = ref.numpy()
        assert (np.abs(got - ref) <= 1e-9 * np.abs(ref).max(0) + 1e-12).all()
    assert np.abs(sums).max() > 1.0               # "unchanged" would be visibly different


@pytest.mark.parametrize("stat_rows", [64, 48])
def test_chan_merge_equals_numpy_variance(stat_rows):
    ys = [CS.real_inputs(M, N, "f32")["y"] for M, N in CS.REAL_SHAPES] + [CS.sync_inputs().reshape(-1, CS.SYNC_N)]
    for y in ys:
        cnt, mean, m2 = CS.chan_merge(CS.partials(y, stat_rows), CS.group_rows(y.shape[0], stat_rows))
        y64 = y.astype(F64)
        assert (cnt == y.shape[0]).all()
        assert (np.abs(mean - y64.mean(0)) <= 1e-14 * np.abs(y64).max(0)).all()
        var = y64.var(0)
        assert (np.abs(m2 / cnt - var) <= 1e-13 * (var + y64.mean(0) ** 2 * 1e-3)).all()
    # the merge of the three ranks' moments is the same thing
    y = CS.sync_inputs()
    part = np.stack([[r.astype(F64).sum(0), ((r - r.astype(F64).mean(0)) ** 2).sum(0)] for r in y]).transpose(0, 2, 1)
    cnt, mean, m2 = CS.chan_merge(part, [CS.SYNC_M_EACH] * CS.SYNC_RANKS)
    allv = y.reshape(-1, CS.SYNC_N).astype(F64)
    assert (np.abs(m2 / cnt - allv.var(0)) <= 1e-12 * allv.var(0)).all()
    means, within = y.astype(F64).mean(1), y.astype(F64).std(1).max(0)
    assert (np.abs(means[0] - means[1]) > 20 * within).all() and (np.abs(means[1] - means[2]) > 20 * within).all()


# ---------------------------------------------------------------------------------------------------------------------
# the exact cases are exact
# ---------------------------------------------------------------------------------------------------------------------
def _exact_shapes():
    out = set()
    for dt in ("f32", "bf16"):
        out.update(CS.apply_shapes(dt))
        out.update(CS.reduce_shapes(dt))
        out.update((N, M) for N, M, _ in CS.SLICES[dt])
    out.update(CS.PLANES_SHAPES)
    out.update(CS.BWD_APPLY_SHAPES)
    return sorted(out)


@pytest.mark.parametrize("N,M", _exact_shapes())
def test_exact_inputs_are_exact(N, M):
    for fine in (False, True):
        d = CS.exact_inputs(M, N, fine_res=fine)
        for k in ("y", "res", "dz", "dres0"):
            assert is32(d[k]) and ((fine and k == "res") or (CS.bf16_round(d[k].astype(F32)) == d[k]).all())
        # forward: every intermediate is a float32 value, so any contraction gives the float64 result
        t1 = d["y"] - d["mean"]
        t2 = t1 * d["scale"]
        t3 = t2 + d["shift"]
        t4 = t3 + d["res"]
        assert all(is32(t) for t in (t1, t2, t3, t4, 2 * t3, 2 * t4))
        e = (d["y"].astype(F32) - d["mean"].astype(F32)) * d["scale"].astype(F32) + d["shift"].astype(F32)
        assert (e.astype(F64) == t3).all() and ((e + d["res"].astype(F32)).astype(F64) == t4).all()
        assert (fma32(t1, d["scale"], d["shift"]).astype(F64) == t3).all()
        if not fine:                               # bf16 outputs hold the exact value too (8 bits), with and without dropout's 2
            assert (CS.store(t4, "bf16") == t4).all() and (CS.store(2 * t3, "bf16") == 2 * t3).all()
        z, _ = CS.fwd_ref(d["y"], d["res"], d["mean"], d["scale"], d["shift"], 1)
        assert (z == 0).any() and (z[0, 0] == 0) and (d["scale"] < 0).any()
        # backward: terms are multiples of 2^-4 and a partial of RED_MAX_ROWS rows stays below 2^24 of them
        g = CS.bwd_g(d["dz"], z > 0, CS.GSCALE)
        xc = d["y"] - d["mean"]
        term = g * xc * d["invstd"]
        assert is32(g) and is32(g * xc) and is32(term) and (term * 16 == np.round(term * 16)).all()
        assert np.abs(term).max() * CS.RED_MAX_ROWS * 16 < 2 ** 24 and np.abs(g).max() * CS.RED_MAX_ROWS * 16 < 2 ** 24
        gf = g.astype(F32)
        assert ((gf * xc.astype(F32) * d["invstd"].astype(F32)).astype(F64) == term).all()
        # backward apply
        c = d["coef"]
        a1, a2 = c[0] * CS.GSCALE, (d["y"] - c[3])
        parts = (a1, a1 * d["dz"], a2, c[1] * a2, a1 * d["dz"] + c[1] * a2, a1 * d["dz"] + c[1] * a2 + c[2], g + d["dres0"])
        assert all(is32(p) for p in parts)


def test_exact_sums_stay_exact_for_every_case():
    """the float64 sums of the whole tensor are float32 values (the kernel's partial rows are added in float64 by the test)"""
    for N, M in _exact_shapes():
        d = CS.exact_inputs(M, N)
        z, _ = CS.fwd_ref(d["y"], d["res"], d["mean"], d["scale"], d["shift"], 1)
        s = CS.bwd_sums(CS.bwd_g(d["dz"], z > 0, CS.GSCALE), d["y"], d["mean"], d["invstd"])
        assert (s * 16 == np.round(s * 16)).all()


# ---------------------------------------------------------------------------------------------------------------------
# float32 evaluations stay inside the bars
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,N", CS.REAL_SHAPES)
def test_float32_evaluations_stay_inside_the_bars(M, N, dtype):
    d = CS.real_case(M, N, dtype)
    y, r, mu, sc, sh = d["y"], d["res"], d["mean"], d["scale"], d["shift"]
    excluded = 0
    for res in (None, r):
        z, pre = CS.fwd_ref(y, res, mu, sc, sh, 1)
        bar = CS.apply_bar(y, res, mu, sc, sh, dtype)
        t = (y - mu) * sc + sh                                       # float32 throughout
        u = fma32(y - mu, sc, sh)
        if res is not None:
            t, u = t + res, u + res
        for ev in (t, u):
            out = CS.store(np.maximum(ev, 0), dtype) if dtype == "bf16" else np.maximum(ev, 0)
            assert (np.abs(out.astype(F64) - z) <= CS.stored_bar(bar, z, dtype)).all()
            decided = np.abs(pre) > bar
            assert ((ev > 0) == (pre > 0))[decided].all()
        excluded = max(excluded, int((np.abs(pre) <= bar).sum()))
    assert excluded <= CS.EXCLUDE_CAP * M * N, excluded
    # backward: sums of one partial of M rows, and the apply
    z, _ = CS.fwd_ref(y, r, mu, sc, sh, 1)
    on = z > 0
    g = CS.bwd_g(d["dz"], on, CS.GSCALE)
    ref = CS.bwd_sums(g, y, mu, d["invstd"])
    bars = CS.reduce_bars(g, y, mu, d["invstd"], M)
    gf = np.where(on, d["dz"] * F32(CS.GSCALE), F32(0))
    term = gf * (y - mu) * d["invstd"]
    for s0, s1 in ((np.add.reduce(gf, 0), np.add.reduce(term, 0)), (np.cumsum(gf, 0)[-1], np.cumsum(term, 0)[-1])):
        assert (np.abs(s0.astype(F64) - ref[0]) <= bars[0]).all() and (np.abs(s1.astype(F64) - ref[1]) <= bars[1]).all()
    acc = np.zeros(N, F32)
    for m in range(M):                                               # contracted: sgx = fma(g (y - mu), is, sgx)
        acc = fma32(gf[m] * (y[m] - mu), d["invstd"], acc)
    assert (np.abs(acc.astype(F64) - ref[1]) <= bars[1]).all()
    coef = CS.bwd_coef(ref, d["gamma"], mu, d["invstd"], M).astype(F32)
    dy = CS.bwd_apply_ref(g, y, coef)
    bar = CS.bwd_apply_bar(g, y, coef, CS.GSCALE)
    gm = np.where(on, d["dz"], F32(0))
    cA = coef[0] * F32(CS.GSCALE)
    plain = cA * gm + coef[1] * (y - coef[3]) + coef[2]
    fused = fma32(coef[1], y - coef[3], fma32(cA, gm, 0.0)) + coef[2]
    fused2 = fma32(cA, gm, fma32(coef[1], y - coef[3], coef[2]))
    for ev in (plain, fused, fused2):
        out = CS.store(ev, dtype) if dtype == "bf16" else ev
        assert (np.abs(out.astype(F64) - dy) <= CS.stored_bar(bar, dy, dtype)).all()


@pytest.mark.parametrize("M", CS.STATS_MS)
def test_stats_bars_hold_a_float32_two_pass(M):
    for N in CS.STATS_NS:
        for dtype in ("f32", "bf16"):
            y = CS.stats_inputs(M, N, dtype)
            ref = CS.partials(y, CS.STAT_ROWS)
            sb, mb = CS.stats_bars(y)
            for g, n in enumerate(CS.group_rows(M, CS.STAT_ROWS)):
                blk = y[g * 64:(g + 1) * 64]
                s = np.zeros(N, F32)
                for row in blk:
                    s = s + row
                mean = s / F32(n)
                for contracted in (False, True):
                    m2 = np.zeros(N, F32)
                    for row in blk:
                        dd = row - mean
                        m2 = fma32(dd, dd, m2) if contracted else m2 + dd * dd
                    assert (np.abs(s.astype(F64) - ref[g, :, 0]) <= sb[g]).all()
                    assert (np.abs(m2.astype(F64) - ref[g, :, 1]) <= mb[g]).all()
                if n == 1:
                    assert (ref[g, :, 1] == 0).all()


def test_finalize_reference_is_consistent():
    """the Chan merge of the hand-built float32 partials against the kernel's own identity Q + P - S^2 / M evaluated with Python's
    exact rationals would be the same number: checked here in float64 with the bar's cancellation term"""
    for G in CS.FIN_GS[:7]:
        for sr, N, ragged, mom, null in CS.fin_combos(G):
            part, rows, M = CS.hand_partials(G, N, sr, ragged)
            cnt, mean, m2 = CS.chan_merge(part, rows)
            assert (cnt == M).all()
            p = part.astype(F64)
            S, Q, P = p[:, :, 0].sum(0), p[:, :, 1].sum(0), (p[:, :, 0] ** 2 / rows[:, None]).sum(0)
            ref = CS.finalize_ref(M, mean, m2, None, None, None, None, mom)
            var = m2 / M
            assert (np.abs((Q + (P - S * S / M)) / M - var) <= ref["cancel"] * (var + CS.BN_EPS)).all()
            if M == 1:
                assert (mean == p[0, :, 0]).all() and (ref["invstd"] == 1.0 / np.sqrt(F64(F32(CS.BN_EPS)))).all()
    assert abs(CS.hand_partials(64, 5, 64, True)[0][:, 0, 0].astype(F64).sum() / CS.hand_partials(64, 5, 64, True)[2]) > 1e3


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def test_bounds_are_far_from_a_power_of_two():
    bs = [CS.fwd_bound_of(c) for c in CS.fwd_bound_cases().values()] + [CS.bwd_bound_of(c) for c in CS.bwd_bound_cases().values()]
    for G, N, sr, mult, at in CS.FUSED_CASES:
        for small in (False, True):
            gamma, beta = CS.bound_params(N, small=small)
            part, rows, M = CS.hand_partials(G, N, sr, True)
            bs.append(CS.fwd_bound(gamma, beta, N, M, mult, 0.0 if at is None else CS.FUSED_RES_MAX))
    for nb, N in CS.BWD_FUSED_CASES:
        bs += [CS.bwd_fused_case(nb, N, f)[2] for f in (1.0, 2.0 ** -8)]
    for Ns in CS.MULTI_CASES:
        bs.append(max(CS.fwd_bound(*CS.bound_params(N, seed=i), N, 297 * (i + 1), 1.0 + i) for i, N in enumerate(Ns)))
    for M in CS.REACH_MS:
        y, dz, gamma, beta = CS.reach_case(M)
        bs.append(CS.fwd_bound(gamma, beta, y.shape[1], M))
    finite = [b for b in bs if b != 0 and np.isfinite(b)]
    assert len(finite) == len(bs) - 2                                 # all-zero parameters and the infinite gamma
    assert all(CS.bound_margin(b) > 1e-4 for b in finite), [CS.bound_margin(b) for b in finite]
    assert CS.unscale_of_bound(0.0) == 1.0 and CS.unscale_of_bound(np.inf) == 1.0 and CS.unscale_of_bound(np.nan) == 1.0
    assert CS.unscale_of_bound(2.0 ** 14) == 1.0 and CS.unscale_of_bound(2.0 ** 14 * 0.9985) == 0.5


def test_the_reach_case_reaches_the_top_binade_of_its_bound():
    """|xhat| of the ones is sqrt(M - 1) (up to eps): with M = 297 the largest |z| lies in the top binade of the scaled range, so a
    bound that were a factor 2 smaller would overflow the planes"""
    for M in CS.REACH_MS:
        y, dz, gamma, beta = CS.reach_case(M)
        mean, var = CS.batch_stats(y)
        invstd = 1.0 / np.sqrt(var + CS.BN_EPS)
        z, _ = CS.fwd_ref(y, None, mean, gamma.astype(F64) * invstd, beta, 0)
        xhat = (y[M // 2] - mean) * invstd
        assert (np.abs(xhat - np.sqrt(max(M - 1, 1))) < 2e-3 * np.sqrt(M)).all()
        b = CS.fwd_bound(gamma, beta, y.shape[1], M)
        un = CS.unscale_of_bound(b)
        assert np.abs(z).max() <= b and np.abs(z).max() / un < 2 ** 15
        if M > 2:
            assert np.abs(z).max() / un >= 2 ** 14


def test_planes_and_mask_helpers():
    x = np.array([0.0, 1.0, -3.0009765625, 1000.123, 6.1e-5, 32752.0], F32)
    hi, lo = CS.h2_planes(x, 0.5)
    rec = (hi.astype(F64) + lo.astype(F64)) * 0.5
    assert (np.abs(rec - x) <= 2.0 ** -21 * np.abs(x) + 2.0 ** -25 * 0.5).all() and (lo != 0).any() and np.isinf(CS.h2_planes(x, 0.25)[0][-1])
    on = np.random.RandomState(0).rand(5, 16) < 0.5
    for V in (4, 8):
        m = CS.pack_mask(on, V)
        assert m.shape == (5, 16 // V) and (CS.unpack_mask(m, V) == on).all()
        assert m[2, 1] == sum(int(on[2, V + q]) << q for q in range(V))
    assert (CS.bf16_round(np.array([1.00390625, 1.01171875, -3.0], F32)) == np.array([1.0, 1.015625, -3.0], F32)).all()
