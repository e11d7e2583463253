"""GPU: the loss end of the backward at its edges, through the C ABI -- dml_loss_fwd / dml_loss_finalize / dml_loss_bwd
(csrc/dml_loss.hip) and dml_head_bwd_fused (csrc/head.hip) on every case of tests/loss_cases.py.

Every comparison is against the float64 definitions of tests/loss_cases.py on the same float32 inputs (proved right on these inputs,
without a GPU, by tests/test_loss_refs.py) and goes through head_cases.check_close.  Exact (dyadic) inputs of the fused kernel must be
reproduced EXACTLY -- the float64 result rounded once to float32, or once (to nearest even) to bfloat16; real-valued inputs per element
against bars that count the float32 roundings of the contract.  The counts sums[1] and sums[3] are compared as integers.  Every output
(de, glogits, sums, block_partials, the loss) sits between two guard regions of 0xAA bytes, each longer than a row of the output, which
must be bitwise unchanged afterwards; feats, logits, labels, protos and the sums a backward reads must be bitwise unchanged too.  The
fused kernel and dml_loss_bwd get their sums from the test, as exact doubles; chained cases (the fused kernel on two geometries, dml_loss_bwd
on one) take them from dml_loss_fwd, as the plan does.  On every real case the unfused chain (dml_loss_bwd -> dml_proto_dist_bwd -> dml_bilinear_bwd) must lie
inside the same bars of the same float64 result.  Each float check prints "MEASURE <what> err=<error> bar=<its bar>" for the element
that takes the largest share of its bar (run with -s to see the figures).

Non-finite inputs.  A NaN or +inf feature at one pixel makes exactly the <= 2 x 2 low-resolution pixels it interpolates into
non-finite (all 16 channels) and leaves every other element inside its bar.  A NaN logit makes the loss and exactly that pixel's K
gradients NaN.  One -inf logit beside finite ones (plane 0, the last plane) gives the float64 definition's finite loss and a gradient
of exactly 0 in that plane.

Measured on the MI355X (the whole file, 70 tests, takes about 6 s there; the slowest tests, the 513 x 513 case and the vector
backward above its cap, 1.3 s each), as the largest share of its bar, error of bar:
  exact cases (de float32 and bfloat16, every geometry, prototype kind and set of scalars)   all equal
  fused, real inputs   float32 3.7e-10 of 3.0e-8 (1.2 %), the 30 N features 1.1e-7 of 1.7e-5 (0.7 %); bfloat16 9.75e-4 of 9.93e-4
  unfused chain        float32 2.0e-10 of 2.1e-8 (0.9 %); bfloat16 as the fused kernel, element for element
  dml_loss_bwd         1.8e-11 of 2.1e-10 (9 %) on the close regime; half of TINY-sized bars where float32 underflows
  sums[0] / sums[2]    4.4e-4 of 6.7e-3 (7 %, K = 40) / 2.2e-5 of 3.6e-4 (6 %);  loss 9.1e-6 of 1.5e-4 (6 %)
  focal, -inf logit    the sum 9.9e-5 of 2.4e-2, the loss 2.1e-6 of 3.4e-4; the gradient inside focal_cases's bars, 0 in the plane
  counts               sums[1], sums[3] (ties: the first maximum) and sums[4] equal as integers everywhere
The fused kernel's float32 bar is about 225 eps32 times the magnitude sum on the real inputs (110 of them the counted roundings, the
rest the softmax term) and a worst case: the kernel's errors do not all point the same way.  What is sharp here are the exact cases
(any wrong weight, halo or scalar moves an element by 2^-21 or more) and the bfloat16 comparison; the record below says what each
catches.

Found by this file and fixed in the kernels (the library as it was before fails exactly these 12 tests, and nothing else here):
  * loss_fwd_kernel / loss_bwd_kernel (dml_loss.hip) and focal_lse_step (focal_loss.hip): a -inf logit in plane 0 met the running
    maximum's initial -inf in the `else` branch, exp(-inf + inf) = NaN: loss and gradient NaN where float64 is finite
    (test_loss_small_cases[neg_inf_plane0_*], test_focal_loss_with_one_neg_inf_logit[*-neg_inf_plane0]).  The branch now adds 1 when
    v == mx.  The fused kernel's general path takes the maximum first (fmaxf) and never had the pattern.
  * head_bwd_fused_c16_kernel multiplied all three column partials, the one with weight zero too: a NaN or inf feature reached a
    third low-resolution column it does not interpolate into, 32 elements (test_fused_nonfinite_feature_reaches_its_neighbours_only,
    all 8).  The zero-weight partial is now skipped.  Train step before / after, 768 x 768 x 16, two runs each: 76.61 / 76.54 ms and
    76.52 / 76.56 ms.

Tried on scratch builds of head.hip / dml_loss.hip, one line at a time (arithmetic only, no address moves), and the tests of this
file that failed:
  wl / wr swapped                          26: exact and real on the 7 geometries with w >= 2 (w = 1 has one column), label kinds,
                                               after-the-forward, all non-finite cases
  p_hi of the right halo group 2 -> 4      none, and none can: pixels 2 and 3 of that group reach columns q and q + 1, both outside
                                               the tile; what they add lands in the halo column of the LDS buffer, which phase 2 never
                                               reads.  The change costs time, not correctness
  `- dk[k]` dropped (diagonal logits)      9: the real cases of every geometry ("diag": its entries differ; with 3 I every logit
                                               moves by the same 9 and the softmax is unchanged -- correctly not a failure; the exact
                                               cases keep their 200 margin)
  w_var dropped, diagonal path             24: every exact and real geometry, label kinds, non-finite with 3 I
  w_var dropped, general path              26: the same, after-the-forward, non-finite with the general matrix
  w_var dropped, loss_bwd_kernel           44: every dml_loss_bwd case and the unfused chain of every real fused case
  `>` -> `>=` in loss_fwd_kernel           4: ties_hw0, ties_hw3 (sums[3]) and neg_inf_plane0 (hw0, hw3)
  inv_hw omitted in loss_sum_kernel        30: every forward case (sums[2], loss)
"""
import functools

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import head_cases as HC
import loss_cases as LC

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 4096                                   # guard elements before and after: more than a row of any output here
TYPES = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2), "f64": (torch.float64, 8)}
DT = {"f32": 0, "bf16": 1}
EINVAL, EUNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def measure(what, seen):
    print("MEASURE %s err=%.3e bar=%.3e" % ((what,) + tuple(seen)))


class Out:
    """GUARD elements, n elements, GUARD elements on the device, every byte 0xAA"""

    def __init__(self, n, dtype="f32", guard=GUARD):
        self.n, self.g = n, guard
        self.tdt, self.esize = TYPES[dtype]
        self.raw = torch.full(((2 * guard + n) * self.esize,), 0xAA, dtype=torch.uint8, device="cuda")
        self.body = self.raw.view(self.tdt)[guard:guard + n]
        self.ptr = self.body.data_ptr()

    def get(self, shape):
        return self.body.to(torch.float64 if self.tdt == torch.float64 else torch.float32).cpu().numpy().reshape(shape)

    def bits(self):
        lo = self.g * self.esize
        return self.raw[lo:lo + self.n * self.esize].clone()

    def untouched(self):
        lo, hi = self.g * self.esize, (self.g + self.n) * self.esize
        assert bool((self.raw[:lo] == 0xAA).all()) and bool((self.raw[hi:] == 0xAA).all()), "a byte outside the output was written"

    def all_aa(self):
        return bool((self.raw == 0xAA).all())


class Frozen:
    """device copies of the inputs: same() asserts that no bit of them changed"""

    def __init__(self, **arrays):
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.t = {k: dev(v) for k, v in self.host.items()}

    def __getitem__(self, k):
        return self.t[k].data_ptr()

    def same(self):
        for k in self.t:
            now = self.t[k].cpu().numpy()
            assert np.array_equal(now.reshape(-1).view(np.uint8), self.host[k].reshape(-1).view(np.uint8)), "the input %s was written" % k


def sums_for(nv, n, s0=0.0, s2=0.0, s3=0.0):
    return np.array([s0, nv, s2, s3, n], F64)


# ---------------------------------------------------------------------------------------------------------------------
# dml_head_bwd_fused
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def fused_ref(case, gout, alpha_on):
    """(inputs, scalars, float64 de, float32 bar or None, parts) -- once per case and set of scalars"""
    kind, pkind, gname, lkind, ignore = case
    f, lab, P = LC.fused_input(kind, pkind, gname, lkind, ignore)
    nv, n, alpha, gout = LC.fused_scalars(kind, lkind, lab, ignore, f.shape[1], f.shape[2], gout, alpha_on)
    de, bar, parts = LC.head_bwd_ref(f, lab, P, nv, n, ignore, alpha, gout, bars=kind != "exact", parts=True)
    return f, lab, P, (nv, n, alpha, gout), de, bar, parts


def call_fused(lib, inp, out, B, h, w, ignore, alpha, n_arg, dname, gout_t):
    return lib.dml_head_bwd_fused(inp["feats"], inp["labels"], inp["sums"], None if gout_t is None else gout_t.data_ptr(), inp["protos"],
                                  out.ptr, B, h, w, 16, 16, 4 * h, 4 * w, ignore, alpha, n_arg, DT[dname], st())


def run_fused(lib, case, scal=LC.SCALARS[0], dnames=("f32", "bf16"), chain=True):
    kind, pkind, gname, lkind, ignore = case
    gout0, alpha_on, n_passed = scal
    f, lab, P, (nv, n, alpha, gout), de, bar, parts = fused_ref(case, gout0, alpha_on)
    B, Hh, Ww, _ = f.shape
    h, w = Hh // 4, Ww // 4
    exact = kind == "exact"
    inp = Frozen(feats=f, labels=lab, protos=P, sums=sums_for(nv, n))
    gout_t = None if gout is None else torch.tensor(gout, dtype=torch.float32, device="cuda")
    what = "fused %s gout=%s alpha=%g n_passed=%d" % ("-".join(str(v) for v in case), gout, alpha, n_passed)
    for dname in dnames:
        out = Out(B * h * w * 16, dname)
        chk(call_fused(lib, inp, out, B, h, w, ignore, alpha, n if n_passed else 0.0, dname, gout_t))
        got = out.get(de.shape)
        if exact:
            HC.check_close(what + " " + dname, got, LC.store(de, dname), None, True)
        else:
            measure(what + " " + dname, HC.check_close(what + " " + dname, got, de, LC.stored_bar(bar, de, dname), False))
        if lkind == "all_ignored":
            assert (got == 0).all(), what + ": w_ce = inf leaked"
        out.untouched()
        first = out.bits()
        out2 = Out(B * h * w * 16, dname)
        chk(call_fused(lib, inp, out2, B, h, w, ignore, alpha, n if n_passed else 0.0, dname, gout_t))
        assert torch.equal(first, out2.bits()), what + ": two launches differ"
        if chain and not exact:
            lg = Frozen(logits=parts["logits"].astype(F32))
            gl, df, de2 = Out(B * 16 * Hh * Ww), Out(B * Hh * Ww * 16), Out(B * h * w * 16, dname)
            chk(lib.dml_loss_bwd(lg["logits"], inp["labels"], inp["sums"], None if gout_t is None else gout_t.data_ptr(), gl.ptr, B, 16, Hh, Ww,
                                 ignore, alpha, n if n_passed else 0.0, st()))
            chk(lib.dml_proto_dist_bwd(gl.ptr, None, inp["feats"], inp["protos"], df.ptr, B, 16, 16, Hh, Ww, st()))
            chk(lib.dml_bilinear_bwd(df.ptr, de2.ptr, B, h, w, Hh, Ww, 16, 16, 16, DT[dname], 1, 0, st()))
            measure(what + " chain " + dname, HC.check_close(what + " chain " + dname, de2.get(de.shape), de, LC.stored_bar(bar, de, dname), False))
            for o in (gl, df, de2):
                o.untouched()
            lg.same()
    inp.same()


@pytest.mark.parametrize("gname", list(LC.GEOMS))
def test_fused_exact_inputs_are_reproduced_exactly(lib, gname):
    """3 I, a dyadic diagonal and a dyadic general matrix; gout given and NULL, alpha on and 0, n_images passed and read from sums[4];
    float32 and bfloat16 de: equal to the float64 result rounded once"""
    for case in [c for c in LC.fused_cases() if c[0] == "exact" and c[2] == gname and c[3] == "ten_percent" and c[4] == 255]:
        for scal in LC.SCALARS:
            run_fused(lib, case, scal)


@pytest.mark.parametrize("gname", list(LC.GEOMS))
def test_fused_real_inputs_and_the_unfused_chain(lib, gname):
    """both arithmetic paths (3 I and a diagonal with a negative and a zero entry: the closed form; a general and an almost diagonal
    matrix: the general path), the 30 N features on the 3 x 3 tiles; the unfused chain inside the same bars"""
    for case in [c for c in LC.fused_cases() if c[0] != "exact" and c[2] == gname and c[3] == "ten_percent" and c[4] == 255]:
        run_fused(lib, case)
        if case[1] in ("eye", "general"):
            for scal in LC.SCALARS[1:]:
                run_fused(lib, case, scal, dnames=("f32",))


@pytest.mark.parametrize("lkind,ignore", [("image0_ignored", -1), ("all_ignored", 255), ("ten_percent", -1)])
def test_fused_label_kinds(lib, lkind, ignore):
    """an image without a valid pixel beside valid ones; no valid pixel at all (sums[1] = 0, w_ce = inf: de exactly 0); ignore_index -1"""
    for case in [c for c in LC.fused_cases() if c[3] == lkind and c[4] == ignore]:
        run_fused(lib, case)


@pytest.mark.parametrize("gname", ["one_row_1x14", "tiles_3x3_15x29"])
def test_fused_with_the_sums_of_the_forward(lib, gname):
    """the plan's chain: dml_loss_fwd's sums (on the float32 logits of the definition) go into the fused kernel unchanged"""
    case = ("real", "general", gname, "ten_percent", 255)
    f, lab, P, (nv, n, alpha, gout), de, bar, parts = fused_ref(case, 0.5, True)
    B, Hh, Ww, _ = f.shape
    h, w = Hh // 4, Ww // 4
    inp = Frozen(feats=f, labels=lab, protos=P, logits=parts["logits"].astype(F32))
    sums, part = Out(5, "f64"), Out(LC.MAX_BLOCKS * 4)
    chk(lib.dml_loss_fwd(inp["logits"], inp["labels"], sums.ptr, part.ptr, B, 16, Hh, Ww, 255, st()))
    assert sums.get((5,))[1] == nv
    gout_t = torch.tensor(gout, dtype=torch.float32, device="cuda")
    out = Out(B * h * w * 16)
    before = sums.bits()
    chk(lib.dml_head_bwd_fused(inp["feats"], inp["labels"], sums.ptr, gout_t.data_ptr(), inp["protos"], out.ptr, B, h, w, 16, 16, Hh, Ww, 255,
                               alpha, n, 0, st()))
    assert torch.equal(before, sums.bits()), "dml_head_bwd_fused wrote sums"
    measure("fused after dml_loss_fwd " + gname, HC.check_close("fused after dml_loss_fwd", out.get(de.shape), de, bar, False))
    for o in (sums, part, out):
        o.untouched()
    inp.same()


@pytest.mark.parametrize("X", LC.NONFINITE_X)
@pytest.mark.parametrize("pkind", ["eye", "general"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_fused_nonfinite_feature_reaches_its_neighbours_only(lib, pkind, value, X):
    """the closed form and the general path; a pixel whose zero-weight column lies to its left, and one with it to its right"""
    f, lab, ref_lab, P, must = LC.fused_nonfinite(pkind, value, X)
    B, Hh, Ww, _ = f.shape
    h, w = Hh // 4, Ww // 4
    nv = float((lab != 255).sum())
    clean = np.where(np.isfinite(f), f, F32(0))
    de, bar = LC.head_bwd_ref(clean, ref_lab, P, nv, float(B), 255, LC.REAL_ALPHA, LC.REAL_GOUT)
    inp = Frozen(feats=f, labels=lab, protos=P, sums=sums_for(nv, B))
    gout_t = torch.tensor(LC.REAL_GOUT, dtype=torch.float32, device="cuda")
    for dname in ("f32", "bf16"):
        out = Out(B * h * w * 16, dname)
        chk(call_fused(lib, inp, out, B, h, w, 255, LC.REAL_ALPHA, float(B), dname, gout_t))
        got = out.get(de.shape)
        assert (~np.isfinite(got[must])).all(), "an element the pixel interpolates into is finite"
        what = "fused %s feature %s %s" % (value, pkind, dname)
        measure(what, HC.check_close(what, got[~must], de[~must], LC.stored_bar(bar, de, dname)[~must], False))
        out.untouched()
    inp.same()


def test_fused_refuses_what_it_does_not_cover(lib):
    """H != 4 h, W != 4 w, C != 16, K != 16: DML_EUNSUPPORTED; a NULL pointer: DML_EINVAL; de keeps every 0xAA byte"""
    B, h, w = 1, 2, 3
    f, lab, P = np.zeros((B, 4 * h, 4 * w, 16), F32), np.zeros((B, 4 * h, 4 * w), np.int64), LC.protos("eye")
    inp = Frozen(feats=f, labels=lab, protos=P, sums=sums_for(96.0, 1.0))
    out = Out(B * h * w * 16)
    ok = dict(feats=inp["feats"], labels=inp["labels"], sums=inp["sums"], protos=inp["protos"], de=out.ptr, C=16, K=16, H=4 * h, W=4 * w)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dml_head_bwd_fused(a["feats"], a["labels"], a["sums"], None, a["protos"], a["de"], B, h, w, a["C"], a["K"], a["H"], a["W"],
                                      255, 0.01, 1.0, 0, st())
    for kw in (dict(H=4 * h + 1), dict(H=4 * h - 4), dict(W=4 * w + 4), dict(W=w), dict(C=15), dict(C=32), dict(K=15), dict(K=17)):
        assert call(**kw) == EUNSUPPORTED, kw
    for name in ("feats", "labels", "sums", "protos", "de"):
        assert call(**{name: None}) == EINVAL, name
    torch.cuda.synchronize()
    assert out.all_aa()
    chk(call())
    assert not out.all_aa()
    out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# dml_loss_fwd / dml_loss_finalize / dml_loss_bwd
# ---------------------------------------------------------------------------------------------------------------------
def run_loss(lib, case, regime, alpha=0.01, variants=((0.5, True), (None, False))):
    """forward sums, both finalize branches, then the backward with exact sums from the test for every (gout, n_images passed?)"""
    name, B, K, Hh, Ww, ign = case[:6]
    lg, lab = LC.loss_input(case, regime)
    ref = LC.loss_ref(lg, lab, ign, alpha, float(B), variants[0][0])
    inp = Frozen(logits=lg, labels=lab)
    sums, part, loss = Out(5, "f64"), Out(LC.MAX_BLOCKS * 4), Out(2)
    what = "loss %s %s" % (name, regime)
    chk(lib.dml_loss_fwd(inp["logits"], inp["labels"], sums.ptr, part.ptr, B, K, Hh, Ww, ign, st()))
    assert bool((sums.bits()[32:] == 0xAA).all()), "dml_loss_fwd wrote sums[4]"
    sums.body[4] = float(B)
    s = sums.get((5,))
    assert int(s[1]) == int(ref["sums"][1]) and s[1] == int(s[1]), what + ": sums[1] %r, expected %r" % (s[1], ref["sums"][1])
    assert int(s[3]) == int(ref["sums"][3]) and s[3] == int(s[3]), what + ": sums[3] %r, expected %r" % (s[3], ref["sums"][3])
    chk(lib.dml_loss_finalize(sums.ptr, loss.ptr, alpha, float(B), st()))
    chk(lib.dml_loss_finalize(sums.ptr, loss.ptr + 4, alpha, 0.0, st()))
    l2 = loss.get((2,))
    if regime == "nan":
        assert np.isnan(l2).all() and np.isnan(s[0])
    else:
        for q in (0, 2):
            measure("%s sums[%d]" % (what, q), HC.check_close("%s sums[%d]" % (what, q), s[q:q + 1], ref["sums"][q:q + 1], ref["sbar"][q:q + 1], False))
        measure(what + " loss", HC.check_close(what + " loss", l2, np.full(2, ref["loss"]), np.full(2, ref["lbar"]), False))
        assert l2[0] == l2[1], "n_images from sums[4] gives another loss"
    for o in (sums, part, loss):
        o.untouched()
    for gout, n_passed in variants:
        r = ref if gout == variants[0][0] else LC.loss_ref(lg, lab, ign, alpha, float(B), gout)
        sup = Frozen(sums=np.array(list(ref["sums"][:4]) + [float(B)], F64) if regime != "nan" else sums_for(ref["sums"][1], float(B)))
        gout_t = None if gout is None else torch.tensor(gout, dtype=torch.float32, device="cuda")
        gl = Out(B * K * Hh * Ww, guard=max(GUARD, Ww + 1))
        chk(lib.dml_loss_bwd(inp["logits"], inp["labels"], sup["sums"], None if gout_t is None else gout_t.data_ptr(), gl.ptr, B, K, Hh, Ww, ign,
                             alpha, float(B) if n_passed else 0.0, st()))
        got = gl.get(lg.shape)
        measure("%s glogits gout=%s" % (what, gout), LC.compare(what + " glogits", got, r["grad"], r["gbar"]))
        if regime.startswith("neg_inf"):
            plane = 0 if regime.endswith("0") else K - 1
            assert (got[:, plane][np.isneginf(lg[:, plane])] == 0).all()
        if K == 1 and alpha == 0:
            assert (got == 0).all()
        gl.untouched()
        sup.same()
        del gl
    inp.same()


SMALL = [(c, r) for c in LC.LOSS_CASES for r in c[7]]


@pytest.mark.parametrize("case,regime", SMALL, ids=["%s-%s" % (c[0], r) for c, r in SMALL])
def test_loss_small_cases(lib, case, regime):
    if case[0] == "hw1_513_grid_stride":                                         # 16.8 M logits: one backward, n from sums[4]
        return run_loss(lib, case, regime, variants=((0.5, False),))
    run_loss(lib, case, regime)
    if case[0] in ("k1_hw3", "k1_hw0", "hw0_6x10", "hw3_3x5"):
        run_loss(lib, case, regime, alpha=0.0, variants=((0.5, True),))


@pytest.mark.parametrize("case", LC.BIG_CASES, ids=[c[0] for c in LC.BIG_CASES])
def test_loss_above_the_grid_caps(lib, case):
    """the smallest shapes whose grid-stride loops make a second trip: the vector forward above 2048 workgroups, the vector and the
    scalar backward above their 8192"""
    run_loss(lib, case, "spread", variants=((0.5, True),))


def test_loss_bwd_with_the_sums_of_the_forward(lib):
    """the chain as the plan runs it: the backward reads what the forward left in sums"""
    case = [c for c in LC.LOSS_CASES if c[0] == "hw0_50x34_k13"][0]
    name, B, K, Hh, Ww, ign = case[:6]
    lg, lab = LC.loss_input(case, "close")
    ref = LC.loss_ref(lg, lab, ign, 0.01, float(B), 0.5)
    inp = Frozen(logits=lg, labels=lab)
    sums, part, gl = Out(5, "f64"), Out(LC.MAX_BLOCKS * 4), Out(lg.size)
    chk(lib.dml_loss_fwd(inp["logits"], inp["labels"], sums.ptr, part.ptr, B, K, Hh, Ww, ign, st()))
    gout_t = torch.tensor(0.5, dtype=torch.float32, device="cuda")
    chk(lib.dml_loss_bwd(inp["logits"], inp["labels"], sums.ptr, gout_t.data_ptr(), gl.ptr, B, K, Hh, Ww, ign, 0.01, float(B), st()))
    measure("loss chain glogits", LC.compare("loss chain glogits", gl.get(lg.shape), ref["grad"], ref["gbar"]))
    for o in (sums, part, gl):
        o.untouched()
    inp.same()


def test_loss_refuses_null_pointers(lib):
    x = Out(64)
    s = Out(5, "f64")
    lab = dev(np.zeros(16, np.int64))
    assert lib.dml_loss_fwd(None, lab.data_ptr(), s.ptr, x.ptr, 1, 4, 2, 2, 255, st()) == EINVAL
    assert lib.dml_loss_fwd(x.ptr, lab.data_ptr(), None, x.ptr, 1, 4, 2, 2, 255, st()) == EINVAL
    assert lib.dml_loss_finalize(None, x.ptr, 0.01, 1.0, st()) == EINVAL
    assert lib.dml_loss_bwd(x.ptr, lab.data_ptr(), s.ptr, None, None, 1, 4, 2, 2, 255, 0.01, 1.0, st()) == EINVAL
    assert lib.dml_loss_bwd(x.ptr, lab.data_ptr(), None, None, x.ptr, 1, 4, 2, 2, 255, 0.01, 1.0, st()) == EINVAL
    torch.cuda.synchronize()
    assert x.all_aa() and s.all_aa()


# ---------------------------------------------------------------------------------------------------------------------
# dml_focal_loss_*: the same running maximum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["neg_inf_plane0", "neg_inf_plane_last"])
@pytest.mark.parametrize("shape", [(5, 7), (6, 10)], ids=["hw3", "hw0"])
def test_focal_loss_with_one_neg_inf_logit(lib, regime, shape):
    """csrc/focal_loss.hip's online log-sum-exp had the same exp(-inf + inf): the float64 definition of tests/focal_cases.py is finite,
    with a gradient of exactly 0 in that plane, and so must the kernels be -- against focal_cases.focal_ref and its bars"""
    import focal_cases as FC
    from dmlnet import _lib as L
    lg, lab = LC.loss_input(("focal", 2, 16) + shape + (255, "5%"), regime)
    assert np.isneginf(lg).sum() == 2
    B, K, Hh, Ww = lg.shape
    ref = FC.focal_ref(lg, lab, 0.25, 2.0, True, 255, gout=0.5)
    assert np.isfinite(ref["loss"]) and (ref["grad"][np.isneginf(lg)] == 0).all()
    inp = Frozen(logits=lg, labels=lab)
    sums, part, loss, gl = Out(4, "f64"), Out(L.FOCAL_PARTIALS), Out(1), Out(lg.size)
    gout_t = torch.tensor(0.5, dtype=torch.float32, device="cuda")
    chk(lib.dml_focal_loss_fwd(inp["logits"], inp["labels"], sums.ptr, part.ptr, B, K, Hh, Ww, 255, 0.25, 2.0, st()))
    chk(lib.dml_focal_loss_finalize(sums.ptr, loss.ptr, 1, st()))
    chk(lib.dml_focal_loss_bwd(inp["logits"], inp["labels"], sums.ptr, gout_t.data_ptr(), gl.ptr, B, K, Hh, Ww, 255, 0.25, 2.0, 1, st()))
    what = "focal %s %s" % (regime, shape)
    s = sums.get((4,))
    assert (s[1:] == ref["sums"][1:]).all(), (what, s, ref["sums"])
    measure(what + " sum", HC.check_close(what + " sum", s[:1], ref["sums"][:1], np.array([ref["sum_bar"]]), False))
    measure(what + " loss", HC.check_close(what + " loss", loss.get((1,)), np.array([ref["loss"]]),
                                           np.array([ref["loss_bar"] + LC.EPS32 * abs(ref["loss"])]), False))
    got = gl.get(lg.shape)
    measure(what + " gradient", HC.check_close(what + " gradient", got, ref["grad"], ref["grad_bar"], False))
    assert (got[ref["grad_bar"] == 0] == 0).all(), what + ": an element with a zero bar is not 0"
    for o in (sums, part, loss, gl):
        o.untouched()
    inp.same()
