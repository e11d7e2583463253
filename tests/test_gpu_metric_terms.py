"""GPU: the Inter and Center terms of the metric loss -- dml_metric_fwd / _finalize / _bwd (csrc/metric_terms.hip) through the C
ABI, through utils.DMLLoss(beta=, gamma=), under the model's train step and under main_embedding.py.

Every float comparison is against the float64 definition of tests/metric_cases.py on the same float32 inputs (proved to be the
reference's statements, without a GPU, by tests/test_metric_refs.py), on EVERY element, to the bars derived there; an element
whose bar is 0 must be exactly 0 (a logit-gradient element added into a buffer: exactly the buffer's value), counts are compared
as integers.  Each float check prints "MEASURE <case> ... err/bar" before it asserts.

Largest err/bar measured on an MI355X: see DESIGN.md 7k.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import metric_cases as MC

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
F64 = np.float64
GUARD = 64                       # elements before and after an output: the output keeps its alignment
NAMES = list(MC.CASES)


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    assert _lib.metric_work_doubles(16, 16) == 2048 * (2 + 16 * 17)
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def shifted(host, shift, dtype):
    """a device copy of `host` that starts `shift` elements into a 256-byte aligned allocation -> (buffer, pointer)"""
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.zeros(host.size + shift, dtype=dtype, device="cuda")
    buf[shift:] = torch.from_numpy(np.array(host).ravel()).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + item * shift


def guarded(n, shift, dtype, fill):
    """an output of n elements, prefilled, between two guards of 7 -> (buffer, first element, pointer)"""
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD + shift,), 7, dtype=dtype, device="cuda")
    lo = GUARD + shift
    buf[lo:lo + n] = fill
    return buf, lo, buf.data_ptr() + item * lo


def unguard(buf, lo, n, what):
    a = buf.cpu().numpy()
    assert (a[:lo] == 7).all() and (a[lo + n:] == 7).all(), "a guard element of %s was written" % what
    return a[lo:lo + n].copy()


class Run:
    """the three entry points on host arrays.  Every output is pre-filled (NaN; counts -7) between two guards that must come back
    untouched, work is guarded past its documented size and the inputs must come back unwritten.  `shift` moves the logits /
    features / labels / logit-gradient / feature-gradient pointers by that many elements.  g0: the buffer the logit gradient is
    added into (zeros when None).  Logits are passed when beta != 0, features when gamma != 0, as utils.DMLLoss does."""

    def __init__(self, lib, lg, f, y, ignore, beta, gamma, shift=(0, 0, 0, 0, 0)):
        from dmlnet import _lib
        self.lib, self.ignore, self.beta, self.gamma, self.shift = lib, ignore, beta, gamma, shift
        self.lg, self.f, self.y = lg, f, y
        self.B, self.K, self.Hh, self.Ww = lg.shape
        self.C = f.shape[3]
        self.lbuf, self.lptr = shifted(lg, shift[0], torch.float32)
        self.fbuf, self.fptr = shifted(f, shift[1], torch.float32)
        self.ybuf, self.yptr = shifted(y, shift[2], torch.int64)
        self.use_l, self.use_f = beta != 0, gamma != 0
        self.ns = 2 * self.B + 3
        self.sums = guarded(self.ns, 0, torch.float64, float("nan"))
        self.nw = _lib.metric_work_doubles(self.K, self.C)
        self.work = torch.full((self.nw + GUARD,), 7.0, dtype=torch.float64, device="cuda")
        self.means = guarded(self.B * self.K * self.C, 0, torch.float32, float("nan"))
        self.counts = guarded(self.B * self.K, 0, torch.int32, -7)

    def fwd(self):
        rc = self.lib.dml_metric_fwd(self.lptr if self.use_l else None, self.fptr if self.use_f else None, self.yptr,
                                     self.means[2] if self.use_f else None, self.counts[2] if self.use_f else None, self.sums[2],
                                     self.work.data_ptr(), self.B, self.K, self.C, self.Hh, self.Ww, self.ignore, st())
        assert rc == 0, "dml_metric_fwd returned %d" % rc
        return self

    def finish(self, gout=None, n_images=None, g0=None):
        """finalize + backward -> dict(sums, term, means, counts, gl, gf)"""
        B, K, C = self.B, self.K, self.C
        nim = float(B) if n_images is None else float(n_images)
        term = guarded(1, 0, torch.float32, float("nan"))
        rc = self.lib.dml_metric_finalize(self.sums[2], B, self.beta, self.gamma, nim, term[2], st())
        assert rc == 0, "dml_metric_finalize returned %d" % rc
        gl = guarded(self.lg.size, self.shift[3], torch.float32, 0.0)
        if g0 is not None:
            gl[0][gl[1]:gl[1] + self.lg.size] = torch.from_numpy(np.ascontiguousarray(g0).ravel()).cuda()
        gf = guarded(self.f.size, self.shift[4], torch.float32, float("nan"))
        go = None if gout is None else torch.tensor([gout], dtype=torch.float32, device="cuda")
        rc = self.lib.dml_metric_bwd(self.fptr if self.use_f else None, self.yptr, self.means[2] if self.use_f else None, self.sums[2],
                                     None if go is None else go.data_ptr(), gl[2] if self.use_l else None,
                                     gf[2] if self.use_f else None, B, K, C, self.Hh, self.Ww, self.ignore, self.beta, self.gamma,
                                     nim, st())
        assert rc == 0, "dml_metric_bwd returned %d" % rc
        torch.cuda.synchronize()
        assert (self.work[self.nw:].cpu().numpy() == 7.0).all(), "work was written past its documented size"
        assert (self.lbuf[self.shift[0]:].cpu().numpy() == np.array(self.lg).ravel()).all(), "the logits were written"
        assert (self.fbuf[self.shift[1]:].cpu().numpy() == np.array(self.f).ravel()).all(), "the features were written"
        assert (self.ybuf[self.shift[2]:].cpu().numpy() == np.array(self.y).ravel()).all(), "the labels were written"
        out = dict(sums=unguard(*self.sums[:2], self.ns, "sums"), term=unguard(*term[:2], 1, "term")[0],
                   gl=unguard(*gl[:2], self.lg.size, "the logit gradient").reshape(self.lg.shape),
                   gf=unguard(*gf[:2], self.f.size, "the feature gradient").reshape(self.f.shape),
                   means=unguard(*self.means[:2], B * K * C, "means").reshape(B, K, C),
                   counts=unguard(*self.counts[:2], B * K, "counts").reshape(B, K))
        if not self.use_f:                                 # not given: not written
            assert np.isnan(out["gf"]).all() and np.isnan(out["means"]).all() and (out["counts"] == -7).all()
            out["gf"] = np.zeros_like(out["gf"])
            out["means"], out["counts"] = np.zeros_like(out["means"]), np.zeros_like(out["counts"])
        return out


def run_case(lib, name, gout="case", n_images=None, g0=None, shift=(0, 0, 0, 0, 0)):
    c = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    return Run(lib, lg, f, y, c["ignore"], c["beta"], c["gamma"], shift).fwd().finish(c["gout"] if gout == "case" else gout,
                                                                                      n_images, g0)


def ratio(err, bar):
    pos = bar > 0
    return float((err[pos] / bar[pos]).max(initial=0.0))


def check(what, got, ref, g0=None, rows=None):
    """counts exactly; means, Inter_i, Center_i, their sums, the term and every gradient element against the definition.
    rows: the images of `ref` that `got` holds (a part of the batch: the term and the sums' tail are not compared)"""
    sel = slice(None) if rows is None else rows
    B = ref["counts"][sel].shape[0]
    sums = got["sums"]
    assert np.array_equal(got["counts"], ref["counts"][sel]), (what, got["counts"], ref["counts"][sel])
    e_mu = np.abs(got["means"].astype(F64) - ref["means"][sel])
    e_in, e_ce = np.abs(sums[0:2 * B:2] - ref["inter"][sel]), np.abs(sums[1:2 * B:2] - ref["center"][sel])
    base = np.zeros_like(ref["gl"][sel]) if g0 is None else g0.astype(F64)
    e_gl = np.abs(got["gl"].astype(F64) - (base + ref["gl"][sel]))
    gl_bar = ref["gl_bar"][sel] + (0 if g0 is None else np.where(ref["gl_bar"][sel] > 0, MC.EPS32 * np.abs(base + ref["gl"][sel]), 0))
    e_gf = np.abs(got["gf"].astype(F64) - ref["gf"][sel])
    print("MEASURE %s worst err/bar: means %.3e | Inter_i %.3e | Center_i %.3e | logit gradient %.3e | feature gradient %.3e"
          % (what, ratio(e_mu, ref["means_bar"][sel]), ratio(e_in, ref["inter_bar"][sel]), ratio(e_ce, ref["center_bar"][sel]),
             ratio(e_gl, gl_bar), ratio(e_gf, ref["gf_bar"][sel])))
    for k in ("sums", "gl", "gf", "means"):
        assert np.isfinite(got[k]).all(), (what, k)
    assert (e_mu <= ref["means_bar"][sel]).all(), (what, "means", e_mu.max())
    assert (e_in <= ref["inter_bar"][sel]).all(), (what, sums[0:2 * B:2], ref["inter"][sel])
    assert (e_ce <= ref["center_bar"][sel]).all(), (what, sums[1:2 * B:2], ref["center"][sel])
    zero = gl_bar == 0
    assert np.array_equal(bits(got["gl"][zero]), bits(base.astype(np.float32)[zero])), what + ": a logit-gradient element with a zero bar changed"
    bad = np.flatnonzero(e_gl > gl_bar)
    assert bad.size == 0, "%s: %d logit-gradient elements above the bar, first %s" % (what, bad.size, bad[:6])
    assert (got["gf"][ref["gf_bar"][sel] == 0] == 0).all(), what + ": a feature-gradient element with a zero bar is not 0"
    bad = np.flatnonzero(e_gf > ref["gf_bar"][sel])
    assert bad.size == 0, "%s: %d feature-gradient elements above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], got["gf"].ravel()[bad[:6]], ref["gf"][sel].ravel()[bad[:6]])
    if rows is None:
        e_term = abs(F64(got["term"]) - ref["term"])
        print("MEASURE %s term err=%.3e bar=%.3e err/bar=%.3e" % (what, e_term, ref["term_bar"], e_term / ref["term_bar"]))
        assert np.isfinite(got["term"]) and e_term <= ref["term_bar"], (what, got["term"], ref["term"])
        assert abs(sums[2 * B] - ref["sums"][2 * B]) <= ref["inter_bar"].sum() and sums[2 * B + 2] == B
        assert abs(sums[2 * B + 1] - ref["sums"][2 * B + 1]) <= ref["center_bar"].sum()


def same_bits(a, b, what):
    for k in ("sums", "term", "means", "counts", "gl", "gf"):
        assert np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k]))), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("name", NAMES)
def test_c_abi_against_float64(lib, name):
    """the case's weights and gout; n read from sums[2 B + 2] instead of the argument: the same bits; the logit gradient added
    into a non-zero buffer"""
    c = MC.CASES[name]
    ref = MC.reference(name)
    got = run_case(lib, name)
    check(name, got, ref)
    same_bits(run_case(lib, name, n_images=0), got, name + " n from sums")
    g0 = H.rng_for(3, "metric.g0." + name).standard_normal(ref["gl"].shape).astype(np.float32) * np.float32(1e-4)
    check(name + " into a non-zero buffer", run_case(lib, name, g0=g0), ref, g0=g0)
    if c["gout"] == 1.0:
        same_bits(run_case(lib, name, gout=None), got, name + " gout NULL")


def test_weights_alone_and_gout_null(lib):
    """beta alone and gamma alone on a case that has both, gout NULL = 1: each term by itself, the other input not read"""
    name = "17x23 edges"
    c = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    for beta, gamma in ((c["beta"], 0.0), (0.0, c["gamma"])):
        ref = MC.metric_ref(lg, f, y, c["ignore"], beta, gamma, with_feats=gamma != 0, with_logits=beta != 0)
        got = Run(lib, lg, f, y, c["ignore"], beta, gamma).fwd().finish()
        check("%s beta=%g gamma=%g" % (name, beta, gamma), got, ref)
        same_bits(Run(lib, lg, f, y, c["ignore"], beta, gamma).fwd().finish(gout=1.0), got, "gout=1 is the NULL one")


@pytest.mark.parametrize("C", (1, 2))
def test_the_largest_lds_tables(lib, C):
    """K = 32 with C = 1 and C = 2: the class-sum launch's dynamic LDS is 4 K (64 + 64 / CP) floats = 64 KiB (the most a launch
    may ask for) and 48 KiB; the tabled cases stop at 33 KiB"""
    name = "17x23 K=32 C=%d" % C
    assert 4 * 32 * (64 + 64 // C) * 4 == (65536 if C == 1 else 49152)
    lg, f, y = MC.make_inputs(name, B=3, H=17, W=23, K=32, C=C, ignore=255, labels="mix", feats="trained")
    assert (np.bincount(y[y != 255], minlength=32) > 0).all()                      # every row of the table is used
    ref = MC.metric_ref(lg, f, y, 255, 1e-4, 1e-2, gout=-2.5)
    got = Run(lib, lg, f, y, 255, 1e-4, 1e-2).fwd().finish(gout=-2.5)
    check(name, got, ref)
    same_bits(Run(lib, lg, f, y, 255, 1e-4, 1e-2).fwd().finish(gout=-2.5), got, name + ": two runs")


def test_two_runs_are_bitwise_equal(lib):
    for name in ("96x160", "17x23 edges"):
        same_bits(run_case(lib, name), run_case(lib, name), name + ": two runs")


@pytest.mark.parametrize("name", ("96x160", "17x23 offset", "96x160 edges"))
def test_shifted_pointers_take_the_narrow_path_bitwise(lib, name):
    """these cases take the 16-byte paths (H W C % 4 == 0 and H W % 4 == 0 where the logits are read); each tensor in turn one
    element off (4 bytes, the labels 8), then all: the same bits"""
    c = MC.CASES[name]
    aligned = run_case(lib, name)
    check(name + " aligned", aligned, MC.reference(name))
    for shift in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (3, 2, 1, 3, 2)):
        same_bits(run_case(lib, name, shift=shift), aligned, "%s shift %s" % (name, shift))


def test_two_half_batches_with_their_tails_added_on_the_device(lib):
    """images {0} and {1, 2} of a batch of three as two calls (two ranks): each forward leaves its sums, the last three doubles
    are added on the device as an all-reduce would, and finalize and backward read n from there (n_images = 0): the term and
    every per-image value and gradient element equal the whole batch's within the bars"""
    name = "96x160"
    c = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    ref = MC.reference(name)
    parts = [Run(lib, lg[r], f[r], y[r], c["ignore"], c["beta"], c["gamma"]).fwd() for r in (slice(0, 1), slice(1, 3))]
    tails = [p.sums[0][p.sums[1] + 2 * p.B:p.sums[1] + 2 * p.B + 3] for p in parts]
    total = tails[0] + tails[1]
    for t in tails:
        t.copy_(total)
    for p, r in zip(parts, (slice(0, 1), slice(1, 3))):
        got = p.finish(gout=c["gout"], n_images=0)
        assert got["sums"][2 * p.B + 2] == 3
        check("%s images %s of 3" % (name, r), got, ref, rows=r)
        e = abs(F64(got["term"]) - ref["term"])
        print("MEASURE half batches term err=%.3e bar=%.3e" % (e, ref["term_bar"]))
        assert e <= ref["term_bar"]


def test_error_codes(lib):
    """argument checks return before any launch: every output is still prefilled"""
    from dmlnet import _lib
    f = torch.full((8192,), -7.0, dtype=torch.float32, device="cuda")
    y = torch.zeros(256, dtype=torch.int64, device="cuda")
    sums = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.full((_lib.metric_work_doubles(32, 32),), 7.0, dtype=torch.float64, device="cuda")
    means = torch.full((2 * 32 * 32,), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    g = torch.full((8192,), float("nan"), dtype=torch.float32, device="cuda")
    gf = torch.full((8192,), float("nan"), dtype=torch.float32, device="cuda")
    term = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
    F, Y = f.data_ptr(), y.data_ptr()
    inf, nan = float("inf"), float("nan")

    def fwd(lg=F, ft=F, lab=Y, mu=means.data_ptr(), cn=counts.data_ptr(), sm=sums.data_ptr(), wk=work.data_ptr(), B=2, K=16, C=16,
            Hh=4, Ww=4):
        return lib.dml_metric_fwd(lg, ft, lab, mu, cn, sm, wk, B, K, C, Hh, Ww, 255, st())

    def bwd(ft=F, lab=Y, mu=means.data_ptr(), sm=sums.data_ptr(), gl=g.data_ptr(), gfe=gf.data_ptr(), B=2, K=16, C=16, Hh=4, Ww=4,
            beta=1e-4, gamma=1e-2):
        return lib.dml_metric_bwd(ft, lab, mu, sm, None, gl, gfe, B, K, C, Hh, Ww, 255, beta, gamma, 2.0, st())

    assert fwd(lab=None) == EINVAL and fwd(sm=None) == EINVAL and fwd(wk=None) == EINVAL and fwd(lg=None, ft=None) == EINVAL
    assert fwd(mu=None) == EINVAL and fwd(cn=None) == EINVAL                       # required with features
    assert bwd(lab=None) == EINVAL and bwd(sm=None) == EINVAL and bwd(gl=None, gfe=None) == EINVAL
    assert bwd(ft=None) == EINVAL and bwd(mu=None) == EINVAL                       # required with a feature gradient
    assert bwd(beta=inf) == EINVAL and bwd(gamma=nan) == EINVAL
    for fn in (fwd, bwd):
        assert fn(B=0) == EINVAL and fn(B=-1) == EINVAL and fn(Hh=0) == EINVAL and fn(Ww=-1) == EINVAL
        assert fn(K=0) == EINVAL and fn(C=0) == EINVAL and fn(K=-3) == EINVAL
        assert fn(K=33) == EUNSUPPORTED and fn(C=33) == EUNSUPPORTED and fn(B=2049) == EUNSUPPORTED
        assert fn(Hh=1 << 15, Ww=1 << 12) == EUNSUPPORTED                          # H W C >= 2^31
    fin = lib.dml_metric_finalize
    assert fin(None, 2, 1e-4, 1e-2, 2.0, term.data_ptr(), st()) == EINVAL
    assert fin(sums.data_ptr(), 2, 1e-4, 1e-2, 2.0, None, st()) == EINVAL
    assert fin(sums.data_ptr(), 0, 1e-4, 1e-2, 2.0, term.data_ptr(), st()) == EINVAL
    assert fin(sums.data_ptr(), 2, nan, 1e-2, 2.0, term.data_ptr(), st()) == EINVAL
    assert fin(sums.data_ptr(), 2, 1e-4, inf, 2.0, term.data_ptr(), st()) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(g.cpu().numpy()).all() and np.isnan(gf.cpu().numpy()).all() and (sums.cpu().numpy() == 7.0).all()
    assert (work.cpu().numpy() == 7.0).all() and (means.cpu().numpy() == 7.0).all() and (counts.cpu().numpy() == -7).all()
    assert term.item() == 7.0 and (y.cpu().numpy() == 0).all() and (f.cpu().numpy() == -7.0).all()
    # the optional pointers: one input or one output alone is a call
    assert fwd(lg=None) == 0 and fwd(ft=None, mu=None, cn=None) == 0
    assert bwd(gl=None) == 0 and bwd(gfe=None, ft=None, mu=None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# utils.DMLLoss
# ---------------------------------------------------------------------------------------------------------------------------
def dml(lg, y, f, **kw):
    """-> (loss, d loss / d logits, d loss / d features or None) of 3 x utils.DMLLoss(**kw)(logits, labels, features)"""
    import utils
    x = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
    ft = None if f is None else torch.from_numpy(np.array(f)).cuda().requires_grad_(True)
    loss = utils.DMLLoss(**kw)(x, torch.from_numpy(np.array(y)).cuda(), ft)
    assert loss.shape == () and loss.dtype == torch.float32
    (3 * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), x.grad.clone(), None if ft is None or ft.grad is None else ft.grad.clone()


def test_zero_weights_are_the_loss_as_it_was_bitwise():
    import utils
    lg, f, y = MC.inputs("96x160")
    old = dml(lg, y, f, alpha=0.01, ignore_index=255)
    new = dml(lg, y, f, alpha=0.01, ignore_index=255, beta=0, gamma=0.0)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]) and old[2] is None and new[2] is None
    assert torch.isfinite(old[0]) and old[1].abs().sum() > 0
    d = utils.DMLLoss(0.02, 255, None, True)                                      # the positional order is unchanged
    assert (d.alpha, d.ignore_index, d.sync, d.fused_backward, d.beta, d.gamma) == (0.02, 255, None, True, 0.0, 0.0)
    x = torch.zeros(1, 16, 4, 4, device="cuda")
    yy = torch.zeros(1, 4, 4, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError):
        utils.DMLLoss(gamma=0.01)(x, yy)                                          # the centre term needs the features
    with pytest.raises(ValueError):
        utils.DMLLoss(gamma=0.01)(x, yy, None)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            utils.DMLLoss(beta=bad)
        with pytest.raises(ValueError):
            utils.DMLLoss(gamma=bad)
    with pytest.raises(RuntimeError):
        utils.DMLLoss(beta=1e-4)(torch.zeros(1, 16, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))      # CPU: no fallback
    assert torch.isfinite(utils.DMLLoss(beta=1e-4)(x, yy))                         # beta alone needs no features


@pytest.mark.parametrize("name", ("96x160", "17x23 edges", "96x160 wide", "96x160 offset"))
def test_dml_loss_against_float64(lib, name):
    """loss - (CE + alpha VAR) / n is the term, d loss / d logits - the old gradient is the Inter gradient, d loss / d features
    the Center gradient, to the definition's bars with gout = 3; and the same bits as the C ABI"""
    c = MC.CASES[name]
    lg, f, y = MC.inputs(name)
    ref = MC.metric_ref(lg, f, y, c["ignore"], c["beta"], c["gamma"], gout=3.0, with_feats=c["gamma"] != 0, with_logits=c["beta"] != 0)
    old = dml(lg, y, None, alpha=0.01, ignore_index=c["ignore"])
    new = dml(lg, y, f, alpha=0.01, ignore_index=c["ignore"], beta=c["beta"], gamma=c["gamma"], fused_backward=True)
    e = abs((F64(new[0].item()) - F64(old[0].item())) - ref["term"])                       # the value does not depend on gout
    bar = ref["term_bar"] + 2 * MC.EPS32 * (abs(new[0].item()) + abs(old[0].item()))     # each loss is a float32
    print("MEASURE python %s loss - old loss err=%.3e bar=%.3e err/bar=%.3e" % (name, e, bar, e / bar))
    assert e <= bar
    direct = Run(lib, lg, f, y, c["ignore"], c["beta"], c["gamma"]).fwd().finish(gout=3.0, g0=old[1].cpu().numpy())
    assert np.array_equal(bits(direct["gl"]), bits(new[1].cpu().numpy())), "the logit gradient is not dml_loss_bwd's plus the C ABI's"
    if c["gamma"] != 0:
        gf = new[2].cpu().numpy()
        assert np.array_equal(bits(direct["gf"]), bits(gf))
        err = np.abs(gf.astype(F64) - ref["gf"])
        assert (err <= ref["gf_bar"]).all() and (gf[ref["gf_bar"] == 0] == 0).all()
    else:
        assert new[2] is None
    if c["beta"] == 0:
        assert torch.equal(new[1], old[1])


SYNC_SCRIPT = r"""
import sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import metric_cases as MC
import utils
dist.init_process_group(backend="nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
lg, f, y = MC.inputs("96x160")
out = []
for sync in (None, True, dist.group.WORLD):
    x = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
    ft = torch.from_numpy(np.array(f)).cuda().requires_grad_(True)
    loss = utils.DMLLoss(alpha=0.01, ignore_index=255, sync=sync, beta=1e-4, gamma=1e-2)(x, torch.from_numpy(np.array(y)).cuda(), ft)
    (3 * loss).backward()
    out.append((loss.detach().clone(), x.grad.clone(), ft.grad.clone()))
torch.cuda.synchronize()
for j in (1, 2):
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[j])), j
assert torch.isfinite(out[0][0]) and out[0][1].abs().sum() > 0 and out[0][2].abs().sum() > 0
dist.destroy_process_group()
print("SYNC-OK")
"""


def test_sync_on_a_one_rank_group_is_bitwise_the_unsynchronised_loss():
    """sync=True (and an explicit group) on a forced single-rank RCCL group: the all-reduces are the identity and n is read from
    the device, so loss and both gradients equal sync=None bitwise.  A process of its own: a process group is process-wide state.
    More than one rank cannot be tested on one GPU."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, "-c", SYNC_SCRIPT, os.path.join(H.ROOT, "tests")], capture_output=True, text=True,
                       cwd=H.PKG, timeout=600, env=env)
    assert r.returncode == 0 and "SYNC-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------
# the model and the driver
# ---------------------------------------------------------------------------------------------------------------------------
def test_model_train_step_with_the_metric_terms():
    """2 x 3 x 64 x 64 (the focal test's fixture): DMLLoss(fused_backward=True) with zero weights still takes the fused head
    backward and equals DMLLoss(alpha) bit for bit; with gamma = 0.01 it trains through the materialised gradient -- finite
    parameter gradients, and the embedding conv's gradient moves"""
    import network
    import utils
    img = H.synth_tensor(5, "g5.img", (2, 3, 64, 64)).cuda()
    lab = H.synth_labels(5, "g5.lab", (2, 64, 64), 16, 255, ignore_rows=3).cuda()
    grads, losses, fused = {}, {}, {}
    for name, kw in (("old", {}), ("zero", dict(beta=0.0, gamma=0.0)), ("gamma", dict(beta=1e-4, gamma=0.01))):
        m = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
        m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=1))
        m.cuda().train()
        lg, _, ft = m(img)
        loss = utils.DMLLoss(alpha=0.01, ignore_index=255, fused_backward=True, **kw)(lg, lab, ft)
        loss.backward()
        torch.cuda.synchronize()
        losses[name] = loss.detach().clone()
        grads[name] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        plan = next(p for k, p in m._engine.plans.items() if k[4])
        fused[name] = plan.heads[0].unfused_range in plan.skip_ranges
        del m
    assert fused == {"old": True, "zero": True, "gamma": False}
    assert torch.equal(losses["old"], losses["zero"])
    for k, g in grads["old"].items():
        assert torch.equal(g, grads["zero"][k]), k
        assert torch.isfinite(grads["gamma"][k]).all(), k
    assert torch.isfinite(losses["gamma"]) and losses["gamma"] != losses["old"]
    k = "classifier.classifier.3.weight"                                           # the conv that writes the embedding
    scale = grads["old"][k].abs().max().item()
    moved = (grads["gamma"][k] - grads["old"][k]).abs().max().item() / scale
    print("MEASURE model step: loss %.7f -> %.7f, the embedding conv's gradient moves by %.3e of its largest element"
          % (losses["old"].item(), losses["gamma"].item(), moved))
    assert moved > 1e-4                                                            # far more than float32 rounding (6e-8)


def test_driver_trains_with_the_metric_terms():
    """main_embedding.py --loss_type dml --beta 1e-4 --gamma 1e-2 end to end: two finite losses"""
    drv = os.path.join(H.PKG, "main_embedding.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--loss_type", "dml", "--beta", "1e-4", "--gamma", "1e-2", "--batch_size", "2",
                        "--crop_size", "128", "--frame_height", "128", "--frame_width", "256", "--total_itrs", "2", "--dtype", "f32",
                        "--print_interval", "1"], capture_output=True, text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(ln.split("Loss=")[1].split(",")[0]) for ln in r.stdout.splitlines() if "Loss=" in ln]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), r.stdout[-2000:]
