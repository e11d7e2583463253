"""GPU: the focal loss -- dml_focal_loss_fwd / _finalize / _bwd (csrc/focal_loss.hip) through the C ABI, through
utils.FocalLoss and utils.CrossEntropyLoss(size_average=False), under the model's train step and under
main_embedding.py --loss_type focal_loss.

Every float comparison is against the float64 definition of tests/focal_cases.py on the same float32 inputs (proved to be the
reference's statements, without a GPU, by tests/test_focal_refs.py), on EVERY element, to the bars derived there; an element
whose bar is 0 must be exactly 0.  Each float check prints
"MEASURE <case> err=<largest error> bar=<largest bar> worst err/bar=<largest ratio>" before it asserts.

Largest err/bar measured on an MI355X: see DESIGN.md 7g.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import focal_cases as FC
import helpers as H

pytestmark = pytest.mark.gpu

EINVAL = -1
F64 = np.float64
GUARD = 64                       # floats before and after an output: 256 bytes, so the output keeps its alignment
PARTIALS = 3 * 2048              # the documented size of block_partials, in floats


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def shifted(host, shift, dtype):
    """a device copy of `host` that starts `shift` elements into a 256-byte aligned allocation -> (buffer, pointer)"""
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.zeros(host.size + shift, dtype=dtype, device="cuda")
    buf[shift:] = torch.from_numpy(np.array(host).ravel()).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + item * shift


def run(lib, lg, lab, alpha, gamma, size_average, ignore_index, gout=None, shift=(0, 0, 0)):
    """the three entry points on host arrays -> (sums (4,) float64, loss float32, gradient [B,K,H,W] float32).  Every output
    is pre-filled with NaN between two guards that must come back untouched; block_partials is guarded past its documented
    size.  `shift` moves the logits / labels / gradient pointers by that many elements (floats, int64s, floats)."""
    B, K, Hh, Ww = lg.shape
    lbuf, lptr = shifted(lg, shift[0], torch.float32)
    ybuf, yptr = shifted(lab, shift[1], torch.int64)
    n = lg.size
    gbuf = torch.full((n + 2 * GUARD + shift[2],), 7.0, dtype=torch.float32, device="cuda")
    gbuf[GUARD + shift[2]:GUARD + shift[2] + n] = float("nan")
    sums = torch.full((4 + 2,), 7.0, dtype=torch.float64, device="cuda")
    sums[1:5] = float("nan")
    part = torch.full((PARTIALS + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    loss = torch.full((3,), 7.0, dtype=torch.float32, device="cuda")
    loss[1] = float("nan")
    go = None if gout is None else torch.tensor([gout], dtype=torch.float32, device="cuda")
    rc = lib.dml_focal_loss_fwd(lptr, yptr, sums.data_ptr() + 8, part.data_ptr(), B, K, Hh, Ww, ignore_index, alpha, gamma, st())
    assert rc == 0, "dml_focal_loss_fwd returned %d" % rc
    rc = lib.dml_focal_loss_finalize(sums.data_ptr() + 8, loss.data_ptr() + 4, int(size_average), st())
    assert rc == 0, "dml_focal_loss_finalize returned %d" % rc
    rc = lib.dml_focal_loss_bwd(lptr, yptr, sums.data_ptr() + 8, None if go is None else go.data_ptr(),
                                gbuf.data_ptr() + 4 * (GUARD + shift[2]), B, K, Hh, Ww, ignore_index, alpha, gamma,
                                int(size_average), st())
    assert rc == 0, "dml_focal_loss_bwd returned %d" % rc
    torch.cuda.synchronize()
    g = gbuf.cpu().numpy()
    lo = GUARD + shift[2]
    assert (g[:lo] == 7.0).all() and (g[lo + n:] == 7.0).all(), "a guard element of the gradient was written"
    s = sums.cpu().numpy()
    assert s[0] == 7.0 and s[5] == 7.0, "a guard element of sums was written"
    ls = loss.cpu().numpy()
    assert ls[0] == 7.0 and ls[2] == 7.0, "a guard element of the loss was written"
    assert (part[PARTIALS:].cpu().numpy() == 7.0).all(), "block_partials was written past 3 x 2048 floats"
    assert (lbuf[shift[0]:].cpu().numpy() == np.array(lg).ravel()).all(), "the logits were written"
    return s[1:5].copy(), ls[1], g[lo:lo + n].reshape(lg.shape).copy()


def check(what, got, ref):
    """sums, loss and every gradient element against the definition"""
    sums, loss, grad = got
    assert sums[1] == ref["sums"][1] and sums[2] == ref["sums"][2] and sums[3] == ref["sums"][3], (what, sums, ref["sums"])
    e_sum, e_loss = abs(sums[0] - ref["sums"][0]), abs(F64(loss) - ref["loss"])
    loss_bar = ref["loss_bar"] + 2.0 ** -24 * abs(ref["loss"])          # the loss is stored as a float32: one more rounding
    err = np.abs(grad.astype(F64) - ref["grad"])
    bar = ref["grad_bar"]
    pos = bar > 0
    ratio = (err[pos] / bar[pos]).max(initial=0.0)
    print("MEASURE %s loss err=%.3e bar=%.3e err/bar=%.3e | sum err/bar=%.3e | gradient err=%.3e bar=%.3e worst err/bar=%.3e"
          % (what, e_loss, loss_bar, e_loss / loss_bar if loss_bar > 0 else 0.0,
             e_sum / ref["sum_bar"] if ref["sum_bar"] > 0 else 0.0, err.max(), bar.max(), ratio))
    assert np.isfinite(grad).all() and np.isfinite(loss), what
    assert e_sum <= ref["sum_bar"], (what, sums[0], ref["sums"][0])
    assert e_loss <= loss_bar, (what, loss, ref["loss"])
    assert (grad[~pos] == 0).all(), "%s: %d elements with a zero bar are not 0" % (what, (grad[~pos] != 0).sum())
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, "%s: %d gradient elements above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], grad.ravel()[bad[:6]], ref["grad"].ravel()[bad[:6]])
    return ratio


def name_of(K, shape, s):
    return "K=%d %s gamma=%g alpha=%g %s ignore=%d gout=%s" % (K, shape, s["gamma"], s["alpha"],
                                                               "mean" if s["size_average"] else "sum", s["ignore_index"], s["gout"])


CELLS = [(K, shape) for K in FC.CLASSES for shape in sorted(FC.SHAPES)]


@pytest.mark.parametrize("K,shape", CELLS)
def test_c_abi_against_float64(lib, K, shape):
    """every gamma x alpha x reduction of the cell, ignore_index and gout cycling (focal_cases.settings)"""
    worst = 0.0
    for s in FC.settings(K, shape):
        lg, lab = FC.inputs(K, shape, s["ignore_index"])
        go = 1.0 if s["gout"] is None else s["gout"]
        ref = FC.focal_ref(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], gout=go)
        got = run(lib, lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], gout=s["gout"])
        worst = max(worst, check(name_of(K, shape, s), got, ref))
    print("MEASURE cell K=%d %s worst gradient err/bar=%.3e" % (K, shape, worst))


@pytest.mark.parametrize("K", FC.CLASSES)
def test_shifted_pointers_take_the_scalar_path_bitwise(lib, K):
    """the vector shape with the logits, the labels or the gradient pointer off a 16-byte boundary (4 bytes; the labels 8):
    one float per lane, and the same bits as the aligned call"""
    for s in FC.settings(K, "vec")[3::7]:
        lg, lab = FC.inputs(K, "vec", s["ignore_index"])
        go = 1.0 if s["gout"] is None else s["gout"]
        ref = FC.focal_ref(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], gout=go)
        args = (lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], s["gout"])
        aligned = run(lib, *args)
        check(name_of(K, "vec", s), aligned, ref)
        for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            moved = run(lib, *args, shift=shift)
            check(name_of(K, "vec", s) + " shift=%s" % (shift,), moved, ref)
            assert np.array_equal(bits(moved[2]), bits(aligned[2])), "shift %s: the gradient differs from the aligned call" % (shift,)
            assert moved[0][1] == aligned[0][1] and moved[0][3] == aligned[0][3]


def test_error_codes(lib):
    """argument checks return before any launch"""
    a = torch.full((4096,), -7.0, dtype=torch.float32, device="cuda")
    y = torch.zeros(256, dtype=torch.int64, device="cuda")
    sums = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    part = torch.full((PARTIALS,), 7.0, dtype=torch.float32, device="cuda")
    g = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
    inf, nan = float("inf"), float("nan")

    def fwd(lg=a.data_ptr(), lab=y.data_ptr(), s=sums.data_ptr(), p=part.data_ptr(), B=1, K=13, Hh=4, Ww=4, alpha=1.0, gamma=2.0):
        return lib.dml_focal_loss_fwd(lg, lab, s, p, B, K, Hh, Ww, 255, alpha, gamma, st())

    def bwd(lg=a.data_ptr(), lab=y.data_ptr(), s=sums.data_ptr(), out=g.data_ptr(), B=1, K=13, Hh=4, Ww=4, alpha=1.0, gamma=2.0):
        return lib.dml_focal_loss_bwd(lg, lab, s, None, out, B, K, Hh, Ww, 255, alpha, gamma, 1, st())

    assert fwd(lg=None) == EINVAL and fwd(lab=None) == EINVAL and fwd(s=None) == EINVAL and fwd(p=None) == EINVAL
    assert bwd(lg=None) == EINVAL and bwd(lab=None) == EINVAL and bwd(s=None) == EINVAL and bwd(out=None) == EINVAL
    for f in (fwd, bwd):
        assert f(K=0) == EINVAL and f(K=-1) == EINVAL and f(B=0) == EINVAL and f(Hh=0) == EINVAL and f(Ww=-1) == EINVAL
        assert f(gamma=-1.0) == EINVAL and f(gamma=-1e-30) == EINVAL and f(gamma=inf) == EINVAL and f(gamma=nan) == EINVAL
        assert f(alpha=inf) == EINVAL and f(alpha=-inf) == EINVAL and f(alpha=nan) == EINVAL
    assert lib.dml_focal_loss_finalize(None, loss.data_ptr(), 1, st()) == EINVAL
    assert lib.dml_focal_loss_finalize(sums.data_ptr(), None, 1, st()) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(g.cpu().numpy()).all() and (sums.cpu().numpy() == 7.0).all() and (part.cpu().numpy() == 7.0).all()
    assert loss.item() == 7.0
    # a negative alpha and gamma = 0 are accepted
    assert fwd(alpha=-1.0, gamma=0.0) == 0 and bwd(alpha=-1.0, gamma=0.0) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("gamma", FC.GAMMAS)
def test_edges(lib, gamma):
    """nothing valid; one image of a batch all ignored; hand-built pixels with ce = 0 exactly, 1e-7, 50 and 90"""
    K = 16
    lg, lab = FC.inputs(K, "vec", 255)
    none = np.full_like(lab, 255)
    for size_average in (True, False):
        sums, loss, grad = run(lib, lg, none, 0.25, gamma, size_average, 255, gout=-2.5)
        assert loss == 0.0 and not grad.any() and sums[0] == 0.0 and sums[1] == 0.0 and sums[2] == lab.size and sums[3] == 0.0
    half = np.array(lab)
    half[1] = 255
    for size_average in (True, False):
        ref = FC.focal_ref(lg, half, 0.25, gamma, size_average, 255)
        got = run(lib, lg, half, 0.25, gamma, size_average, 255)
        check("gamma=%g one image ignored %s" % (gamma, "mean" if size_average else "sum"), got, ref)
        assert not got[2][1].any()
    elg, elab = FC.edge_frame(K)
    for size_average, gout in ((True, None), (False, -2.5)):
        ref = FC.focal_ref(elg, elab, 0.25, gamma, size_average, 255, gout=1.0 if gout is None else gout)
        sums, loss, grad = got = run(lib, elg, elab, 0.25, gamma, size_average, 255, gout=gout)
        check("gamma=%g hand-built ce in {0, 1e-7, 50, 90}" % gamma, got, ref)
        assert np.isfinite(grad).all() and np.isfinite(loss)
        # the u = 0 limit: the pixels with ce = 0 exactly have a zero gradient for every gamma (m = alpha at gamma = 0
        # multiplies softmax - onehot = 0), and the definition's m there is alpha or 0
        assert not grad[0, :, :, 0].any()
        assert (ref["m"][0, :, 0] == (0.25 if gamma == 0 else 0.0)).all()


def test_grid_stride(lib):
    """more pixels than one pass of the launch grid covers (2048 workgroups x 256 lanes x 4 pixels = 2 097 152) at K = 2:
    the loss and a seeded 1/64 sample of the pixels against the definition, the pixels beyond the first pass included"""
    B, K, Hh, Ww = 2, 2, 1024, 1100
    assert B * Hh * Ww > 2048 * 256 * 4
    lg, lab = FC.make_inputs("stride", B, K, Hh, Ww, FC.SIGMA[K], 255)
    ref = FC.focal_ref(lg, lab, 0.25, 2.0, True, 255, gout=-2.5)
    lt, yt = torch.from_numpy(lg).cuda(), torch.from_numpy(lab).cuda()
    sums = torch.empty(4, dtype=torch.float64, device="cuda")
    part = torch.empty(PARTIALS, dtype=torch.float32, device="cuda")
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    go = torch.tensor([-2.5], dtype=torch.float32, device="cuda")
    g = torch.full_like(lt, float("nan"))
    assert lib.dml_focal_loss_fwd(lt.data_ptr(), yt.data_ptr(), sums.data_ptr(), part.data_ptr(), B, K, Hh, Ww, 255, 0.25, 2.0, st()) == 0
    assert lib.dml_focal_loss_finalize(sums.data_ptr(), loss.data_ptr(), 1, st()) == 0
    assert lib.dml_focal_loss_bwd(lt.data_ptr(), yt.data_ptr(), sums.data_ptr(), go.data_ptr(), g.data_ptr(), B, K, Hh, Ww, 255,
                                  0.25, 2.0, 1, st()) == 0
    torch.cuda.synchronize()
    s, grad = sums.cpu().numpy(), g.cpu().numpy()
    assert s[1] == ref["sums"][1] and s[2] == B * Hh * Ww and s[3] == ref["sums"][3]
    e_loss = abs(F64(loss.item()) - ref["loss"])
    loss_bar = ref["loss_bar"] + 2.0 ** -24 * abs(ref["loss"])
    pick = H.rng_for(3, "focal.stride.sample").random((B, Hh, Ww)) < 1.0 / 64
    pick[1, -1, -8:] = True                                              # the last pixels of the tensor
    assert pick[1, 900:].any() and pick.sum() > 30000
    sel = np.broadcast_to(pick[:, None], grad.shape)
    err, bar = np.abs(grad.astype(F64) - ref["grad"])[sel], ref["grad_bar"][sel]
    pos = bar > 0
    print("MEASURE grid stride loss err=%.3e bar=%.3e err/bar=%.3e | gradient (%d elements) err=%.3e bar=%.3e worst err/bar=%.3e"
          % (e_loss, loss_bar, e_loss / loss_bar, err.size, err.max(), bar.max(), (err[pos] / bar[pos]).max()))
    assert e_loss <= loss_bar and abs(s[0] - ref["sums"][0]) <= ref["sum_bar"]
    assert (err <= bar).all() and (grad[sel][~pos] == 0).all()
    assert not np.isnan(grad).any()                                       # every element was written


@pytest.mark.parametrize("K,shape", [(13, "odd"), (16, "vec"), (19, "vec"), (33, "odd")])
def test_determinism(lib, K, shape):
    """two runs are bitwise equal; without the mean, an image's gradient inside a batch is its gradient alone"""
    lg, lab = FC.inputs(K, shape, 255)
    a = run(lib, lg, lab, 0.25, 2.0, True, 255, gout=-2.5)
    b = run(lib, lg, lab, 0.25, 2.0, True, 255, gout=-2.5)
    assert np.array_equal(bits(a[2]), bits(b[2])) and a[1] == b[1] and np.array_equal(a[0], b[0])
    batch = run(lib, lg, lab, 0.25, 0.5, False, 255)
    for i in range(lg.shape[0]):
        alone = run(lib, lg[i:i + 1], lab[i:i + 1], 0.25, 0.5, False, 255)
        assert np.array_equal(bits(alone[2][0]), bits(batch[2][i])), "image %d differs from its solo run" % i


def ce_mean_bars(lg, lab):
    """utils.CrossEntropyLoss(): sum nll / #valid / B in float64, with the bars of the definition at alpha = 1, gamma = 0 (the
    same per-pixel error model: nll = ce) scaled by the same divisor"""
    B = lg.shape[0]
    ref = FC.focal_ref(lg, lab, 1.0, 0.0, False, 255)
    d = ref["sums"][1] * B
    return ref["loss"] / d, ref["loss_bar"] / d, ref["grad"] / d, ref["grad_bar"] / d


@pytest.mark.parametrize("K,shape", [(16, "vec"), (19, "odd")])
def test_tie_to_the_cross_entropy_kernels(K, shape):
    """nothing ignored: FocalLoss(gamma=0, alpha=1) (sum nll / (B H W)) = B x CrossEntropyLoss() (sum nll / #valid / B), loss
    and gradient, within the sum of the two bars; CrossEntropyLoss(size_average=False) = sum nll / B"""
    import utils
    lg, lab_i = FC.inputs(K, shape, 255)
    lab = np.where(lab_i == 255, 0, lab_i)
    assert (lab != 255).all()
    B = lg.shape[0]
    x1 = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
    x2 = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
    y = torch.from_numpy(lab).cuda()
    fl = utils.FocalLoss(alpha=1, gamma=0, ignore_index=255)(x1, y)
    ce = utils.CrossEntropyLoss(ignore_index=255)(x2, y)
    fl.backward()
    ce.backward()
    f_ref = FC.focal_ref(lg, lab, 1.0, 0.0, True, 255)
    c_loss, c_lbar, c_grad, c_gbar = ce_mean_bars(lg, lab)
    assert abs(f_ref["loss"] - B * c_loss) <= 1e-12 * f_ref["loss"]              # the two definitions agree
    e = abs(F64(fl.item()) - B * F64(ce.item()))
    bar = f_ref["loss_bar"] + B * c_lbar + 2.0 ** -23 * f_ref["loss"]             # two float32 stores
    ge = np.abs(x1.grad.cpu().numpy().astype(F64) - B * x2.grad.cpu().numpy().astype(F64))
    gbar = f_ref["grad_bar"] + B * c_gbar
    print("MEASURE tie K=%d %s loss err=%.3e bar=%.3e err/bar=%.3e | gradient err=%.3e bar=%.3e worst err/bar=%.3e"
          % (K, shape, e, bar, e / bar, ge.max(), gbar.max(), (ge / gbar).max()))
    assert e <= bar and (ge <= gbar).all()
    # the sum reduction of the reference's CrossEntropyLoss: sum nll / n, the gradient materialised even with fused_backward
    yi = torch.from_numpy(np.array(lab_i)).cuda()
    s_ref = FC.focal_ref(lg, lab_i, 1.0, 0.0, False, 255, gout=1.0 / B)
    for fused in (False, True):
        x3 = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
        tot = utils.CrossEntropyLoss(ignore_index=255, size_average=False, fused_backward=fused)(x3, yi, None)
        tot.backward()
        e = abs(F64(tot.item()) - s_ref["loss"] / B)
        bar = s_ref["loss_bar"] / B + 2.0 ** -23 * s_ref["loss"] / B
        ge = np.abs(x3.grad.cpu().numpy().astype(F64) - s_ref["grad"])
        gbar = s_ref["grad_bar"] + 2.0 ** -24 * np.abs(s_ref["grad"])             # 1 / B is applied by a float32 multiplication
        print("MEASURE sum reduction K=%d %s loss err=%.3e bar=%.3e | gradient err=%.3e worst err/bar=%.3e"
              % (K, shape, e, bar, ge.max(), (ge[gbar > 0] / gbar[gbar > 0]).max()))
        assert e <= bar and (ge <= gbar).all()


def test_python_layer(lib):
    import utils
    K, shape = 16, "vec"
    lg, lab = FC.inputs(K, shape, 255)
    ref = FC.focal_ref(lg, lab, 0.25, 2.0, True, 255, gout=3.0)
    x = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
    y = torch.from_numpy(np.array(lab)).cuda()
    feats = torch.zeros(2, 8, 12, 16, device="cuda")
    crit = utils.FocalLoss(alpha=0.25, gamma=2, size_average=True, ignore_index=255)
    loss = crit(x, y, feats)                                              # the drivers' third argument is accepted and ignored
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    (3 * loss).backward()
    sums = np.array([ref["sums"][0], ref["sums"][1], ref["sums"][2], ref["sums"][3]])
    check("python layer, 3 x loss", (sums, loss.item(), x.grad.cpu().numpy()), ref)
    # the same bits as the C ABI with gout = 3
    direct = run(lib, lg, lab, 0.25, 2.0, True, 255, gout=3.0)
    assert np.array_equal(bits(direct[2]), bits(x.grad.cpu().numpy())) and direct[1] == np.float32(loss.item())
    # the reference's constructor order and defaults
    d = utils.FocalLoss()
    assert (d.alpha, d.gamma, d.size_average, d.ignore_index, d.sync) == (1.0, 0.0, True, 255, None)
    p = utils.FocalLoss(0.5, 1.5, False, -1)
    assert (p.alpha, p.gamma, p.size_average, p.ignore_index) == (0.5, 1.5, False, -1)
    for bad in (dict(gamma=-1), dict(gamma=float("nan")), dict(alpha=float("inf")), dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            utils.FocalLoss(**bad)
    with pytest.raises(RuntimeError):
        utils.FocalLoss(gamma=2)(torch.zeros(1, 13, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))    # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        utils.FocalLoss(gamma=2)(x, y[:, :4])                             # labels of another shape
    with pytest.raises(ValueError):
        utils.FocalLoss(gamma=2)(x[0], y[0])                              # not 4-D


SYNC_SCRIPT = r"""
import sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import focal_cases as FC
import utils
dist.init_process_group(backend="nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
lg, lab = FC.inputs(16, "vec", 255)
out = []
for sync in (None, True, dist.group.WORLD):
    for crit in (utils.FocalLoss(alpha=0.25, gamma=2, sync=sync), utils.FocalLoss(alpha=0.25, gamma=0.5, size_average=False, sync=sync),
                 utils.CrossEntropyLoss(size_average=False, sync=sync)):
        x = torch.from_numpy(np.array(lg)).cuda().requires_grad_(True)
        loss = crit(x, torch.from_numpy(np.array(lab)).cuda(), None)
        (3 * loss).backward()
        out.append((loss.detach().clone(), x.grad.clone()))
torch.cuda.synchronize()
for i in range(3):
    for j in (1, 2):
        assert torch.equal(out[i][0], out[3 * j + i][0]) and torch.equal(out[i][1], out[3 * j + i][1]), (i, j)
    assert torch.isfinite(out[i][0]) and out[i][1].abs().sum() > 0
dist.destroy_process_group()
print("SYNC-OK")
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sync_on_a_one_rank_group_is_bitwise_the_unsynchronised_loss():
    """sync=True (and an explicit group) on a forced single-rank RCCL group: the all-reduce of the four doubles is the
    identity, so loss and gradient equal sync=None bitwise.  A process of its own: a process group is process-wide state."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, "-c", SYNC_SCRIPT, os.path.join(H.ROOT, "tests")], capture_output=True, text=True,
                       cwd=H.PKG, timeout=600, env=env)
    assert r.returncode == 0 and "SYNC-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_model_train_step_with_the_focal_loss():
    """one train step of the embedding model at 2 x 3 x 64 x 64 under FocalLoss(gamma=2): every parameter gradient finite,
    and nonzero where the cross-entropy step's is"""
    import network
    import utils
    img = H.synth_tensor(5, "g5.img", (2, 3, 64, 64)).cuda()
    lab = H.synth_labels(5, "g5.lab", (2, 64, 64), 16, 255, ignore_rows=3).cuda()
    grads = {}
    for name, crit in (("ce", utils.CrossEntropyLoss(ignore_index=255)), ("focal", utils.FocalLoss(gamma=2, ignore_index=255))):
        m = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
        m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=1))
        m.cuda().train()
        lg, _, ft = m(img)
        loss = crit(lg, lab, ft)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss), name
        grads[name] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        del m
    assert grads["ce"].keys() == grads["focal"].keys()
    for k, g in grads["focal"].items():
        assert torch.isfinite(g).all(), k
        if grads["ce"][k].abs().sum() > 0:
            assert g.abs().sum() > 0, "%s has a zero gradient under the focal loss" % k


def test_driver_trains_with_the_focal_loss():
    """main_embedding.py --loss_type focal_loss end to end (--print_interval 1: the default of 10 prints nothing in 2 steps)"""
    drv = os.path.join(H.PKG, "main_embedding.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--loss_type", "focal_loss", "--focal_gamma", "2", "--batch_size", "2",
                        "--crop_size", "128", "--frame_height", "128", "--frame_width", "256", "--total_itrs", "2", "--dtype", "f32",
                        "--print_interval", "1"], capture_output=True, text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(ln.split("Loss=")[1].split(",")[0]) for ln in r.stdout.splitlines() if "Loss=" in ln]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), r.stdout[-2000:]
