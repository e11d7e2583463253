"""GPU: the feature-distillation term -- dml_distill_fwd / _finalize / _bwd (csrc/distill_loss.hip) through the C ABI, through
utils.CrossEntropyLoss_dis, under the model's train step and under main_distillation.py.

Every float comparison is against the float64 definition of tests/distill_cases.py on the same float32 inputs (proved to be the
reference's statements, without a GPU, by tests/test_distill_refs.py), on EVERY element, to the bars derived there; an element
whose bar is 0 must be exactly 0, counts and labels are compared as integers.  Each float check prints
"MEASURE <case> err=<largest error> bar=<largest bar> worst err/bar=<largest ratio>" before it asserts.

Largest err/bar measured on an MI355X: see DESIGN.md 7j.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import distill_cases as DC
import helpers as H

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
F64 = np.float64
GUARD = 64                       # elements before and after an output: the output keeps its alignment
PARTIALS = 2 * 2048              # the documented size of block_partials, in floats
SENTINEL = -7                    # prefill of labels_out


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    assert _lib.DISTILL_PARTIALS == PARTIALS
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def shifted(host, shift, dtype):
    """a device copy of `host` that starts `shift` elements into a 256-byte aligned allocation -> (buffer, pointer)"""
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.zeros(host.size + shift, dtype=dtype, device="cuda")
    buf[shift:] = torch.from_numpy(np.array(host).ravel()).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + item * shift


def run(lib, t, s, lab, novel, lg=None, gout=None, shift=(0, 0, 0, 0, 0), inplace=False, n_images=None, ignore=DC.IGNORE):
    """the three entry points on host arrays -> (sums (2B+2,) float64, dis float32, gradient [B,H,W,Cs] float32, labels_out or
    None).  Every output is pre-filled (NaN, labels_out with SENTINEL) between two guards that must come back untouched;
    block_partials is guarded past its documented size; the inputs must come back unwritten.  `shift` moves the teacher /
    student / labels / gradient / teacher-logits pointers by that many elements.  n_images None: B is passed; 0: the kernels read
    it from sums."""
    B, Hh, Ww, Cs = s.shape
    Ct = t.shape[3]
    tbuf, tptr = shifted(t, shift[0], torch.float32)
    sbuf, sptr = shifted(s, shift[1], torch.float32)
    ybuf, yptr = shifted(lab, shift[2], torch.int64)
    n, px = s.size, lab.size
    gbuf = torch.full((n + 2 * GUARD + shift[3],), 7.0, dtype=torch.float32, device="cuda")
    glo = GUARD + shift[3]
    gbuf[glo:glo + n] = float("nan")
    ns = 2 * B + 2
    sums = torch.full((ns + 2,), 7.0, dtype=torch.float64, device="cuda")
    sums[1:1 + ns] = float("nan")
    part = torch.full((PARTIALS + GUARD,), 7.0, dtype=torch.float32, device="cuda")
    dis = torch.full((3,), 7.0, dtype=torch.float32, device="cuda")
    dis[1] = float("nan")
    go = None if gout is None else torch.tensor([gout], dtype=torch.float32, device="cuda")
    lptr = optr = None
    if lg is not None:
        lbuf, lptr = shifted(lg, shift[4], torch.float32)
        if inplace:
            optr = yptr
        else:
            obuf = torch.full((px + 2 * GUARD,), 7, dtype=torch.int64, device="cuda")
            obuf[GUARD:GUARD + px] = SENTINEL
            optr = obuf.data_ptr() + 8 * GUARD
    nim = float(B) if n_images is None else float(n_images)
    rc = lib.dml_distill_fwd(lptr, tptr, sptr, yptr, optr, sums.data_ptr() + 8, part.data_ptr(), B, Ct, Cs, Hh, Ww, ignore, novel, st())
    assert rc == 0, "dml_distill_fwd returned %d" % rc
    rc = lib.dml_distill_finalize(sums.data_ptr() + 8, B, nim, dis.data_ptr() + 4, st())
    assert rc == 0, "dml_distill_finalize returned %d" % rc
    rc = lib.dml_distill_bwd(tptr, sptr, yptr if optr is None else optr, sums.data_ptr() + 8, None if go is None else go.data_ptr(),
                             gbuf.data_ptr() + 4 * glo, B, Ct, Cs, Hh, Ww, novel, nim, st())
    assert rc == 0, "dml_distill_bwd returned %d" % rc
    torch.cuda.synchronize()
    g = gbuf.cpu().numpy()
    assert (g[:glo] == 7.0).all() and (g[glo + n:] == 7.0).all(), "a guard element of the gradient was written"
    sm = sums.cpu().numpy()
    assert sm[0] == 7.0 and sm[ns + 1] == 7.0, "a guard element of sums was written"
    ds = dis.cpu().numpy()
    assert ds[0] == 7.0 and ds[2] == 7.0, "a guard element of dis was written"
    assert (part[PARTIALS:].cpu().numpy() == 7.0).all(), "block_partials was written past 2 x 2048 floats"
    assert (tbuf[shift[0]:].cpu().numpy() == np.array(t).ravel()).all(), "the teacher features were written"
    assert (sbuf[shift[1]:].cpu().numpy() == np.array(s).ravel()).all(), "the student features were written"
    out = None
    if lg is not None:
        assert (lbuf[shift[4]:].cpu().numpy() == np.array(lg).ravel()).all(), "the teacher logits were written"
        if inplace:
            out = ybuf[shift[2]:].cpu().numpy().reshape(lab.shape)
        else:
            o = obuf.cpu().numpy()
            assert (o[:GUARD] == 7).all() and (o[GUARD + px:] == 7).all(), "a guard element of labels_out was written"
            out = o[GUARD:GUARD + px].reshape(lab.shape).copy()
    if lg is None or not inplace:
        assert (ybuf[shift[2]:].cpu().numpy() == np.array(lab).ravel()).all(), "the labels were written"
    return sm[1:1 + ns].copy(), ds[1], g[glo:glo + n].reshape(s.shape).copy(), out


def check(what, got, ref):
    """counts and labels exactly; S_i, their normalised sum, dis and every gradient element against the definition"""
    sums, dis, grad, labels_out = got
    B = ref["cnt"].size
    assert np.array_equal(sums[1:2 * B:2], ref["cnt"]) and sums[2 * B + 1] == B, (what, sums, ref["sums"])
    if labels_out is not None:
        assert np.array_equal(labels_out, ref["labels"]), "%s: %d labels differ" % (what, (labels_out != ref["labels"]).sum())
    e_S = np.abs(sums[0:2 * B:2] - ref["S"])
    e_tot, e_dis = abs(sums[2 * B] - ref["sums"][2 * B]), abs(F64(dis) - ref["dis"])
    err = np.abs(grad.astype(F64) - ref["grad"])
    bar = ref["grad_bar"]
    pos = bar > 0
    ratio = (err[pos] / bar[pos]).max(initial=0.0)
    spos = ref["S_bar"] > 0
    print("MEASURE %s dis err=%.3e bar=%.3e err/bar=%.3e | S_i worst err/bar=%.3e | gradient err=%.3e bar=%.3e worst err/bar=%.3e"
          % (what, e_dis, ref["dis_bar"], e_dis / ref["dis_bar"] if ref["dis_bar"] > 0 else 0.0,
             (e_S[spos] / ref["S_bar"][spos]).max(initial=0.0), err.max(), bar.max(), ratio))
    assert np.isfinite(grad).all() and np.isfinite(dis) and np.isfinite(sums).all(), what
    assert (e_S <= ref["S_bar"]).all(), (what, sums[0:2 * B:2], ref["S"])
    assert e_tot <= ref["total_bar"] and e_dis <= ref["dis_bar"], (what, dis, ref["dis"])
    assert (grad[~pos] == 0).all(), "%s: %d elements with a zero bar are not 0" % (what, (grad[~pos] != 0).sum())
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, "%s: %d gradient elements above the bar, first %s: got %s, want %s" % (
        what, bad.size, bad[:6], grad.ravel()[bad[:6]], ref["grad"].ravel()[bad[:6]])
    return ratio


def same_bits(a, b, what):
    assert np.array_equal(bits(a[0]), bits(b[0])), what + ": sums differ"
    assert bits(np.float32(a[1])) == bits(np.float32(b[1])), what + ": dis differs"
    assert np.array_equal(bits(a[2]), bits(b[2])), what + ": the gradient differs"
    assert (a[3] is None) == (b[3] is None) and (a[3] is None or np.array_equal(a[3], b[3])), what + ": labels_out differs"


CELLS = [(shape, ch) for shape in DC.SHAPES for ch in DC.CHANNELS]


@pytest.mark.parametrize("shape,ch", CELLS)
def test_c_abi_against_float64(lib, shape, ch):
    """t_logits NULL with gout NULL; the fill out of place with gout = -2.5; the fill in place (labels_out == labels_in), which
    must equal the out-of-place call in every bit; n read from sums[2B+1] instead of the argument"""
    t, s, lab, lg = DC.inputs(shape, ch)
    novel = DC.novel_of(ch[0])
    name = "%s Ct,Cs=%s" % (shape, ch)
    plain = run(lib, t, s, lab, novel)
    assert plain[3] is None
    check(name + " no logits, gout NULL", plain, DC.distill_ref(t, s, lab, novel))
    ref = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=lg, gout=-2.5)
    out = run(lib, t, s, lab, novel, lg=lg, gout=-2.5)
    check(name + " fill, gout=-2.5", out, ref)
    same_bits(run(lib, t, s, lab, novel, lg=lg, gout=-2.5, inplace=True), out, name + " in place")
    same_bits(run(lib, t, s, lab, novel, lg=lg, gout=-2.5, n_images=0), out, name + " n from sums")
    # a unit gout is the NULL one
    same_bits(run(lib, t, s, lab, novel, gout=1.0), plain, name + " gout=1")


@pytest.mark.parametrize("novel", (3, DC.IGNORE))
def test_a_novel_id_the_teacher_can_predict_or_equal_to_ignore_index(lib, novel):
    """novel_id inside the teacher's classes: a filled pixel is masked out where the teacher predicts it, so every lane that
    touches an ignored pixel needs the prediction, not only the one that writes it.  novel_id == ignore_index: without the fill
    the ignored pixels are masked out, with it they are all masked in."""
    t, s, lab, lg = DC.inputs((3, 33, 65), (16, 17))
    lab = np.where(lab == 16, 5, lab)
    for logits in (None, lg):
        ref = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=logits)
        if novel == 3 and logits is not None:
            assert ((lab == DC.IGNORE) & ~ref["mask"]).sum() > 20
        out = run(lib, t, s, lab, novel, lg=logits)
        check("novel_id=%d %s" % (novel, "fill" if logits is not None else "no logits"), out, ref)
        if logits is not None:
            same_bits(run(lib, t, s, lab, novel, lg=logits, inplace=True), out, "novel_id=%d in place" % novel)


@pytest.mark.parametrize("ch", DC.CHANNELS)
def test_shifted_pointers_take_the_scalar_path_bitwise(lib, ch):
    """2 x 64 x 64 takes the 16-byte path; each tensor in turn, then all, one element off (4 bytes, the labels 8): the same bits"""
    t, s, lab, lg = DC.inputs((2, 64, 64), ch)
    novel = DC.novel_of(ch[0])
    assert (s.size // 2) % 4 == 0
    ref = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=lg, gout=-2.5)
    aligned = run(lib, t, s, lab, novel, lg=lg, gout=-2.5)
    check("Ct,Cs=%s aligned" % (ch,), aligned, ref)
    for shift in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (3, 2, 1, 3, 2)):
        same_bits(run(lib, t, s, lab, novel, lg=lg, gout=-2.5, shift=shift), aligned, "Ct,Cs=%s shift %s" % (ch, shift))
    # an odd image size next to an even one: the scalar path inside a batch of the same pixels gives the image's own bits
    odd = DC.inputs((2, 5, 7), ch)
    a = run(lib, *odd[:3], novel, lg=odd[3])
    b = run(lib, *odd[:3], novel, lg=odd[3], shift=(1, 1, 1, 1, 1))
    same_bits(a, b, "Ct,Cs=%s odd shape shifted" % (ch,))


@pytest.mark.parametrize("ch", ((16, 17), (16, 16), (3, 8)))
def test_edges(lib, ch):
    """one image entirely novel: cnt = 0, contribution 0, gradient all zero, nothing NaN; one image entirely ignored"""
    t, s, lab, lg = DC.inputs((3, 33, 65), ch)
    novel = DC.novel_of(ch[0])
    lab = np.array(lab)
    lab[0] = novel
    lab[2] = DC.IGNORE
    for logits in (None, lg):
        ref = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=logits, gout=3.0)
        got = run(lib, t, s, lab, novel, lg=logits, gout=3.0)
        check("Ct,Cs=%s image 0 novel, image 2 ignored, %s" % (ch, "fill" if logits is not None else "no logits"), got, ref)
        sums, dis, grad, out = got
        assert sums[0] == 0.0 and sums[1] == 0.0 and not grad[0].any()
        assert sums[5] == 33 * 65 and grad[2].any()
        if out is not None:
            assert (out[0] == novel).all() and (out[2] < ch[0]).all() and (out[2] >= 0).all()
    # every image novel: dis = 0
    allnovel = np.full_like(lab, novel)
    sums, dis, grad, _ = run(lib, t, s, allnovel, novel, gout=3.0)
    assert dis == 0.0 and not grad.any() and not sums[:7].any() and sums[7] == 3


def test_grid_stride(lib):
    """1 x 360 x 360 x 17: more groups (550 800) than one pass of the image's 2048 workgroups covers (524 288), on the 16-byte
    path and, with the student one float off, on the scalar path"""
    B, Hh, Ww, Ct, Cs = 1, 360, 360, 16, 17
    assert (Hh * Ww * Cs) % 4 == 0 and Hh * Ww * Cs // 4 > 2048 * 256
    t, s, lab, lg = DC.make_inputs("stride", B, Hh, Ww, Ct, Cs, 16, DC.IGNORE)
    ref = DC.distill_ref(t, s, lab, 16, DC.IGNORE, t_logits=lg, gout=-2.5)
    assert DC.chain_depth(B, Hh, Ww, Cs) == 4 * 5 + 9              # without logits 2 groups per lane, with them 5 (one tile)
    got = run(lib, t, s, lab, 16, gout=-2.5)
    check("grid stride", got, DC.distill_ref(t, s, lab, 16, gout=-2.5))
    same_bits(run(lib, t, s, lab, 16, gout=-2.5, shift=(0, 1, 0, 0, 0)), got, "grid stride, scalar path")
    check("grid stride, fill", run(lib, t, s, lab, 16, lg=lg, gout=-2.5), ref)


def test_many_images_share_the_workgroups(lib):
    """1024 x 17 x 31 x 17: two workgroups per image (2048 / B), so a workgroup strides five times over the image's groups
    without logits and takes two of its three 256-pixel tiles with them; H W Cs is odd: the scalar path"""
    B, Hh, Ww, Ct, Cs = 1024, 17, 31, 16, 17
    t, s, lab, lg = DC.make_inputs("many", B, Hh, Ww, Ct, Cs, 16, DC.IGNORE)
    assert DC.chain_depth(B, Hh, Ww, Cs) == 4 * 10 + 9
    check("1024 images", run(lib, t, s, lab, 16, gout=-2.5), DC.distill_ref(t, s, lab, 16, gout=-2.5))
    ref = DC.distill_ref(t, s, lab, 16, DC.IGNORE, t_logits=lg, gout=-2.5)
    out = run(lib, t, s, lab, 16, lg=lg, gout=-2.5)
    check("1024 images, fill", out, ref)
    same_bits(run(lib, t, s, lab, 16, lg=lg, gout=-2.5, inplace=True), out, "1024 images, fill in place")


def test_determinism(lib):
    t, s, lab, lg = DC.inputs((3, 33, 65), (16, 17))
    a = run(lib, t, s, lab, 16, lg=lg, gout=-2.5)
    b = run(lib, t, s, lab, 16, lg=lg, gout=-2.5)
    same_bits(a, b, "two runs")


def test_error_codes(lib):
    """argument checks return before any launch: every output is still prefilled"""
    f = torch.full((4096,), -7.0, dtype=torch.float32, device="cuda")
    y = torch.zeros(256, dtype=torch.int64, device="cuda")
    yo = torch.full((256,), SENTINEL, dtype=torch.int64, device="cuda")
    sums = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    part = torch.full((PARTIALS,), 7.0, dtype=torch.float32, device="cuda")
    g = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    dis = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
    F, Y = f.data_ptr(), y.data_ptr()

    def fwd(lg=F, t=F, s=F, lab=Y, out=yo.data_ptr(), sm=sums.data_ptr(), p=part.data_ptr(), B=2, Ct=16, Cs=17, Hh=4, Ww=4):
        return lib.dml_distill_fwd(lg, t, s, lab, out, sm, p, B, Ct, Cs, Hh, Ww, 255, 16, st())

    def bwd(t=F, s=F, lab=Y, sm=sums.data_ptr(), out=g.data_ptr(), B=2, Ct=16, Cs=17, Hh=4, Ww=4):
        return lib.dml_distill_bwd(t, s, lab, sm, None, out, B, Ct, Cs, Hh, Ww, 16, 2.0, st())

    assert fwd(t=None) == EINVAL and fwd(s=None) == EINVAL and fwd(lab=None) == EINVAL and fwd(sm=None) == EINVAL
    assert fwd(p=None) == EINVAL and fwd(out=None) == EINVAL                 # labels_out is required with t_logits
    assert bwd(t=None) == EINVAL and bwd(s=None) == EINVAL and bwd(lab=None) == EINVAL and bwd(sm=None) == EINVAL
    assert bwd(out=None) == EINVAL
    for fn in (fwd, bwd):
        assert fn(B=0) == EINVAL and fn(B=-1) == EINVAL and fn(Hh=0) == EINVAL and fn(Ww=-1) == EINVAL
        assert fn(Ct=0) == EINVAL and fn(Ct=-1) == EINVAL and fn(Ct=17, Cs=16) == EINVAL and fn(Ct=18) == EINVAL
        assert fn(Cs=33) == EINVAL and fn(Ct=33, Cs=33) == EINVAL and fn(Ct=16, Cs=0) == EINVAL
        assert fn(B=2049) == EUNSUPPORTED and fn(Hh=1 << 15, Ww=1 << 12) == EUNSUPPORTED      # H W Cs >= 2^31
    assert lib.dml_distill_finalize(None, 2, 2.0, dis.data_ptr(), st()) == EINVAL
    assert lib.dml_distill_finalize(sums.data_ptr(), 2, 2.0, None, st()) == EINVAL
    assert lib.dml_distill_finalize(sums.data_ptr(), 0, 2.0, dis.data_ptr(), st()) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(g.cpu().numpy()).all() and (sums.cpu().numpy() == 7.0).all() and (part.cpu().numpy() == 7.0).all()
    assert dis.item() == 7.0 and (yo.cpu().numpy() == SENTINEL).all() and (y.cpu().numpy() == 0).all()
    # t_logits NULL: labels_out may be NULL too
    assert fwd(lg=None, out=None) == 0 and bwd() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# utils.CrossEntropyLoss_dis
# ---------------------------------------------------------------------------------------------------------------------------
def python_inputs():
    """2 x 64 x 64, 16 teacher and 17 student classes; student logits [B,17,H,W] = -|f - 3 e_k|^2 of the student features"""
    t, s, lab, lg = DC.inputs((2, 64, 64), (16, 17))
    sf = s.astype(F64)
    logits = -((sf[..., None, :] - 3.0 * np.eye(17)[None, None, None]) ** 2).sum(-1)
    logits = np.ascontiguousarray(logits.transpose(0, 3, 1, 2).astype(np.float32))
    return t, s, lab, lg, logits


def test_dis_weight_zero_is_the_cross_entropy_loss_bitwise():
    import utils
    t, s, lab, lg, logits = python_inputs()
    y = torch.from_numpy(np.array(lab)).cuda()
    f1 = torch.from_numpy(np.array(t)).cuda()
    outs = []
    for crit, args in ((utils.CrossEntropyLoss(ignore_index=255), None), (utils.CrossEntropyLoss_dis(ignore_index=255), "features"),
                       (utils.CrossEntropyLoss_dis(), "none")):
        x = torch.from_numpy(logits).cuda().requires_grad_(True)
        f2 = torch.from_numpy(np.array(s)).cuda().requires_grad_(True)
        loss = crit(x, y) if args is None else crit(x, y, f1, f2) if args == "features" else crit(x, y, None, None)
        (3 * loss).backward()
        assert f2.grad is None
        outs.append((loss.detach().clone(), x.grad.clone()))
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    assert torch.isfinite(outs[0][0]) and outs[0][1].abs().sum() > 0
    d = utils.CrossEntropyLoss_dis()
    assert (d.alpha, d.beta, d.gamma, d.size_average, d.ignore_index, d.dis_weight, d.novel_id, d.sync) == (0, 0, 0, True, 255, 0.0, 16, None)
    with pytest.raises(RuntimeError):
        utils.CrossEntropyLoss_dis(dis_weight=0.01)(torch.zeros(1, 17, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long),
                                                    torch.zeros(1, 4, 4, 16), torch.zeros(1, 4, 4, 17))     # CPU: no fallback
    with pytest.raises(ValueError):
        utils.CrossEntropyLoss_dis(dis_weight=0.01)(x, y, None, None)
    with pytest.raises(ValueError):
        utils.CrossEntropyLoss_dis(dis_weight=0.01)(x, y, f2.detach(), f1)                                   # teacher wider than student


@pytest.mark.parametrize("with_fill", (False, True))
def test_dis_weight_against_float64(lib, with_fill):
    """loss - CE = 0.01 dis and d loss / d features_2 = 0.01 d dis / d features_2 to the definition's bars (the weight reaches the
    backward as the float32 0.01: gout of the definition); the logit gradient is the cross entropy's, bit for bit"""
    import utils
    t, s, lab, lg, logits = python_inputs()
    w32 = float(np.float32(0.01))
    ref = DC.distill_ref(t, s, lab, 16, 255, t_logits=lg if with_fill else None, gout=w32)
    y = torch.from_numpy(np.array(lab)).cuda()
    f1 = torch.from_numpy(np.array(t)).cuda()
    tl = torch.from_numpy(np.array(lg)).cuda() if with_fill else None
    res = {}
    for w in (0.0, 0.01):
        x = torch.from_numpy(logits).cuda().requires_grad_(True)
        f2 = torch.from_numpy(np.array(s)).cuda().requires_grad_(True)
        loss = utils.CrossEntropyLoss_dis(dis_weight=w)(x, y, f1, f2, teacher_logits=tl)
        assert loss.shape == () and loss.dtype == torch.float32
        loss.backward()
        res[w] = (loss.item(), x.grad.clone(), None if f2.grad is None else f2.grad.cpu().numpy())
    assert res[0.0][2] is None and torch.equal(res[0.0][1], res[0.01][1])
    assert (y.cpu().numpy() == lab).all(), "the caller's labels were written"
    e = abs((F64(res[0.01][0]) - F64(res[0.0][0])) - 0.01 * ref["dis"])
    bar = 0.01 * ref["dis_bar"] + 2 * DC.EPS32 * (abs(res[0.01][0]) + 0.01 * ref["dis"])     # the product and the sum, in float32
    err = np.abs(res[0.01][2].astype(F64) - ref["grad"])
    pos = ref["grad_bar"] > 0
    print("MEASURE python fill=%s loss - CE err=%.3e bar=%.3e err/bar=%.3e | gradient err=%.3e bar=%.3e worst err/bar=%.3e"
          % (with_fill, e, bar, e / bar, err.max(), ref["grad_bar"].max(), (err[pos] / ref["grad_bar"][pos]).max()))
    assert e <= bar and (err <= ref["grad_bar"]).all() and (res[0.01][2][~pos] == 0).all()
    # the same bits as the C ABI with gout = float32(0.01)
    direct = run(lib, t, s, lab, 16, lg=lg if with_fill else None, gout=w32)
    assert np.array_equal(bits(direct[2]), bits(res[0.01][2]))


def test_teacher_logits_change_the_cross_entropy_as_the_filled_labels_do():
    import utils
    t, s, lab, lg, logits = python_inputs()
    filled = DC.fill(lab, lg, 255)
    assert (filled != lab).sum() > 500
    f1, f2 = torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(s)).cuda()
    out = {}
    for name, crit, labels, tl in (("fill", utils.CrossEntropyLoss_dis(), lab, lg), ("filled", utils.CrossEntropyLoss(), filled, None),
                                   ("plain", utils.CrossEntropyLoss_dis(), lab, None)):
        x = torch.from_numpy(logits).cuda().requires_grad_(True)
        y = torch.from_numpy(np.array(labels)).cuda()
        loss = crit(x, y) if name == "filled" else crit(x, y, f1, f2, teacher_logits=None if tl is None else torch.from_numpy(np.array(tl)).cuda())
        loss.backward()
        out[name] = (loss.detach().clone(), x.grad.clone())
    assert torch.equal(out["fill"][0], out["filled"][0]) and torch.equal(out["fill"][1], out["filled"][1])
    assert not torch.equal(out["fill"][0], out["plain"][0]) and not torch.equal(out["fill"][1], out["plain"][1])


SYNC_SCRIPT = r"""
import sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import distill_cases as DC
import utils
dist.init_process_group(backend="nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
t, s, lab, lg = DC.inputs((2, 64, 64), (16, 17))
logits = np.ascontiguousarray(np.concatenate([lg, lg[:, :1]], axis=1))
out = []
for sync in (None, True, dist.group.WORLD):
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    f2 = torch.from_numpy(np.array(s)).cuda().requires_grad_(True)
    loss = utils.CrossEntropyLoss_dis(dis_weight=0.01, sync=sync)(x, torch.from_numpy(np.array(lab)).cuda(), torch.from_numpy(np.array(t)).cuda(),
                                                                  f2, teacher_logits=torch.from_numpy(np.array(lg)).cuda())
    (3 * loss).backward()
    out.append((loss.detach().clone(), x.grad.clone(), f2.grad.clone()))
torch.cuda.synchronize()
for j in (1, 2):
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[j])), j
assert torch.isfinite(out[0][0]) and out[0][1].abs().sum() > 0 and out[0][2].abs().sum() > 0
dist.destroy_process_group()
print("SYNC-OK")
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sync_on_a_one_rank_group_is_bitwise_the_unsynchronised_loss():
    """sync=True (and an explicit group) on a forced single-rank RCCL group: the all-reduces are the identity and n is read from
    the device, so loss and both gradients equal sync=None bitwise.  A process of its own: a process group is process-wide state.
    More than one rank cannot be tested on one GPU."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, "-c", SYNC_SCRIPT, os.path.join(H.ROOT, "tests")], capture_output=True, text=True,
                       cwd=H.PKG, timeout=600, env=env)
    assert r.returncode == 0 and "SYNC-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------
# the model and the driver
# ---------------------------------------------------------------------------------------------------------------------------
def test_model_train_step_with_the_distillation_term():
    """2 x 3 x 64 x 64 (the smallest input of tests/test_gpu_model.py): a train-mode 17-class student under
    CrossEntropyLoss_dis(dis_weight=0.01) with the features of an eval() 16-class teacher, against the same step with the term
    composed from torch operators on features_2 -- every parameter gradient within 1e-3 of the tensor's largest element (the
    train step's bar of tests/test_gpu_model.py)"""
    import network
    import utils
    img = H.synth_tensor(5, "g5.img", (2, 3, 64, 64)).cuda()
    lab = H.synth_labels(5, "g5.lab", (2, 64, 64), 17, 255, ignore_rows=3).cuda()
    teacher = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
    teacher.load_state_dict(H.synth_state_dict(H.shapes_of(teacher), seed=1))
    teacher.cuda().eval()
    with torch.no_grad():
        _, _, f1 = teacher(img)
    assert tuple(f1.shape) == (2, 64, 64, 16)
    grads, losses = {}, {}
    for name in ("fused", "composed", "ce"):
        m = network.deeplabv3plus_embedding_resnet101(num_classes=17, output_stride=16, pretrained_backbone=False)
        m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=2))
        m.cuda().train()
        m.classifier.aspp.project[3].eval()
        lg, _, f2 = m(img)
        assert tuple(f2.shape) == (2, 64, 64, 17)
        if name == "fused":
            loss = utils.CrossEntropyLoss_dis(dis_weight=0.01)(lg, lab, f1, f2)
        elif name == "ce":
            loss = utils.CrossEntropyLoss_dis(dis_weight=0)(lg, lab, f1, f2)
        else:
            mask = (lab != 16).float()
            d = (f2 - torch.nn.functional.pad(f1, (0, 1))) * mask[..., None]
            dis = ((d * d).sum(dim=(1, 2, 3)) / mask.sum(dim=(1, 2))).sum() / 2
            loss = utils.CrossEntropyLoss()(lg, lab) + 0.01 * dis
        loss.backward()
        torch.cuda.synchronize()
        losses[name] = loss.item()
        grads[name] = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
        del m
    worst, where, moved = 0.0, None, 0.0
    for k, g in grads["composed"].items():
        scale = g.abs().max().item()
        assert np.isfinite(scale) and scale > 0, k
        r = (grads["fused"][k] - g).abs().max().item() / scale
        if r > worst:
            worst, where = r, k
        moved = max(moved, (grads["fused"][k] - grads["ce"][k]).abs().max().item() / scale)
    print("MEASURE model step: loss fused %.7f composed %.7f ce %.7f, worst parameter gradient err / max = %.3e (%s), bar 1e-3, "
          "ratio %.3e; the term moves a parameter gradient by up to %.3e of its max"
          % (losses["fused"], losses["composed"], losses["ce"], worst, where, worst / 1e-3, moved))
    assert abs(losses["fused"] - losses["composed"]) <= 1e-3 * abs(losses["composed"])
    assert worst <= 1e-3
    # the feature gradient reaches the parameters: far more than float32 rounding (6e-8) separates this step from the
    # cross-entropy step
    assert losses["fused"] > losses["ce"] and moved > 1e-5


def _drive(tmp, dis_weight):
    drv = os.path.join(H.PKG, "main_distillation.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--batch_size", "2", "--crop_size", "128", "--frame_height", "128",
                        "--frame_width", "256", "--total_itrs", "2", "--print_interval", "1", "--dtype", "f32", "--dis_weight",
                        str(dis_weight), "--pseudo_labels", "--save_interval", "2", "--save_dir", str(tmp)],
                       capture_output=True, text=True, cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(ln.split("Loss=")[1].split(",")[0]) for ln in r.stdout.splitlines() if "Loss=" in ln]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), r.stdout[-2000:]
    return losses


def test_driver_trains_with_and_without_the_distillation_term(tmp_path):
    """main_distillation.py end to end at 2 x 128 x 128 (the smallest crop the drivers' tests use): finite losses, the student's
    checkpoint in the reference's keys, and another loss with --dis_weight 0 on the same seed"""
    import network
    with_term = _drive(tmp_path / "a", 0.01)
    ck = torch.load(str(tmp_path / "a" / "latest_deeplabv3plus_embedding_resnet101_synthetic_os16.pth"), map_location="cpu")
    student = network.deeplabv3plus_embedding_resnet101(num_classes=17, output_stride=16, pretrained_backbone=False)
    assert list(ck["model_state"].keys()) == list(student.state_dict().keys())
    assert ck["model_state"]["classifier.classifier.3.weight"].shape[0] == 17 and ck["cur_itrs"] == 2
    assert all(torch.isfinite(v).all() for v in ck["model_state"].values() if v.is_floating_point())
    without = _drive(tmp_path / "b", 0)
    print("MEASURE driver losses with the term %s, without %s" % (with_term, without))
    assert with_term[0] != without[0]
