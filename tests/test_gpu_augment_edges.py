"""GPU: the input-pipeline kernels of csrc/augment.hip (dml_aug_contrast_sum, dml_aug_apply, dml_aug_apply_encoded,
dml_label_encode) at their edges, through the C ABI -- every case of tests/aug_cases.py.

Every output is compared for equality with oracle/transforms_ref.py on the same bytes (image floats bit for bit, labels as
integers), and sits between two guard regions of 0xAA bytes that must be bitwise unchanged afterwards; an output the call must
not write (no labels given, a refused call) is all 0xAA afterwards.  The luminance sums start as garbage: the call zeroes them.

Measured on the MI355X: the whole file, 20 tests, takes about 1.2 s there (the slowest test 0.1 s); every case equal, every
guard byte intact.  There are no bars here: nothing but equality is accepted.  No kernel had to be changed.

Tried on a scratch copy, one single-line change at a time, each caught by this file:
  c0 = x0 for flipped rows in stage_row            every width above 1024 (1025, 1028, 1029 through ExtCompose, 2053), nothing below
  the ops before the contrast op dropped in aug_contrast_sum_kernel      every case whose contrast is not the first op
  + 0.5 removed from the pivot                     the .5 pivot case and most random crops
  fp contract(off) removed from blend1             only the (R, G, 0) sweep of aug_cases.contraction_case -- the random crops and
                                                   the uniform frames all passed, so that case was added
  lsum[b] = t for the atomicAdd                    every case with more than one row or segment
  the partial last dword assembled in the wrong byte order      the last-pixel cases (and the 1 x 2 pivot frame, 6 bytes)
  lut for lut_true in the second label output      the label-table cases
  lab[3], lab[2] swapped in the 16-byte label store      every tw % 4 == 0 case with aligned outputs
NOT caught, and not catchable: `t >= 256.f` for `t >= 255.f` in blend1's clip -- a t in [255, 256) truncates to 255 either way.
"""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import aug_cases as AC

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
GUARD = 1024                                   # guard bytes before and after


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def chk(rc):
    assert rc == 0, "kernel returned %d" % rc
    torch.cuda.synchronize()


class Out:
    """GUARD bytes, `lead` elements, n elements of `tdt`, GUARD bytes on the device, every byte 0xAA; `lead` moves the addressed
    elements off the allocation's alignment"""

    def __init__(self, n, tdt, lead=0):
        es = torch.empty((), dtype=tdt).element_size()
        self.lo, self.hi = GUARD + lead * es, GUARD + (lead + n) * es
        self.raw = torch.full((self.hi + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        self.t = self.raw[self.lo:self.hi].view(tdt)
        self.ptr = self.t.data_ptr()

    def numpy(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        assert bool((self.raw[:self.lo] == 0xAA).all()) and bool((self.raw[self.hi:] == 0xAA).all()), "a byte outside the output was written"

    def untouched(self):
        assert bool((self.raw == 0xAA).all()), "a buffer the call must not write was written"


def pack_samples(params):
    from dmlnet._lib import AugSample
    arr = (AugSample * len(params))()
    for b, p in enumerate(params):
        a = arr[b]
        a.i, a.j, a.flip, a.n_ops = p["i"], p["j"], int(p["flip"]), len(p["ops"])
        for k, (code, f) in enumerate(p["ops"]):
            a.op[k], a.factor[k] = code, f
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def same_floats(what, got, ref):
    got, ref = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(ref, np.float32).view(np.uint32)
    bad = got.reshape(-1) != ref.reshape(-1)
    assert not bad.any(), "%s: %d of %d image floats differ bitwise, the first at %d" % (what, int(bad.sum()), bad.size, int(np.argmax(bad)))


def same_ints(what, got, ref):
    bad = np.asarray(got).reshape(-1) != np.asarray(ref).astype(np.int64).reshape(-1)
    assert not bad.any(), "%s: %d of %d labels differ, the first at %d" % (what, int(bad.sum()), bad.size, int(np.argmax(bad)))


def run(lib, case, lead_img=0, lead_lbl=0, labels=True, luts=None, true_out=True, lsum=None):
    """contrast sum + apply on one batch; returns the luminance-sum buffer for reuse"""
    B, Hh, Ww, _ = case.img.shape
    th, tw = case.crop
    img, lbl = torch.from_numpy(case.img).cuda(), torch.from_numpy(case.lbl).cuda()
    smp = pack_samples(case.params)
    lsum = lsum or Out(B, torch.int32)
    assert lsum.t.numel() == B
    oi, ol, ot = Out(B * 3 * th * tw, torch.float32, lead_img), Out(B * th * tw, torch.int64, lead_lbl), Out(B * th * tw, torch.int64)
    chk(lib.dml_aug_contrast_sum(img.data_ptr(), smp.data_ptr(), lsum.ptr, B, Hh, Ww, th, tw, st()))
    m, s = AC.MEAN, AC.STD
    if luts is None:
        chk(lib.dml_aug_apply(img.data_ptr(), lbl.data_ptr() if labels else None, smp.data_ptr(), lsum.ptr, oi.ptr, ol.ptr, B, Hh, Ww,
                              th, tw, m[0], m[1], m[2], s[0], s[1], s[2], st()))
    else:
        lut, lut_true = (torch.from_numpy(t).cuda() if t is not None else None for t in luts)
        chk(lib.dml_aug_apply_encoded(img.data_ptr(), lbl.data_ptr(), smp.data_ptr(), lsum.ptr, oi.ptr, ol.ptr, B, Hh, Ww, th, tw,
                                      m[0], m[1], m[2], s[0], s[1], s[2], lut.data_ptr(), lut_true.data_ptr() if lut_true is not None else None,
                                      ot.ptr if true_out else None, st()))
    ri, rl = case.reference()
    what = "%s lead=(%d, %d)" % (case.name, lead_img, lead_lbl)
    same_floats(what, oi.numpy(), ri)
    oi.guards_intact(), lsum.guards_intact()
    if not labels:
        ol.untouched()
    elif luts is None:
        same_ints(what, ol.numpy(), rl)
        ol.guards_intact()
    else:
        same_ints(what + " lut", ol.numpy(), luts[0][rl])
        ol.guards_intact()
    if luts is not None and true_out:
        same_ints(what + " lut_true", ot.numpy(), (luts[1] if luts[1] is not None else np.arange(256))[rl])
        ot.guards_intact()
    else:
        ot.untouched()
    assert np.array_equal(img.cpu().numpy(), case.img) and np.array_equal(lbl.cpu().numpy(), case.lbl)
    return lsum


@pytest.mark.parametrize("tw", AC.WIDTHS)
def test_widths_with_and_without_flip(lib, tw):
    """1 to 4 pixels, one full segment and one pixel less, a second segment of one pixel / one full thread, three segments with a
    ragged last one; th = 1 and 3; an unflipped and a flipped sample each: the mirrored start of a later segment"""
    for th in AC.HEIGHTS:
        run(lib, AC.width_case(tw, th))


@pytest.mark.parametrize("tw", AC.MULTI)
def test_contrast_position_on_several_segments(lib, tw):
    """every order of the three ops and 0 to 2 ops, with and without a contrast op in one batch: the luminance sum is folded from
    several segments and taken after the ops in front of the contrast.  The same garbage-filled sum buffer serves two calls."""
    case = AC.order_case(tw)
    lsum = run(lib, case)
    other = AC.Case(case.name + " reversed", case.img[::-1], case.lbl[::-1], case.crop, case.params[::-1])
    run(lib, other, lsum=lsum)


def test_pivot_uniform_white_and_full_frame(lib):
    """a mean luminance of exactly 10.5; all-0 and all-255 frames at factors 0, 1, 0.5, 1.5 and a clipping factor; 64 x 2053 white
    pixels whose pivot must be exactly 255; a crop equal to the frame"""
    for case in (AC.pivot_case(), AC.uniform_case(), AC.white_case(), AC.full_frame_case()):
        run(lib, case)


def test_blend_rounds_product_and_sum_separately(lib):
    """all (R, G, 0) pixels under a saturation and a contrast blend at 0.8: hundreds of them truncate to another byte under a
    fused multiply-add"""
    run(lib, AC.contraction_case())


def test_partial_last_dword_of_the_batch(lib):
    """B H W 3 % 4 in {1, 2, 3} and a crop that ends on the last pixel of the last frame, flipped and not: the values only"""
    for case in AC.last_pixel_cases():
        run(lib, case)


@pytest.mark.parametrize("tw", AC.ALIGN_WIDTHS)
def test_outputs_off_16_byte_alignment(lib, tw):
    """tw % 4 == 0 with the image one float off, the labels one int64 off, and both: the scalar stores give the aligned result"""
    case = AC.align_case(tw)
    for lead_img, lead_lbl in ((0, 0), (1, 0), (0, 1), (1, 1), (3, 1)):
        run(lib, case, lead_img, lead_lbl)
        run(lib, case, lead_img, lead_lbl, luts=(AC.LUT, AC.LUT_TRUE))


def test_without_labels_and_with_label_tables(lib):
    for case in (AC.width_case(1025, 3), AC.width_case(3, 1), AC.align_case(8)):
        run(lib, case, labels=False)
        run(lib, case, luts=(AC.LUT, AC.LUT_TRUE))
        run(lib, case, luts=(AC.LUT, None))                           # no second table: the raw id
        run(lib, case, luts=(AC.LUT, AC.LUT_TRUE), true_out=False)
        run(lib, case, luts=(AC.LUT, None), true_out=False)


def test_label_encode(lib):
    lut, lut_true = torch.from_numpy(AC.LUT).cuda(), torch.from_numpy(AC.LUT_TRUE).cuda()
    for n in AC.ENCODE_NS:
        raw = AC.raw_labels(n)
        r = torch.from_numpy(raw).cuda()
        o, t = Out(n, torch.int64), Out(n, torch.int64)
        chk(lib.dml_label_encode(r.data_ptr(), n, lut.data_ptr(), lut_true.data_ptr(), o.ptr, t.ptr, st()))
        same_ints("label_encode n=%d" % n, o.numpy(), AC.LUT[raw])
        same_ints("label_encode true n=%d" % n, t.numpy(), AC.LUT_TRUE[raw])
        o.guards_intact(), t.guards_intact()
        o, t = Out(n, torch.int64), Out(n, torch.int64)
        chk(lib.dml_label_encode(r.data_ptr(), n, lut.data_ptr(), None, o.ptr, None, st()))
        same_ints("label_encode without out_true n=%d" % n, o.numpy(), AC.LUT[raw])
        o.guards_intact(), t.untouched()
        o = Out(n, torch.int64)
        chk(lib.dml_label_encode(r.data_ptr(), n, lut.data_ptr(), lut_true.data_ptr(), o.ptr, None, st()))
        same_ints("label_encode with an unused table n=%d" % n, o.numpy(), AC.LUT[raw])
        o.guards_intact()
    o, t = Out(4, torch.int64), Out(4, torch.int64)
    chk(lib.dml_label_encode(r.data_ptr(), 0, lut.data_ptr(), lut_true.data_ptr(), o.ptr, t.ptr, st()))          # n = 0: nothing
    assert lib.dml_label_encode(r.data_ptr(), 4, lut.data_ptr(), None, o.ptr, t.ptr, st()) == EINVAL              # out_true without lut_true
    assert lib.dml_label_encode(None, 4, lut.data_ptr(), None, o.ptr, None, st()) == EINVAL
    assert lib.dml_label_encode(r.data_ptr(), 4, None, None, o.ptr, None, st()) == EINVAL
    assert lib.dml_label_encode(r.data_ptr(), 4, lut.data_ptr(), None, None, None, st()) == EINVAL
    assert lib.dml_label_encode(r.data_ptr(), -1, lut.data_ptr(), None, o.ptr, None, st()) == EINVAL
    torch.cuda.synchronize()
    o.untouched(), t.untouched()


def test_refusals_leave_the_outputs_alone(lib):
    case = AC.full_frame_case()
    B, Hh, Ww, _ = case.img.shape
    th, tw = case.crop
    img, lbl, smp = torch.from_numpy(case.img).cuda(), torch.from_numpy(case.lbl).cuda(), pack_samples(case.params)
    lut = torch.from_numpy(AC.LUT).cuda()
    lsum, oi, ol, ot = Out(B, torch.int32), Out(B * 3 * th * tw, torch.float32), Out(B * th * tw, torch.int64), Out(B * th * tw, torch.int64)
    m, s = AC.MEAN, AC.STD

    def csum(i=img.data_ptr(), p=smp.data_ptr(), l=lsum.ptr, b=B, hh=Hh, ww=Ww, h=th, w=tw):
        return lib.dml_aug_contrast_sum(i, p, l, b, hh, ww, h, w, st())

    def apply(i=img.data_ptr(), lb=lbl.data_ptr(), p=smp.data_ptr(), l=lsum.ptr, o=oi.ptr, olb=ol.ptr, b=B, hh=Hh, ww=Ww, h=th, w=tw, sd=s):
        return lib.dml_aug_apply(i, lb, p, l, o, olb, b, hh, ww, h, w, m[0], m[1], m[2], sd[0], sd[1], sd[2], st())

    def enc(i=img.data_ptr(), lb=lbl.data_ptr(), p=smp.data_ptr(), l=lsum.ptr, o=oi.ptr, olb=ol.ptr, b=B, hh=Hh, ww=Ww, h=th, w=tw, sd=s,
            lu=lut.data_ptr()):
        return lib.dml_aug_apply_encoded(i, lb, p, l, o, olb, b, hh, ww, h, w, m[0], m[1], m[2], sd[0], sd[1], sd[2], lu, None, ot.ptr, st())

    for fn in (csum, apply, enc):
        assert fn(h=Hh + 1) == EINVAL and fn(w=Ww + 1) == EINVAL                  # th > H, tw > W
        assert fn(b=0) == EINVAL and fn(h=0) == EINVAL and fn(w=0) == EINVAL and fn(b=-1) == EINVAL
        assert fn(i=None) == EINVAL and fn(p=None) == EINVAL and fn(l=None) == EINVAL
    for fn in (apply, enc):
        assert fn(o=None) == EINVAL
        for k in range(3):
            sd = list(s)
            sd[k] = 0.0
            assert fn(sd=sd) == EINVAL                                            # a zero std
    assert enc(lb=None) == EINVAL and enc(olb=None) == EINVAL and enc(lu=None) == EINVAL
    # th * tw * 255 >= 2^32 does not fit the uint32 luminance sum: refused before any launch (H, W, th, tw are plain integers)
    assert csum(hh=4105, ww=4105, h=4105, w=4105) == EUNSUPPORTED
    assert csum(hh=1, ww=16843010, h=1, w=16843010) == EUNSUPPORTED
    torch.cuda.synchronize()
    for b in (lsum, oi, ol, ot):
        b.untouched()


def test_compose_packs_the_samples_at_a_multi_segment_width():
    """utils.ext_transforms.ExtCompose(..., params=...) at tw = 1029 with flipped and unflipped samples"""
    import utils
    et = utils.ext_transforms
    case = AC.compose_case()
    tf = et.ExtCompose([et.ExtRandomCrop(size=case.crop), et.ExtColorJitter(brightness=0.5, contrast=0.5, saturation=0.5),
                        et.ExtRandomHorizontalFlip(), et.ExtToTensor(), et.ExtNormalize(mean=AC.MEAN, std=AC.STD)])
    out, olb = tf(torch.from_numpy(case.img).cuda(), torch.from_numpy(case.lbl).cuda(), params=case.params)
    torch.cuda.synchronize()
    ri, rl = case.reference()
    assert out.dtype == torch.float32 and olb.dtype == torch.int64
    same_floats(case.name, out.cpu().numpy(), ri)
    same_ints(case.name, olb.cpu().numpy(), rl)
