"""CPU: the edge cases of tests/aug_cases.py are what they are meant to be (every staging alignment, flipped and not, in first
and later segments; the partial last dword; the .5 pivot; a luminance sum that needs every segment), and the oracle they are
checked against equals the live Pillow on the new edge inputs."""
import numpy as np
import pytest

import helpers as H  # noqa: F401  (path setup)
import aug_cases as AC
from oracle import transforms_ref as TR


def test_width_cases_cover_segments_flips_and_alignments():
    assert set(AC.WIDTHS) == {1, 3, 4, 1023, 1024, 1025, 1028, 2053} and set(AC.HEIGHTS) == {1, 3}
    seen = set()
    for c in AC.width_cases():
        assert {p["flip"] for p in c.params} == {True, False}
        assert all(p["j"] > 0 for p in c.params) and c.img.shape[2] % 2 == 1
        seen |= AC.segment_shifts(c)
    for flip in (False, True):
        for later in (False, True):
            assert {s for f, l, s in seen if f == flip and l == later} == {0, 1, 2, 3}, (flip, later)
    assert -(-1028 // AC.SEG) == 2 and 1028 - AC.SEG == 4 and -(-2053 // AC.SEG) == 3 and 2053 % AC.SEG == 5
    assert -(-1024 // AC.SEG) == 1 and -(-1025 // AC.SEG) == 2


def test_order_cases_hold_every_order_and_position_of_the_contrast():
    for tw in AC.MULTI:
        c = AC.order_case(tw)
        codes = [tuple(o for o, _ in p["ops"]) for p in c.params]
        assert len({k for k in codes if len(k) == 3}) == 6
        assert () in codes and (1,) in codes and (0,) in codes                     # with and without a contrast op in one batch
        assert {k.index(1) for k in codes if 1 in k and len(k) == 2} == {0, 1}
        assert {p["flip"] for p in c.params} == {True, False}
        # the ops in front of the contrast change its pivot: the sum must be taken after them
        for p in c.params:
            k = [o for o, _ in p["ops"]]
            if 1 in k and k.index(1) > 0:
                crop = c.img[c.params.index(p)][p["i"]:p["i"] + 3, p["j"]:p["j"] + tw]
                x = crop
                for code, f in p["ops"][:k.index(1)]:
                    x = TR._ADJ[code](x, f)
                assert TR.contrast_mean(x) != TR.contrast_mean(crop)


def test_pivot_and_uniform_cases():
    c = AC.pivot_case()
    crop = c.img[0]
    assert TR.luma(crop).tolist() == [[10, 11]] and TR.contrast_mean(crop) == 11
    out = TR.adjust_contrast(crop, 0.5)
    assert out[0, :, 0].tolist() == [10, 11]                                       # a pivot of 10 would give [10, 10]
    assert TR.blend(np.full_like(crop, 10), crop, 0.5)[0, :, 0].tolist() == [10, 10]
    assert (TR.adjust_contrast(crop, 0.0) == 11).all()
    w = AC.white_case()
    assert w.crop == w.img.shape[1:3] and 64 * 2053 * 255 < 2 ** 32 and TR.contrast_mean(w.img[0]) == 255
    per_segment = 255 * 64 * 5                                                      # the last segment's share of the sum
    assert int((64 * 2053 * 255 - per_segment) / (64 * 2053) + 0.5) < 255          # losing even the ragged segment shows
    ref, _ = w.reference()
    one = ((np.float32(255) / np.float32(255) - np.asarray(AC.MEAN, np.float32)) / np.asarray(AC.STD, np.float32))
    assert (ref[0] == one[:, None, None]).all()
    u = AC.uniform_case()
    assert {(o, f) for p in u.params[:24] for o, f in p["ops"]} == {(o, f) for o in (0, 1, 2) for f in AC.EDGE_FACTORS}
    assert (u.img[:12] == 0).all() and (u.img[12:24] == 255).all()
    assert (TR.adjust_brightness(u.img[24], 1.5) == 255).all()                      # 300 clipped
    f = AC.full_frame_case()
    assert f.crop == f.img.shape[1:3]


def test_contraction_case_tells_a_fused_blend_apart():
    c = AC.contraction_case()
    img = c.img[0]
    grey = np.repeat(TR.luma(img)[..., None], 3, axis=-1)
    assert AC.fused_blend_differs(grey, img, 0.8).sum() > 100                       # saturation
    assert AC.fused_blend_differs(np.full_like(img, TR.contrast_mean(img)), img, 0.8).sum() > 100
    px = np.array([[[0, 179, 0]]], np.uint8)                                        # luma 105: 105 + 0.8 (0 - 105)
    assert TR.luma(px)[0, 0] == 105 and TR.adjust_saturation(px, 0.8)[0, 0, 0] == 21
    assert AC.fused_blend_differs(np.full_like(px, 105), px, 0.8)[0, 0, 0]


def test_last_pixel_cases_leave_a_partial_dword():
    rem = set()
    for c in AC.last_pixel_cases():
        B, Hh, Ww, _ = c.img.shape
        assert (B * Hh * Ww * 3) % 4 != 0
        rem.add((B * Hh * Ww) % 4)
        p = c.params[-1]
        assert p["i"] + c.crop[0] == Hh and p["j"] + c.crop[1] == Ww
    assert rem == {1, 2, 3}
    assert {c.params[-1]["flip"] for c in AC.last_pixel_cases()} == {True, False}
    for tw in AC.ALIGN_WIDTHS:
        assert tw % 4 == 0
    assert AC.compose_case().crop[1] == 1029 and {p["flip"] for p in AC.compose_case().params} == {True, False}


def test_reference_flip_is_the_mirror_of_the_unflipped_result():
    """a property of the oracle on the multi-segment width: flipping only mirrors (the jitter does not see it)"""
    c = AC.order_case(1025)
    ri, rl = c.reference()
    for b, p in enumerate(c.params):
        q = dict(p, flip=not p["flip"])
        oi, ol = TR.apply(c.img[b], c.lbl[b], q, c.crop, AC.MEAN, AC.STD)
        assert np.array_equal(oi[:, :, ::-1], ri[b]) and np.array_equal(ol[:, ::-1], rl[b])


def test_label_tables_are_not_the_identity():
    assert (AC.LUT != np.arange(256)).any() and (AC.LUT_TRUE != np.arange(256)).any() and (AC.LUT != AC.LUT_TRUE).any()
    assert set(AC.ENCODE_NS) == {1, 255, 256, 257, 6145}


def test_oracle_equals_live_pillow_on_the_edge_inputs():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    u = AC.uniform_case()
    inputs = [u.img[0], u.img[12], u.img[24], AC.pivot_case().img[0], u.img[25]]
    for a in inputs:
        im = Image.fromarray(a)
        assert np.array_equal(np.array(im.convert("L")), TR.luma(a))
        for f in AC.EDGE_FACTORS + (1.4999,):
            assert np.array_equal(np.array(ImageEnhance.Brightness(im).enhance(f)), TR.adjust_brightness(a, f))
            assert np.array_equal(np.array(ImageEnhance.Contrast(im).enhance(f)), TR.adjust_contrast(a, f))
            assert np.array_equal(np.array(ImageEnhance.Color(im).enhance(f)), TR.adjust_saturation(a, f))
