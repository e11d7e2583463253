"""Case table shared by tests/test_aug_refs.py (CPU) and tests/test_gpu_augment_edges.py (GPU): edge inputs of the device input
pipeline (csrc/augment.hip: dml_aug_contrast_sum, dml_aug_apply, dml_aug_apply_encoded, dml_label_encode) and their expected
outputs from oracle/transforms_ref.py, which is proved bit-exact against the reference's fixtures and the live Pillow
(tests/test_input_pipeline.py, tests/test_aug_refs.py).  A plain module (no fixtures, no hooks, numpy only); nothing here looks at
a kernel's output or imports the library.  Everything is compared for equality, image floats bit for bit.

A workgroup of the kernels covers SEG = 1024 output pixels of one crop row: widths up to 1024 are one segment, 1025 and 1028 two
(the second holding one pixel / exactly one full thread), 2053 three with a ragged last one.  A case is a batch: frames
img[B, H, W, 3] and labels lbl[B, H, W] (uint8), one crop size and one parameter dict per sample ({"i", "j", "ops", "flip"} as
TR.apply takes it; op codes 0 brightness, 1 contrast, 2 saturation)."""
import itertools

import numpy as np

import helpers as H  # noqa: F401  (path setup)
from oracle import transforms_ref as TR

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SEG = 1024
WIDTHS = (1, 3, 4, 1023, 1024, 1025, 1028, 2053)
HEIGHTS = (1, 3)
MULTI = (1025, 2053)                             # the widths of the contrast cases
FB, FC, FS = (0, 0.73), (1, 1.27), (2, 1.31)
EDGE_FACTORS = (0.0, 1.0, 0.5, 1.5)


class Case:
    def __init__(self, name, img, lbl, crop, params):
        self.name, self.img, self.lbl, self.crop, self.params = name, np.ascontiguousarray(img), np.ascontiguousarray(lbl), crop, params
        B, Hh, Ww, _ = self.img.shape
        assert self.lbl.shape == (B, Hh, Ww) and len(params) == B and self.img.dtype == np.uint8 and self.lbl.dtype == np.uint8
        for p in params:
            assert 0 <= p["i"] <= Hh - crop[0] and 0 <= p["j"] <= Ww - crop[1] and len(p["ops"]) <= 3
        self._ref = None

    def __repr__(self):
        return self.name

    def reference(self):
        """(images float32 [B, 3, th, tw], labels uint8 [B, th, tw]) -- computed once"""
        if self._ref is None:
            r = [TR.apply(self.img[b], self.lbl[b], self.params[b], self.crop, MEAN, STD) for b in range(len(self.params))]
            self._ref = (np.stack([a for a, _ in r]).astype(np.float32), np.stack([l for _, l in r]))
        return self._ref


def frames(B, Hh, Ww, seed):
    rs = np.random.RandomState(7000 + seed)
    return rs.randint(0, 256, (B, Hh, Ww, 3)).astype(np.uint8), rs.randint(0, 34, (B, Hh, Ww)).astype(np.uint8)


def P(i, j, ops, flip):
    return {"i": i, "j": j, "ops": list(ops), "flip": bool(flip)}


def width_case(tw, th):
    """an unflipped and a flipped sample, j > 0 and an odd W: the source rows start at every byte offset modulo 4"""
    Ww = tw + 4 if (tw + 4) % 2 else tw + 5
    img, lbl = frames(2, th + 2, Ww, tw + th)
    return Case("width tw=%d th=%d" % (tw, th), img, lbl, (th, tw),
                [P(1, 1 + tw % 3, [FB, FC, FS], False), P(2, 3, [(2, 0.5), (1, 1.5)], True)])


def width_cases():
    return [width_case(tw, th) for tw in WIDTHS for th in HEIGHTS]


def order_case(tw):
    """all six orders of the three ops, then 0 to 2 ops with the contrast first, last or absent; flips alternate"""
    opsets = [list(o) for o in itertools.permutations([FB, FC, FS])]
    opsets += [[], [FC], [FB], [FB, FC], [FC, FS], [FS, FB], [FS, FC], [FC, FB]]
    img, lbl = frames(len(opsets), 5, tw + 7, tw)
    return Case("orders tw=%d" % tw, img, lbl, (3, tw), [P(b % 3, 1 + b % 7, o, b % 2) for b, o in enumerate(opsets)])


def grey(values):
    v = np.asarray(values, np.uint8)
    return np.repeat(v[..., None], 3, axis=-1)


def pivot_case():
    """a 1 x 2 crop with lumas 10 and 11: mean 10.5, pivot int(10.5 + 0.5) = 11"""
    img = np.stack([grey([[10, 11]])] * 4)
    lbl = np.array([[[1, 2]]] * 4, np.uint8)
    return Case("pivot .5", img, lbl, (1, 2), [P(0, 0, [(1, 0.5)], False), P(0, 0, [(1, 0.0)], False), P(0, 0, [(1, 1.5)], True),
                                             P(0, 0, [(1, 0.5), (0, 1.0)], True)])


def uniform_case():
    """all-0 and all-255 frames under every single op at factors 0, 1, 0.5, 1.5; then factors above 1 that clip"""
    opsets = [[(code, f)] for code in (0, 1, 2) for f in EDGE_FACTORS]
    imgs, params = [], []
    for b, o in enumerate(opsets * 2):
        imgs.append(np.full((4, 9, 3), 0 if b < len(opsets) else 255, np.uint8))
        params.append(P(b % 2, b % 5, o, b % 3 == 0))
    rnd, _ = frames(2, 4, 9, 99)
    imgs += [np.full((4, 9, 3), 200, np.uint8), rnd[0], rnd[1]]
    params += [P(0, 0, [(0, 1.5)], False), P(1, 2, [(0, 1.5), (2, 1.5), (1, 1.5)], True), P(0, 4, [(2, 1.5), (1, 1.4999)], False)]
    lbl = frames(len(imgs), 4, 9, 98)[1]
    return Case("uniform frames", np.stack(imgs), lbl, (3, 5), params)


def white_case():
    """64 x 2053 all white, the crop the whole frame: the pivot is 255 only if no segment's share of the luminance sum is lost"""
    img = np.full((2, 64, 2053, 3), 255, np.uint8)
    lbl = frames(2, 64, 2053, 97)[1]
    return Case("white 64x2053", img, lbl, (64, 2053), [P(0, 0, [(1, 0.0)], False), P(0, 0, [(1, 0.5), (2, 1.5)], True)])


def contraction_case():
    """every (R, G, 0) pixel under a saturation and a contrast blend at 0.8: Pillow rounds the product and the sum separately;
    a fused multiply-add gives 20.999998 -> 20 for 105 + 0.8 (0 - 105) where Pillow has 21 (fused_blend_differs counts them)"""
    r, g = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.stack([r, g, np.zeros_like(r)], -1).astype(np.uint8)
    return Case("contraction", np.stack([img, img]), frames(2, 256, 256, 95)[1], (256, 256), [P(0, 0, [(2, 0.8)], False), P(0, 0, [(1, 0.8)], True)])


def fused_blend_differs(degenerate, img, factor):
    """elements where one rounding of a + f (b - a) (a fused multiply-add; exact in float64 for 8-bit a, b and a float32 f)
    truncates to another byte than Pillow's two roundings"""
    f = float(np.float32(factor))
    assert 0.0 <= f <= 1.0
    d, x = degenerate.astype(np.float64), img.astype(np.float64)
    fused = (d + f * (x - d)).astype(np.float32).astype(np.uint8)
    return fused != TR.blend(degenerate, img, factor)


def full_frame_case():
    img, lbl = frames(3, 5, 7, 96)
    return Case("crop equals frame", img, lbl, (5, 7), [P(0, 0, [FC, FS], False), P(0, 0, [FS, FB, FC], True), P(0, 0, [], True)])


def last_pixel_cases():
    """the crop ends on the last pixel of the last frame and B H W 3 is no multiple of 4: the last dword of the batch is partial"""
    out = []
    for Hh, Ww, crop in ((3, 5, (2, 3)), (2, 7, (1, 4)), (3, 7, (2, 5)), (1, 1, (1, 1)), (1, 3, (1, 3))):
        for flip in (False, True):
            img, lbl = frames(3, Hh, Ww, 90 + Hh * Ww)
            i, j = Hh - crop[0], Ww - crop[1]
            out.append(Case("last pixel %dx%d flip=%d" % (Hh, Ww, flip), img, lbl, crop,
                            [P(0, 0, [FC], not flip), P(i, j, [FS, FC], flip), P(i, j, [FB, FC, FS], flip)]))
    return out


ALIGN_WIDTHS = (4, 8, 1028)


def align_case(tw):
    img, lbl = frames(2, 4, tw + 3, 80 + tw)
    return Case("alignment tw=%d" % tw, img, lbl, (3, tw), [P(1, 2, [FB, FC, FS], False), P(0, 3, [FC], True)])


def compose_case():
    """through utils.ext_transforms.ExtCompose(..., params=...): 1029 = 1024 + 5"""
    img, lbl = frames(3, 5, 1035, 70)
    return Case("compose 1029", img, lbl, (3, 1029), [P(0, 0, [FB, FC, FS], False), P(2, 6, [FS, FC], True), P(1, 3, [], True)])


def all_cases():
    return (width_cases() + [order_case(tw) for tw in MULTI] + [pivot_case(), uniform_case(), white_case(), full_frame_case(), contraction_case()]
            + last_pixel_cases() + [align_case(tw) for tw in ALIGN_WIDTHS] + [compose_case()])


def segment_shifts(case):
    """byte offset modulo 4 of the first source byte of every (sample, row, segment), for a 4-byte aligned batch: the four staging
    alignments; used only to assert that the cases cover them"""
    B, Hh, Ww, _ = case.img.shape
    th, tw = case.crop
    out = set()
    for b, p in enumerate(case.params):
        for y in range(th):
            for x0 in range(0, tw, SEG):
                n = min(SEG, tw - x0)
                c0 = tw - x0 - n if p["flip"] else x0
                out.add((bool(p["flip"]), x0 > 0, (((b * Hh + p["i"] + y) * Ww + p["j"] + c0) * 3) % 4))
    return out


# label tables that are not the identity, and label_encode sizes
LUT = ((np.arange(256) * 7 + 3) % 256).astype(np.uint8)
LUT_TRUE = (255 - np.arange(256)).astype(np.uint8)
ENCODE_NS = (1, 255, 256, 257, 2048 * 3 + 1)


def raw_labels(n):
    return np.random.RandomState(7500 + n).randint(0, 256, n).astype(np.uint8)
