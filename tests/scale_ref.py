"""Test infrastructure: a CPU restatement of the reference's scale / resize / pad / crop transforms (utils/ext_transforms.py
there: ExtRandomScale, ExtScale, ExtResize, ExtCenterCrop, ExtRandomCrop with padding / pad_if_needed) on numpy arrays, stage
by stage as the reference runs them on PIL images -- resize the whole image, pad it, crop it -- so that it checks the
product's single-window reduction instead of repeating it.  BILINEAR is tests/pil_resample.py; NEAREST restates Pillow's
Geometry.c (ImagingScaleAffine: a double that starts at 0.5 * in / out and grows by in / out per output pixel, truncated);
jitter, flip and normalisation are oracle.transforms_ref.  Pinned to the reference by tests/golden/g16_scale_*.npz and to live
Pillow by tests/test_aug_scale.py.  The product never imports this module.

A transform block is a `spec`: a list of [class name, keyword arguments] pairs, the form the g16 fixtures store as JSON.
"""
import numpy as np

import pil_resample as PR
from oracle import transforms_ref as TR


def nearest_index(in_size, out_size):
    """Source index of every output pixel along one axis, the C loop restated."""
    step = float(in_size) / out_size
    xo = 0.0 + step * 0.5
    out = []
    for _ in range(out_size):
        out.append(-1 if xo < 0.0 else int(xo))
        xo += step
    return out


def resize_nearest(a, size):
    """Image.fromarray(a).resize((W, H), Image.NEAREST) for a uint8 [h, w] array; size = (H, W)."""
    h, w = a.shape[:2]
    H, W = size
    if (H, W) == (h, w):
        return a.copy()
    out = np.zeros((H, W) + a.shape[2:], a.dtype)
    cols = nearest_index(w, W)
    for y, sy in enumerate(nearest_index(h, H)):
        if not 0 <= sy < h:
            continue
        for x, sx in enumerate(cols):
            if 0 <= sx < w:
                out[y, x] = a[sy, sx]
    return out


def resize_target(stage, kw, h, w):
    """(H, W) that the resize stage asks for."""
    if stage == "ExtResize":
        size = kw["size"]
        if isinstance(size, int):                           # torchvision 0.6.0 functional.resize
            if (w <= h and w == size) or (h <= w and h == size):
                return h, w
            if w < h:
                return int(size * h / w), size
            return size, int(size * w / h)
        return int(size[0]), int(size[1])
    raise ValueError(stage)


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def pad_all(a, q):
    """F.pad(img, q): q zero pixels on all four borders."""
    return np.pad(a, ((q, q), (q, q)) + ((0, 0),) * (a.ndim - 2), mode="constant")


def crop(a, i, j, th, tw):
    """Image.crop((j, i, j + tw, i + th)): zeros outside the image."""
    h, w = a.shape[:2]
    out = np.zeros((th, tw) + a.shape[2:], a.dtype)
    y0, y1, x0, x1 = max(i, 0), min(i + th, h), max(j, 0), min(j + tw, w)
    if y1 > y0 and x1 > x0:
        out[y0 - i:y1 - i, x0 - j:x1 - j] = a[y0:y1, x0:x1]
    return out


def run(spec, img, lbl, rng, mean=PR.MEAN, std=PR.STD):
    """The block on one frame, drawing from `rng` as the reference draws from `random`.  Returns (float32 [3, th, tw] image,
    uint8 [th, tw] label, trace): trace holds what the product's host side must agree with -- the resized size, the window
    origin in the resized image, the output size, the jitter ops and the flip."""
    trace = {"size": img.shape[:2], "oy": 0, "ox": 0, "ops": [], "flip": False}
    names = [s[0] for s in spec]
    assert names[-2:] == ["ExtToTensor", "ExtNormalize"]
    for name, kw in spec[:-2]:
        h, w = img.shape[:2]
        if name in ("ExtRandomScale", "ExtScale", "ExtResize"):
            if name == "ExtRandomScale":
                scale = rng.uniform(kw["scale_range"][0], kw["scale_range"][1])
                tgt = (int(h * scale), int(w * scale))
            elif name == "ExtScale":
                tgt = (int(h * kw["scale"]), int(w * kw["scale"]))
            else:
                tgt = resize_target(name, kw, h, w)
            img, lbl = PR.resize(img, tgt), resize_nearest(lbl, tgt)
            trace["size"] = tgt
        elif name == "ExtRandomCrop":
            th, tw = _pair(kw["size"])
            py = px = 0
            if kw.get("padding", 0) > 0:
                img, lbl = pad_all(img, kw["padding"]), pad_all(lbl, kw["padding"])
                py, px = py + kw["padding"], px + kw["padding"]
            if kw.get("pad_if_needed", False) and img.shape[1] < tw:
                q = int((1 + tw - img.shape[1]) / 2)
                img, lbl = pad_all(img, q), pad_all(lbl, q)
                py, px = py + q, px + q
            if kw.get("pad_if_needed", False) and img.shape[0] < th:
                q = int((1 + th - img.shape[0]) / 2)
                img, lbl = pad_all(img, q), pad_all(lbl, q)
                py, px = py + q, px + q
            h, w = img.shape[:2]
            if w == tw and h == th:
                i, j = 0, 0
            else:
                i = rng.randint(0, h - th)
                j = rng.randint(0, w - tw)
            img, lbl = crop(img, i, j, th, tw), crop(lbl, i, j, th, tw)
            trace["oy"], trace["ox"] = i - py, j - px
        elif name == "ExtCenterCrop":
            th, tw = _pair(kw["size"])
            i, j = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
            img, lbl = crop(img, i, j, th, tw), crop(lbl, i, j, th, tw)
            trace["oy"], trace["ox"] = i, j
        elif name == "ExtColorJitter":
            ops = []
            for code, amount in ((TR.ORDER_B, kw.get("brightness", 0)), (TR.ORDER_C, kw.get("contrast", 0)),
                                 (TR.ORDER_S, kw.get("saturation", 0))):
                if amount:
                    ops.append((code, rng.uniform(max(0.0, 1.0 - amount), 1.0 + amount)))
            rng.shuffle(ops)
            trace["ops"] = ops
        elif name == "ExtRandomHorizontalFlip":
            trace["flip"] = bool(rng.random() < kw.get("p", 0.5))
        else:
            raise ValueError(name)
    trace["out"] = img.shape[:2]
    oi, ol = TR.apply(img, lbl, {"i": 0, "j": 0, "ops": trace["ops"], "flip": trace["flip"]}, img.shape[:2], mean, std)
    return oi, ol, trace


def window(img, lbl, size, oy, ox, out):
    """The uint8 window of forced parameters: resize to `size`, then the th x tw window at (oy, ox), zeros outside."""
    th, tw = out
    return crop(PR.resize(img, size), oy, ox, th, tw), crop(resize_nearest(lbl, size), oy, ox, th, tw)


def build(et, spec, **kw):
    """The same block from the classes of module `et` (the product's utils.ext_transforms)."""
    return et.ExtCompose([getattr(et, name)(**args) for name, args in spec], **kw)
