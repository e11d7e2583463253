"""Mint tests/golden/g16_scale_*.npz from the REFERENCE's own transform classes (authoring container only).

The reference's utils/ext_transforms.py is loaded by file path (mint_golden_aug.REF) and run unchanged through the
torchvision shim of mint_golden_aug.py, extended by the three functions the scale / pad / crop classes call, each forwarding
to the real Pillow exactly as torchvision 0.6.0 does (functional.py: resize -> Image.resize with the int rule for the smaller
edge, pad -> ImageOps.expand(border, fill=0), center_crop -> crop at int(round((size - crop) / 2.))).  The reference's
ExtResize names `collections.Iterable` without importing `collections`; the loaded module gets that name bound to
collections.abc.Iterable, nothing else is touched.  Outputs are data only: input image / label, the seed given to `random`,
the block as JSON settings ([class name, keyword arguments] pairs), and the tensors the reference pipeline returned.
"""
import collections.abc
import json
import numbers
import os
import random
import types

import numpy as np
from PIL import Image, ImageOps

import mint_golden_aug as A                     # installs the shim and loads the reference module as A.et

F, et = A.F, A.et


def _resize(img, size, interpolation=Image.BILINEAR):
    if isinstance(size, int):
        w, h = img.size
        if (w <= h and w == size) or (h <= w and h == size):
            return img
        if w < h:
            return img.resize((size, int(size * h / w)), interpolation)
        return img.resize((int(size * w / h), size), interpolation)
    return img.resize(tuple(size[::-1]), interpolation)


def _center_crop(img, output_size):
    if isinstance(output_size, numbers.Number):
        output_size = (int(output_size), int(output_size))
    w, h = img.size
    th, tw = output_size
    return F.crop(img, int(round((h - th) / 2.)), int(round((w - tw) / 2.)), th, tw)


F.resize = _resize
F.pad = lambda img, padding, fill=0, padding_mode="constant": ImageOps.expand(img, border=padding, fill=fill)
F.center_crop = _center_crop
et.collections = types.SimpleNamespace(Iterable=collections.abc.Iterable)

MEAN, STD = A.MEAN, A.STD
JITTER = ["ExtColorJitter", {"brightness": 0.5, "contrast": 0.5, "saturation": 0.5}]
TAIL = [["ExtToTensor", {}], ["ExtNormalize", {"mean": MEAN, "std": STD}]]


def run(name, seed, H, W, spec, raw_ids=False):
    rs = np.random.RandomState(seed)
    img = (rs.rand(H, W, 3) * 256).astype(np.uint8)
    img = (img.astype(np.float32) * rs.uniform(0.3, 1.0)).astype(np.uint8)
    # blocky content under the noise, so that a resize that is off by a source pixel shows
    img[H // 3:, : W // 2] //= 2
    if raw_ids:
        lbl = (rs.rand(H, W) * 34).astype(np.uint8)          # raw Cityscapes ids 0..33
    else:
        lbl = (rs.rand(H, W) * 19).astype(np.uint8)
        lbl[rs.rand(H, W) < 0.05] = 255
    spec = spec + TAIL
    tf = et.ExtCompose([getattr(et, cls)(**{k: (tuple(v) if isinstance(v, list) and k != "mean" and k != "std" else v)
                                            for k, v in kw.items()}) for cls, kw in spec])
    random.seed(seed)
    t, l = tf(Image.fromarray(img), Image.fromarray(lbl))
    out = os.path.join(A.ROOT, "tests", "golden", "g16_scale_%s.npz" % name)
    np.savez_compressed(out, seed=seed, img=img, lbl=lbl, spec=json.dumps(spec), out_img=t.numpy(), out_lbl=l.numpy())
    print(name, tuple(t.shape), tuple(l.shape), l.dtype, float(t.mean()), os.path.getsize(out))


if __name__ == "__main__":
    flip = ["ExtRandomHorizontalFlip", {}]
    # the scale-augmented train block (get_dataset of the reference's main.py): scale < 1, both pad_if_needed stages fire
    run("train_down", 31, 32, 44, [["ExtRandomScale", {"scale_range": [0.5, 0.55]}],
                                   ["ExtRandomCrop", {"size": [28, 30], "pad_if_needed": True}], JITTER, flip])
    # the same block, scale > 1: no padding
    run("train_up", 32, 32, 44, [["ExtRandomScale", {"scale_range": [1.5, 2.0]}],
                                 ["ExtRandomCrop", {"size": [24, 32], "pad_if_needed": True}], JITTER, flip])
    # a draw that pads the width only (all four borders, so the height grows too)
    run("train_onepad", 33, 32, 44, [["ExtRandomScale", {"scale_range": [0.7, 0.8]}],
                                     ["ExtRandomCrop", {"size": [20, 40], "pad_if_needed": True}], JITTER, flip])
    run("train_full", 34, 32, 44, [["ExtRandomScale", {"scale_range": [0.5, 2.0]}],
                                   ["ExtRandomCrop", {"size": 24, "pad_if_needed": True}], JITTER, flip])
    run("scale", 35, 32, 44, [["ExtScale", {"scale": 0.75}]])
    run("scale_up_flip", 36, 23, 31, [["ExtScale", {"scale": 1.3}], flip])
    run("resize_int", 37, 32, 44, [["ExtResize", {"size": 24}], flip])
    run("resize_int_tall", 38, 44, 32, [["ExtResize", {"size": 23}]])
    run("resize_pair", 39, 32, 44, [["ExtResize", {"size": [26, 38]}]])
    # --crop_val block; the crop is wider than the resized image (24 x 33)
    run("resize_center_wide", 40, 32, 44, [["ExtResize", {"size": 24}], ["ExtCenterCrop", {"size": [20, 40]}]])
    run("crop_val", 41, 32, 44, [["ExtResize", {"size": 24}], ["ExtCenterCrop", {"size": 24}]])
    run("center_only", 42, 25, 35, [["ExtCenterCrop", {"size": [29, 24]}]])
    run("crop_padding", 43, 32, 44, [["ExtRandomCrop", {"size": [20, 28], "padding": 3}], JITTER, flip])
    run("raw_ids", 44, 32, 44, [["ExtRandomScale", {"scale_range": [0.5, 0.6]}],
                                ["ExtRandomCrop", {"size": [28, 32], "pad_if_needed": True}], JITTER, flip], raw_ids=True)
