"""Test infrastructure: a numpy restatement of Pillow's 8-bit BILINEAR resampler (libImaging/Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, ImagingResampleInner) and
of the reference's evaluation transform (anomaly/dataset.py: img_transform, segm_transform).  Written from the
arithmetic, loop by loop, so that it checks the product's vectorised tables instead of repeating them; pinned to live
Pillow by tests/test_pil_resize.py."""
import math

import numpy as np
import torch

PRECISION_BITS = 22
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def coeffs(in_size, out_size):
    """(bounds [out][2] = (xmin, n), fixed-point weights [out][ksize]) exactly as Resample.c builds them."""
    scale = float(in_size) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)          # C (int) truncates toward zero
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        ww = 0.0
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            wgt = 1.0 - t if t < 1.0 else 0.0
            k.append(wgt)
            ww += wgt
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(src, bounds, kk, axis):
    """One 8-bit pass along `axis` of an int array (the other axes ride along)."""
    src = np.moveaxis(src.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for i, (xmin, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for q in range(n):
            acc += src[xmin + q] * int(kk[i, q])
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31  # the C accumulator is int32
        out[i] = _clip8(acc)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """Image.fromarray(img).resize((W, H), Image.BILINEAR) for uint8 [h, w] or [h, w, 3]; size = (H, W)."""
    h, w = img.shape[:2]
    H, W = size
    if (H, W) == (h, w):
        return img.copy()
    vb, vk = coeffs(h, H)
    hb, hk = coeffs(w, W)
    first, last = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    tmp = img[first:last]
    if W != w:                                              # need_horizontal: only the rows the vertical pass reads
        tmp = _pass(tmp, hb, hk, axis=1)
    if H != h:
        vb = vb.copy()
        vb[:, 0] -= first
        tmp = _pass(tmp, vb, vk, axis=0)
    return tmp


def img_transform(img_u8):
    """dataset.py img_transform: np.float32(img) / 255., HWC -> CHW, Normalize (sub_ then div_ by fp32 mean / std)."""
    a = np.float32(np.array(img_u8)) / 255.
    t = torch.from_numpy(a.transpose((2, 0, 1)).copy())
    m = torch.as_tensor(MEAN, dtype=t.dtype)[:, None, None]
    s = torch.as_tensor(STD, dtype=t.dtype)[:, None, None]
    return t.sub_(m).div_(s)


def segm_transform(segm_u8):
    return torch.from_numpy(np.array(segm_u8)).long() - 1


def resized_shapes(h, w, img_sizes=(300, 375, 450, 525, 600), max_size=1000, padding=8):
    """ValDataset's target sizes (dataset.py:270-280)."""
    out = []
    for short in img_sizes:
        scale = min(short / float(min(h, w)), max_size / float(max(h, w)))
        th, tw = int(h * scale), int(w * scale)
        out.append((((th - 1) // padding + 1) * padding, ((tw - 1) // padding + 1) * padding))
    return out


def eval_inputs(img_u8, segm_u8, sizes):
    """(img_resized_list, seg_label) of ValDataset.__getitem__ for one frame, on the CPU."""
    return [img_transform(resize(img_u8, s))[None] for s in sizes], segm_transform(segm_u8)
