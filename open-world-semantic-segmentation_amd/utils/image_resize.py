"""The evaluation input of the anomaly sub-project on the device: Pillow's BILINEAR `Image.resize` of a uint8 RGB frame to
every scale of the multi-scale test, then ToTensor + Normalize (anomaly/dataset.py:249-300 of the reference,
`img_transform(imresize(img, (W_s, H_s), 'bilinear'))`), bit for bit, in one launch (dml_pil_resize_normalize).

The per-axis coefficient tables are Pillow's (libImaging/Resample.c, precompute_coeffs + normalize_coeffs_8bpc): built
here in double, rounded to fixed point with 22 fraction bits, and cached on the device per (frame size, target sizes).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from dmlnet import _lib

PRECISION_BITS = 22
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_LDS_ROWS_MAX = 256          # source rows one workgroup can hold (csrc/image_resize.hip)
_BAND_TW = 64                # output columns per workgroup


def resample_coeffs(in_size: int, out_size: int):
    """Pillow's BILINEAR coefficients of one axis: bounds int32 [out, 2] = (first source index, tap count) and the
    fixed-point weights int32 [out, ksize] (zero past the tap count)."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError("resample_coeffs: sizes must be positive")
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                             # bilinear support 1.0
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.int64)
    t = np.abs(((taps[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (taps[None, :] < xmax[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(out_size)
    for k in range(ksize):                                  # the C loop's summation order, tap by tap
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fx = w * float(1 << PRECISION_BITS)
    coef = np.trunc(np.where(w < 0, fx - 0.5, fx + 0.5)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return bounds, coef


def _band_rows(vbounds):
    """Output rows per workgroup: the largest of 16, 8, 4, 2, 1 whose bands read at most 64 source rows (else at most
    256); returns (band_rows, source rows of the widest band)."""
    hs = vbounds.shape[0]
    best = None
    for band in (16, 8, 4, 2, 1):
        y0 = np.arange(0, hs, band)
        y1 = np.minimum(y0 + band, hs) - 1
        rows = int((vbounds[y1, 0] + vbounds[y1, 1] - vbounds[y0, 0]).max())
        if rows <= 64:
            return band, rows
        if best is None and rows <= _LDS_ROWS_MAX:
            best = (band, rows)
    if best is None:
        raise ValueError("pil_resize_normalize: a downscale this large needs more than %d source rows per output row"
                         % _LDS_ROWS_MAX)
    return best


class _Tables:
    """Device coefficient tables of one (frame size, target sizes) pair."""

    def __init__(self, h, w, sizes, device):
        self.sizes = sizes
        self.scales = (_lib.ResizeScale * len(sizes))()
        self.keep = []
        for i, (hs, ws) in enumerate(sizes):
            hb, hk = resample_coeffs(w, ws)
            vb, vk = resample_coeffs(h, hs)
            band, rows = _band_rows(vb)
            dev = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (hb, hk, vb, vk)]
            self.keep += dev
            s = self.scales[i]
            s.hbounds, s.hcoef, s.vbounds, s.vcoef = (t.data_ptr() for t in dev)
            s.Hs, s.Ws, s.kh, s.kv = hs, ws, hk.shape[1], vk.shape[1]
            s.band_rows, s.lds_rows = band, rows


_CACHE: dict = {}


def _tables(h, w, sizes, device):
    key = (h, w, sizes, device)
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = _Tables(h, w, sizes, device)
    return t


def pil_resize_normalize(frame: torch.Tensor, sizes, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """frame: uint8 CUDA [h, w, 3] (RGB, HWC).  sizes: (H_s, W_s) per scale (at most 8).  Returns one fp32 [1, 3, H_s, W_s]
    tensor per scale equal to the reference's img_transform(imresize(img, (W_s, H_s), 'bilinear')), on the current
    stream."""
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.uint8):
        raise TypeError("pil_resize_normalize takes a uint8 CUDA frame (there is no CPU fallback)")
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError("pil_resize_normalize: frame must be [h, w, 3]")
    sizes = tuple((int(a), int(b)) for a, b in sizes)
    if not 1 <= len(sizes) <= _lib.RESIZE_MAX_SCALES:
        raise ValueError("pil_resize_normalize: 1 to %d target sizes" % _lib.RESIZE_MAX_SCALES)
    lib = _lib.load()
    frame = frame.contiguous()
    h, w = int(frame.shape[0]), int(frame.shape[1])
    tab = _tables(h, w, sizes, frame.device)
    # Normalize's mean / std as torch.as_tensor(..., dtype=float32) rounds them
    m = torch.as_tensor(mean, dtype=torch.float32).tolist()
    s = torch.as_tensor(std, dtype=torch.float32).tolist()
    outs = [torch.empty((1, 3, hs, ws), dtype=torch.float32, device=frame.device) for hs, ws in sizes]
    scales = (_lib.ResizeScale * len(sizes))()
    C.memmove(scales, tab.scales, C.sizeof(scales))
    for i, o in enumerate(outs):
        scales[i].out = o.data_ptr()
    st = torch.cuda.current_stream(frame.device).cuda_stream
    _lib.check(lib.dml_pil_resize_normalize(frame.data_ptr(), h, w, scales, len(sizes), m[0], m[1], m[2], s[0], s[1], s[2],
                                            st), "dml_pil_resize_normalize")
    return outs


def segm_to_label(segm: torch.Tensor) -> torch.Tensor:
    """segm_transform of the same dataset: uint8 CUDA annotation -> int64 segm - 1 (0 becomes -1)."""
    if not (isinstance(segm, torch.Tensor) and segm.is_cuda and segm.dtype == torch.uint8):
        raise TypeError("segm_to_label takes a uint8 CUDA tensor (there is no CPU fallback)")
    lib = _lib.load()
    segm = segm.contiguous()
    out = torch.empty(segm.shape, dtype=torch.int64, device=segm.device)
    _lib.check(lib.dml_segm_to_label(segm.data_ptr(), segm.numel(), out.data_ptr(), torch.cuda.current_stream(segm.device).cuda_stream),
               "dml_segm_to_label")
    return out
