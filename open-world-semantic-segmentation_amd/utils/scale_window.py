"""Host side of dml_aug_scale_window (csrc/aug_scale.hip): the scale / resize / pad / crop stages of the reference's
transforms reduced, per sample, to a VIRTUAL image (the frame resized to (Hs, Ws)) and a th x tw window of it whose origin
may be negative and whose extent may pass the far edge; outside the virtual image a pixel is 0.

Image tables are Pillow's BILINEAR coefficients (utils/image_resize.resample_coeffs) restricted to the window's rows and
columns; label tables are Pillow's NEAREST source indices (Geometry.c, ImagingScaleAffine), which accumulate in double
(xo = 0.5 * in / out; idx = int(xo); xo += in / out) and therefore differ from every closed form.  Full-axis tables are
cached by (H, W, Hs, Ws); the windows of a batch are concatenated into one int32 buffer so that one upload and one launch
serve all samples.  Everything the kernel will use as a source index is validated here, against the frame.
"""
from __future__ import annotations

import numpy as np

from .image_resize import PRECISION_BITS, resample_coeffs

_LDS_ROWS_MAX = 256          # source rows one workgroup can hold (csrc/aug_scale.hip)
_CACHE_MAX = 512
_CACHE: dict = {}


def nearest_index(in_size: int, out_size: int):
    """Source index of every output pixel of Pillow's NEAREST resize along one axis, int32 [out]."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError("nearest_index: sizes must be positive")
    step = float(in_size) / out_size
    xo = np.full(out_size, step, dtype=np.float64)
    xo[0] = 0.5 * step
    idx = np.add.accumulate(xo).astype(np.int64)            # a sequential sum, as the C loop's xo += step
    if idx[0] < 0 or idx[-1] >= in_size:
        raise ValueError("nearest_index: index outside the source (in %d, out %d)" % (in_size, out_size))
    return idx.astype(np.int32)


def _axis(in_size, out_size):
    """(bounds [out][2], coef [out][k], nearest [out]) of one axis; the identity when the size does not change (Pillow skips
    that pass: one tap of weight 1.0 passes the arithmetic through unchanged)."""
    if in_size == out_size:
        ar = np.arange(out_size, dtype=np.int32)
        return (np.stack([ar, np.ones_like(ar)], axis=1), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32), ar)
    b, k = resample_coeffs(in_size, out_size)
    return b, k, nearest_index(in_size, out_size)


def full_tables(H, W, Hs, Ws):
    """((hbounds, hcoef, lcol), (vbounds, vcoef, lrow)) of the whole virtual image, cached."""
    key = (H, W, Hs, Ws)
    t = _CACHE.get(key)
    if t is None:
        if len(_CACHE) >= _CACHE_MAX:
            _CACHE.clear()
        t = _CACHE[key] = (_axis(W, Ws), _axis(H, Hs))
    return t


def _window_axis(axis, origin, extent):
    """Rows `origin .. origin + extent - 1` of one axis' tables.  Outside the virtual image: tap count 0, label index -1, and
    a first source index that keeps the sequence monotone (before: the first inside entry's, after: the last one's end)."""
    bounds, coef, near = axis
    size = bounds.shape[0]
    v = np.arange(origin, origin + extent)
    inside = (v >= 0) & (v < size)
    vc = np.clip(v, 0, size - 1)
    wb = bounds[vc].copy()
    wk = coef[vc].copy()
    wn = near[vc].copy()
    wb[~inside, 1] = 0
    wk[~inside] = 0
    wn[~inside] = -1
    if inside.any():
        after = v >= size
        wb[after, 0] = bounds[-1, 0] + bounds[-1, 1]
    else:
        wb[:, 0] = 0
    return wb, wk, wn


def window_tables(H, W, Hs, Ws, oy, ox, th, tw):
    """The six tables of one sample's window: hbounds [tw][2], hcoef [tw][kh], vbounds [th][2], vcoef [th][kv], lrow [th],
    lcol [tw] (all int32)."""
    if min(H, W, Hs, Ws, th, tw) <= 0:
        raise ValueError("window_tables: sizes must be positive")
    hax, vax = full_tables(H, W, Hs, Ws)
    hb, hk, lc = _window_axis(hax, ox, tw)
    vb, vk, lr = _window_axis(vax, oy, th)
    return hb, hk, vb, vk, lr, lc


def validate(tabs, H, W):
    """Every index the kernel reads through lies inside the frame, every tap count within its table's width."""
    hb, hk, vb, vk, lr, lc = tabs
    for b, k, size, what in ((hb, hk, W, "column"), (vb, vk, H, "row")):
        if (b[:, 1] < 0).any() or (b[:, 1] > k.shape[1]).any():
            raise ValueError("scale window: %s tap count outside the table width" % what)
        if (b[:, 0] < 0).any() or (b[:, 0] + b[:, 1] > size).any():
            raise ValueError("scale window: %s taps outside the frame" % what)
    if (np.diff(vb[:, 0]) < 0).any() or (np.diff(vb[:, 0] + vb[:, 1]) < 0).any():
        raise ValueError("scale window: row bounds are not monotone")
    for n, size, what in ((lr, H, "row"), (lc, W, "column")):
        if (n < -1).any() or (n >= size).any():
            raise ValueError("scale window: label %s index outside the frame" % what)


def band_rows(vbounds_list):
    """Window rows per workgroup for a batch: the largest of 16, 8, 4, 2, 1 whose bands read at most 64 source rows in every
    sample (else at most 256); returns (band_rows, source rows of the widest band).  At scale 0.5 (at most five vertical taps
    per row) 16 rows read at most 35."""
    best = None
    for band in (16, 8, 4, 2, 1):
        rows = 0
        for vb in vbounds_list:
            th = vb.shape[0]
            y0 = np.arange(0, th, band)
            y1 = np.minimum(y0 + band, th) - 1
            rows = max(rows, int((vb[y1, 0] + vb[y1, 1] - vb[y0, 0]).max()))
        if rows <= 64:
            return band, max(rows, 1)
        if best is None and rows <= _LDS_ROWS_MAX:
            best = (band, rows)
    if best is None:
        raise ValueError("scale window: a downscale this large needs more than %d source rows per output row" % _LDS_ROWS_MAX)
    return best


def pack(windows, H, W, th, tw):
    """windows: per sample (Hs, Ws, oy, ox).  Returns (buffer int32 [B * 8 + ...], band_rows, lds_rows): the B DmlScaleWindow
    records (eight int32 each, element offsets into this same buffer) followed by every sample's validated tables."""
    B = len(windows)
    head = np.zeros((B, 8), np.int32)
    parts, off, vbs = [head.reshape(-1)], B * 8, []
    for b, (Hs, Ws, oy, ox) in enumerate(windows):
        tabs = window_tables(H, W, Hs, Ws, oy, ox, th, tw)
        validate(tabs, H, W)
        vbs.append(tabs[2])
        for f, t in enumerate(tabs):
            head[b, f] = off
            t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1)
            parts.append(t)
            off += t.size
        head[b, 6], head[b, 7] = tabs[1].shape[1], tabs[3].shape[1]
    if off >= 2 ** 31:
        raise ValueError("scale window: tables too large")
    band, rows = band_rows(vbs)
    parts[0] = head.reshape(-1)
    return np.concatenate(parts), band, rows
