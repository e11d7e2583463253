"""Measurement tool (GPU box): the scale-augmented train transform on the device.

    python3 tools/bench_aug_scale.py [--batch 16] [--height 1024 --width 2048] [--crop 768] [--rounds 30]

For every scale in --scales (default 0.5 1.0 1.5 2.0), all samples of the batch at that scale with a window in the middle of
the padded / scaled frame, it prints one line and finally one JSON line:
  stage_us        device time of dml_aug_scale_window alone (tables already on the device), events around the launch;
  transform_us    device time of the whole transform's three launches (window, contrast sum, apply), events around them;
  call_ms         wall time of ExtCompose.__call__ with forced parameters, host table build and uploads included;
  crop_only_us    the yardstick: the same batch through the crop-only transform (dml_aug_contrast_sum + dml_aug_apply
                  on the source frames), events around its two launches; ratio = transform_us / crop_only_us;
  bytes           what the new stage requests (source taps of every workgroup's horizontal pass, label gather, tables, the
                  uint8 window) against its algorithmic minimum (the source rows x columns the window needs, once, their
                  labels, the window).
Rounds are interleaved (every variant once per round); medians are reported.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def stage_bytes(tabs, band, th, tw):
    """(requested, minimum) bytes of one sample's window stage."""
    hb, hk, vb, vk, lr, lc = tabs
    y0 = np.arange(0, th, band)
    y1 = np.minimum(y0 + band, th) - 1
    band_rows = (vb[y1, 0] + vb[y1, 1] - vb[y0, 0]).astype(np.int64)
    taps = int(hb[:, 1].sum())
    tables = 4 * sum(t.size for t in tabs)
    inside = int((lr >= 0).sum()) * int((lc >= 0).sum())
    requested = int(band_rows.sum()) * taps * 3 + inside + tables + th * tw * 4
    rows = int(vb[-1, 0] + vb[-1, 1] - vb[0, 0])
    cols_used = np.zeros(int(hb[:, 0].max() + hb[:, 1].max()) + 1, bool)
    for x0, n in hb:
        cols_used[x0:x0 + n] = True
    minimum = rows * int(cols_used.sum()) * 3 + len(set(lr[lr >= 0].tolist())) * len(set(lc[lc >= 0].tolist())) + th * tw * 4
    return requested, minimum


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=2048)
    p.add_argument("--crop", type=int, default=768)
    p.add_argument("--scales", type=float, nargs="+", default=[0.5, 1.0, 1.5, 2.0])
    p.add_argument("--rounds", type=int, default=30)
    a = p.parse_args()
    from dmlnet import _lib
    from utils import ext_transforms as et
    from utils import scale_window as SW
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W, th, tw = a.batch, a.height, a.width, a.crop, a.crop
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 19, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
    ops = [(0, 1.2), (1, 0.8), (2, 1.3)]
    tail = [et.ExtColorJitter(0.5, 0.5, 0.5), et.ExtRandomHorizontalFlip(), et.ExtToTensor(), et.ExtNormalize(MEAN, STD)]
    crop_tf = et.ExtCompose([et.ExtRandomCrop((th, tw))] + tail)
    scale_tf = et.ExtCompose([et.ExtRandomScale((min(a.scales), max(a.scales))), et.ExtRandomCrop((th, tw), pad_if_needed=True)]
                             + tail)
    crop_params = [{"i": (H - th) // 2, "j": (W - tw) // 2, "ops": ops, "flip": bool(b & 1)} for b in range(B)]
    st = torch.cuda.current_stream(dev).cuda_stream

    def aug_samples(params, windowed):
        arr = (_lib.AugSample * B)()
        for b, q in enumerate(params):
            s = arr[b]
            s.i, s.j = (0, 0) if windowed else (q["i"], q["j"])
            s.flip, s.n_ops = int(q["flip"]), len(q["ops"])
            for k, (code, f) in enumerate(q["ops"]):
                s.op[k], s.factor[k] = code, f
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

    lsum = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty((B, 3, th, tw), dtype=torch.float32, device=dev)
    olb = torch.empty((B, th, tw), dtype=torch.int64, device=dev)
    wimg = torch.empty((B, th, tw, 3), dtype=torch.uint8, device=dev)
    wlbl = torch.empty((B, th, tw), dtype=torch.uint8, device=dev)

    def jitter(img, lbl, samples, h, w):
        _lib.check(lib.dml_aug_contrast_sum(img.data_ptr(), samples.data_ptr(), lsum.data_ptr(), B, h, w, th, tw, st), "sum")
        _lib.check(lib.dml_aug_apply(img.data_ptr(), lbl.data_ptr(), samples.data_ptr(), lsum.data_ptr(), out.data_ptr(),
                                     olb.data_ptr(), B, h, w, th, tw, MEAN[0], MEAN[1], MEAN[2], STD[0], STD[1], STD[2], st),
                   "apply")

    crop_samples = aug_samples(crop_params, False)
    variants = {}
    for sc in a.scales:
        Hs, Ws = int(H * sc), int(W * sc)
        oy, ox = (Hs - th) // 2, (Ws - tw) // 2               # negative when the scaled frame is smaller: padding
        params = [{"i": 0, "j": 0, "ops": ops, "flip": bool(b & 1), "size": (Hs, Ws), "oy": oy, "ox": ox, "out": (th, tw)}
                  for b in range(B)]
        buf, band, rows = SW.pack([(Hs, Ws, oy, ox)] * B, H, W, th, tw)
        req, mn = stage_bytes(SW.window_tables(H, W, Hs, Ws, oy, ox, th, tw), band, th, tw)
        variants[sc] = {"params": params, "buf": torch.from_numpy(buf).to(dev), "n": int(buf.size), "band": band, "rows": rows,
                        "samples": aug_samples(params, True), "requested": req * B, "minimum": mn * B,
                        "stage": [], "transform": [], "call": []}

    def stage(v):
        _lib.check(lib.dml_aug_scale_window(frames.data_ptr(), labels.data_ptr(), v["buf"].data_ptr(), v["buf"].data_ptr(), v["n"],
                                            wimg.data_ptr(), wlbl.data_ptr(), B, H, W, th, tw, v["band"], v["rows"], st), "window")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    def whole(v):
        stage(v)
        jitter(wimg, wlbl, v["samples"], th, tw)

    crop_us = []
    for r in range(a.rounds + 3):
        keep = r >= 3                                          # three warm-up rounds
        t = timed(lambda: jitter(frames, labels, crop_samples, H, W))
        if keep:
            crop_us.append(t)
        for v in variants.values():
            t0, t1 = timed(lambda: stage(v)), timed(lambda: whole(v))
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            scale_tf(frames, labels, params=v["params"])
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            if keep:
                v["stage"].append(t0)
                v["transform"].append(t1)
                v["call"].append(1e3 * (w1 - w0))
    crop_only = float(np.median(crop_us))
    res = {"batch": B, "frame": [H, W], "crop": [th, tw], "rounds": a.rounds, "crop_only_us": round(crop_only, 1), "scales": {}}
    print("crop-only transform (yardstick): %.1f us" % crop_only)
    for sc, v in variants.items():
        s_us, t_us, c_ms = (float(np.median(v[k])) for k in ("stage", "transform", "call"))
        res["scales"]["%g" % sc] = {"stage_us": round(s_us, 1), "transform_us": round(t_us, 1), "call_ms": round(c_ms, 2),
                                    "ratio_to_crop_only": round(t_us / crop_only, 2), "band_rows": v["band"],
                                    "lds_rows": v["rows"], "requested_MB": round(v["requested"] / 1e6, 1),
                                    "minimum_MB": round(v["minimum"] / 1e6, 1),
                                    "stage_GBps_of_minimum": round(v["minimum"] / s_us / 1e3, 1)}
        print("scale %g: stage %.1f us, transform %.1f us (%.2fx crop-only), call %.2f ms, bytes %.1f MB requested / %.1f MB minimum"
              % (sc, s_us, t_us, t_us / crop_only, c_ms, v["requested"] / 1e6, v["minimum"] / 1e6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
