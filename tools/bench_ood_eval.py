"""Measurement tool (GPU box): the open-set evaluation of eval_ood_traditional.py on a StreetHazards-layout tree.

    python3 tools/bench_ood_eval.py [--root DIR --list FILE.odgt] [--frames 16] [--workers N] [--dtype bf16|f32|f16x2|f32x3]

Without --root it writes a StreetHazards-shaped tree of its own (720 x 1280 RGB PNGs, 'L' annotations) to a temporary
directory.  Prints, one per line and then as one JSON line:
  decode_ms_per_frame_per_worker  Image.open(...).convert('RGB') + Image.open(segm), one thread, every frame once;
  resize_us_per_frame             device time of one dml_pil_resize_normalize launch (all five scales), events around it;
  model_ms_per_frame              evaluate()'s model-only time per frame (the reference's "Inference Time");
  wall_fps / model_fps            end-to-end frames/s of reader + evaluate at the requested workers, and 1 / model time.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_tree(root, n, h=720, w=1280, seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy // 3 + xx // 5) % 256, (xx // 2) % 256, (yy // 2) % 256], -1)
    recs = []
    for i in range(n):
        img = np.clip(base + rs.randint(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)
        segm = rs.randint(1, 15, ((h + 31) // 32, (w + 31) // 32)).repeat(32, 0).repeat(32, 1)[:h, :w].astype(np.uint8)
        fi, fs = "images/%d.png" % i, "annotations/%d.png" % i
        Image.fromarray(img).save(os.path.join(root, fi))
        Image.fromarray(segm, mode="L").save(os.path.join(root, fs))
        recs.append({"fpath_img": fi, "fpath_segm": fs, "height": h, "width": w})
    odgt = os.path.join(root, "test.odgt")
    with open(odgt, "w") as f:
        f.write(json.dumps(recs) + "\n")
    return odgt


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default="")
    p.add_argument("--list", default="")
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--workers", type=int, default=0)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"])
    p.add_argument("--ood", default="dissum")
    a = p.parse_args()
    from PIL import Image
    import eval_ood_traditional as E
    import models
    import utils
    from datasets.streethazards import StreetHazardsReader, default_workers, parse_odgt, resized_shapes

    tmp = None
    if not a.root:
        tmp = tempfile.TemporaryDirectory()
        a.root, a.list = tmp.name, make_tree(tmp.name, a.frames)
    recs = parse_odgt(a.list, max_sample=a.frames)
    workers = a.workers or default_workers()

    dec = []
    for r in recs:
        t0 = time.perf_counter()
        segm = Image.open(os.path.join(a.root, r["fpath_segm"]))
        img = Image.open(os.path.join(a.root, r["fpath_img"])).convert("RGB")
        np.asarray(segm), np.asarray(img)
        dec.append(time.perf_counter() - t0)
    decode_ms = 1e3 * float(np.mean(dec))

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    frame = torch.from_numpy(np.array(img)).to(device)
    shapes = resized_shapes(*frame.shape[:2])
    for _ in range(3):
        utils.pil_resize_normalize(frame, shapes)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(50):
        e0.record()
        utils.pil_resize_normalize(frame, shapes)
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    resize_us = float(np.median(us))

    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048)
    decd = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, decd, None).to(device).eval()
    seg.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32,
                          fp32_products={"f32": "exact", "f32x3": "bf16x3", "f16x2": "f16x2"}.get(a.dtype))
    warm = StreetHazardsReader(a.root, recs[:2], workers=workers, device=device)
    E.evaluate(seg, warm, 14, a.ood, (13,))                 # plans, allocator, tables
    reader = StreetHazardsReader(a.root, recs, workers=workers, device=device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = E.evaluate(seg, reader, 14, a.ood, (13,))
    wall = time.perf_counter() - t0
    out = {"frames": len(recs), "frame": list(frame.shape[:2]), "scales": shapes, "workers": workers, "dtype": a.dtype,
           "decode_ms_per_frame_per_worker": round(decode_ms, 2), "resize_us_per_frame": round(resize_us, 1),
           "model_ms_per_frame": round(1e3 * r["sec_per_frame"], 2), "model_fps": round(1.0 / r["sec_per_frame"], 2),
           "wall_fps": round(len(recs) / wall, 2)}
    print("decode: %.2f ms/frame per worker" % out["decode_ms_per_frame_per_worker"])
    print("resize kernel: %.1f us/frame (%d scales)" % (resize_us, len(shapes)))
    print("model only: %.2f ms/frame (%.2f frames/s)" % (out["model_ms_per_frame"], out["model_fps"]))
    print("end to end: %.2f frames/s with %d workers, %s" % (out["wall_fps"], workers, a.dtype))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
