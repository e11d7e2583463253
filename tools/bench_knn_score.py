"""Measurement tool (GPU box): the kNN cosine-similarity anomaly score of one StreetHazards frame, kernel against torch.

    timeout -k 10 300 python3 tools/bench_knn_score.py [--height 720 --width 1280] [--iters 20] [--reps 5] [--out F.json]

One process, one frame of 1 x 13 x H x W features (the `ft1` of the open-set driver).  It times
  kernel  dml_knn_cosine_score through the C ABI on a preallocated output (what utils.knn_cosine_score launches; the
          wrapper's allocation would put the host on the clock)
  torch   the `--ood knn` branch of the reference (anomaly/eval_ood_traditional.py:512-525) executed with torch on the
          device: for every shift (i, j) in 1..8 x 1..8 a zero tensor that receives the features moved up-left by (i, j)
          and one that receives them moved down-right, and F.cosine_similarity of each with the features over the
          channel axis, added into the map
A kernel repetition is --iters calls back to back between two events, divided by --iters, after a warm-up; the calls
rotate through six input sets (288 MB at the default size) so that none finds its input in the 256 MB last-level cache.
The torch route is timed per call (--torch-reps calls after one warm-up call).  The spread is max - min over the
repetitions.  The HBM bound is B H W (C + 1) 4 bytes -- the features read once, the map written once -- at 8 TB/s.
Prints one line per route, the ratio, the kernel's share of the bound, the largest difference between the two maps,
and then one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOF_GBS = 8000.0
NEIGHBOR_SIZE = 9


def torch_route(ft1, neighbor_size=NEIGHBOR_SIZE):
    """the reference's branch on one image ft1 [C, H, W], on ft1's device"""
    c, h, w = ft1.shape
    total = torch.zeros((h, w), dtype=ft1.dtype, device=ft1.device)
    for i in range(1, neighbor_size):
        for j in range(1, neighbor_size):
            moved = torch.zeros_like(ft1)
            moved[:, :h - i, :w - j] = ft1[:, i:, j:]
            total += torch.nn.functional.cosine_similarity(ft1, moved, dim=0)
            moved = torch.zeros_like(ft1)
            moved[:, i:, j:] = ft1[:, :h - i, :w - j]
            total += torch.nn.functional.cosine_similarity(ft1, moved, dim=0)
    return total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--height", type=int, default=720)
    p.add_argument("--width", type=int, default=1280)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--torch-reps", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from dmlnet import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    Hh, Ww, C = a.height, a.width, 13
    g = torch.Generator(device="cuda").manual_seed(7)
    sets = [2.5 * torch.randn(1, C, Hh, Ww, generator=g, device="cuda") for _ in range(6)]
    score = torch.empty((1, Hh, Ww), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def kernel(s):
        _lib.check(lib.dml_knn_cosine_score(sets[s].data_ptr(), score.data_ptr(), 1, C, Hh, Ww, NEIGHBOR_SIZE, st),
                   "dml_knn_cosine_score")

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(n):
            fn(it % len(sets))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for it in range(6):
        kernel(it)
    torch.cuda.synchronize()
    k_reps = [timed(kernel, a.iters) for _ in range(a.reps)]
    kernel(0)
    ours = score[0].clone()
    theirs = torch_route(sets[0][0])                                  # the warm-up call of the torch route
    torch.cuda.synchronize()
    diff = float((ours - theirs).abs().max())
    t_reps = [timed(lambda s: torch_route(sets[s][0]), 1) for _ in range(a.torch_reps)]

    nbytes = Hh * Ww * (C + 1) * 4
    bound_ms = nbytes / (ROOF_GBS * 1e9) * 1e3
    k_ms, t_ms = float(np.median(k_reps)), float(np.median(t_reps))
    res = {"frame": [Hh, Ww], "C": C, "neighbor_size": NEIGHBOR_SIZE, "iters": a.iters, "reps": a.reps,
           "kernel": {"ms_reps": [round(v, 4) for v in k_reps], "ms": round(k_ms, 4),
                      "spread_ms": round(max(k_reps) - min(k_reps), 4)},
           "torch": {"ms_reps": [round(v, 3) for v in t_reps], "ms": round(t_ms, 3),
                     "spread_ms": round(max(t_reps) - min(t_reps), 3)},
           "torch_over_kernel": round(t_ms / k_ms, 1), "mbytes": round(nbytes / 1e6, 1), "roof_gbs": ROOF_GBS,
           "hbm_bound_ms": round(bound_ms, 5), "kernel_share_of_bound": round(bound_ms / k_ms, 3),
           "max_abs_diff": diff}
    print("kernel %.4f ms (spread %.4f over %d reps of %d calls)" % (k_ms, res["kernel"]["spread_ms"], a.reps, a.iters))
    print("torch  %.3f ms (spread %.3f over %d calls)" % (t_ms, res["torch"]["spread_ms"], a.torch_reps))
    print("torch / kernel = %.1f; HBM bound %.1f MB at %g TB/s = %.4f ms: the kernel runs at %.1f %% of it; largest |kernel - torch| = %.3e"
          % (t_ms / k_ms, nbytes / 1e6, ROOF_GBS / 1e3, bound_ms, 100 * bound_ms / k_ms, diff))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
