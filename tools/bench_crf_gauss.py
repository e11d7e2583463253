"""Measurement tool (GPU box): the Gaussian dense-CRF confidence of one frame, utils.dense_crf_gauss against the same
algorithm composed from torch operators on the same GPU.

    timeout -k 10 900 python3 tools/bench_crf_gauss.py [--calls 5] [--torch_calls 2] [--reps 5] [--out F.json]

One process, one frame of 1 x K x H x W scores per shape: 13 x 720 x 1280 (StreetHazards) and 19 x 1024 x 2048, each with
100 (the reference's inference(100)) and 10 mean-field steps.  It times
  hip    utils.dense_crf_gauss(scores, sxy=3, compat=3, iters=n): 1 + 2 n launches of dml_crf_gauss
  torch  the definition of tests/crf_cases.py spelled with torch on the device -- per step
             t = conv2d(q * nx, kx[1, 1, 1, 37], padding=(0, 18))            (channels as the batch: one plane per image)
             m = conv2d(t * ny, ky[1, 1, 37, 1], padding=(18, 0))
             q = softmax(torch.addcmul(-u, m, compat * ny * nx), dim=0)
         two conv2d calls, two multiplies, one addcmul and one softmax per step, zero padding (= the sum over the pixels
         inside the image), the same 6 sigma cut.
Both routes run through Python as a caller gets them.  A repetition is --calls (--torch_calls) calls back to back between
two events, divided by the number of calls, after a warm-up call of each route and shape; the spread is max - min over the
repetitions.  A call iterates on its own workspace (U, Q, T: 3 x 48 MB at 13 x 720 x 1280, 3 x 159 MB at 19 x 1024 x 2048),
which is what a user's call does, so the first shape runs out of the 256 MB last-level cache and the second does not.
The traffic model per step is 5 K H W 4 bytes (Q read, T written, T read, U read, Q written); the GB/s figure is that model
over the time per step, (t_100 - t_10) / 90, which leaves the init launch out.  The two routes are compared with each other
on every pixel (both are float32; tests/test_gpu_crf_gauss.py holds the hip route to 1e-5 of the float64 definition at
sizes where that definition is affordable).  Prints one line per measurement and then one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((13, 720, 1280), (19, 1024, 2048))
STEPS = (100, 10)
SXY, COMPAT, CLIP = 3.0, 3.0, 1e-5
ROUTES_BAR = 2e-5                # each route may sit 1e-5 from the definition


def make_scores(K, Hh, Ww, g):
    """the input recipe of tests/crf_cases.py on the device: 2 * (a field replicated over 8 x 8 pixels + 0.3 * pixel noise)"""
    low = torch.randn(1, K, (Hh + 7) // 8, (Ww + 7) // 8, generator=g, device="cuda")
    up = low.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)[:, :, :Hh, :Ww]
    return (2.0 * (up + 0.3 * torch.randn(1, K, Hh, Ww, generator=g, device="cuda"))).contiguous()


def torch_route(scores, iters):
    K, Hh, Ww = scores.shape[1:]
    R = int(np.ceil(6.0 * SXY))
    d = torch.arange(-R, R + 1, device="cuda", dtype=torch.float32)
    k1 = torch.exp(-d * d / (2.0 * SXY * SXY))
    kx, ky = k1.view(1, 1, 1, -1), k1.view(1, 1, -1, 1)
    nx = F.conv2d(torch.ones(1, 1, 1, Ww, device="cuda"), kx, padding=(0, R)).rsqrt()          # [1, 1, 1, W]
    ny = F.conv2d(torch.ones(1, 1, Hh, 1, device="cuda"), ky, padding=(R, 0)).rsqrt()          # [1, 1, H, 1]
    scale = COMPAT * ny * nx
    p = torch.softmax(scores[0], dim=0).clamp(CLIP, 1.0)
    nu = torch.log(p).unsqueeze(1)                                                            # -U, [K, 1, H, W]
    q = torch.softmax(nu, dim=0)
    for _ in range(iters):
        t = F.conv2d(q * nx, kx, padding=(0, R))
        m = F.conv2d(t * ny, ky, padding=(R, 0))
        q = torch.softmax(torch.addcmul(nu, m, scale), dim=0)
    return q.amax(dim=0)                                                                      # [1, H, W]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--torch_calls", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    import utils
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    results = []
    for K, Hh, Ww in SHAPES:
        scores = make_scores(K, Hh, Ww, g)
        unit = 4 * K * Hh * Ww
        per_shape = {}
        for n in STEPS:
            hip_fn = lambda: utils.dense_crf_gauss(scores, sxy=SXY, compat=COMPAT, iters=n, clip=CLIP)  # noqa: E731
            torch_fn = lambda: torch_route(scores, n)  # noqa: E731
            ours, theirs = hip_fn(), torch_fn()                          # warm-up, and the comparison
            torch.cuda.synchronize()
            diff = float((ours - theirs).abs().max())
            h_reps = [timed(hip_fn, a.calls) for _ in range(a.reps)]
            t_reps = [timed(torch_fn, a.torch_calls) for _ in range(a.reps)]
            h_ms, t_ms = float(np.median(h_reps)), float(np.median(t_reps))
            per_shape[n] = h_ms
            res = {"K": K, "frame": [Hh, Ww], "steps": n, "calls": a.calls, "torch_calls": a.torch_calls, "reps": a.reps,
                   "hip": {"ms": round(h_ms, 3), "spread_ms": round(max(h_reps) - min(h_reps), 3), "launches": 1 + 2 * n,
                           "ms_per_step": round(h_ms / n, 4)},
                   "torch": {"ms": round(t_ms, 3), "spread_ms": round(max(t_reps) - min(t_reps), 3),
                             "ms_per_step": round(t_ms / n, 4)},
                   "torch_over_hip": round(t_ms / h_ms, 2), "unit_mbytes": round(unit / 1e6, 1),
                   "routes_max_abs_diff": diff, "routes_agree": diff <= ROUTES_BAR}
            print("K %d %dx%d steps %d: hip %.3f ms per frame (spread %.3f, %d launches, %.4f ms per step), torch %.3f ms "
                  "(spread %.3f, %.4f ms per step), torch / hip = %.2f; routes differ by at most %.2e"
                  % (K, Hh, Ww, n, h_ms, res["hip"]["spread_ms"], 1 + 2 * n, h_ms / n, t_ms, res["torch"]["spread_ms"],
                     t_ms / n, t_ms / h_ms, diff))
            results.append(res)
        step_ms = (per_shape[100] - per_shape[10]) / 90.0
        gbs = 5 * unit / (step_ms * 1e-3) / 1e9
        print("K %d %dx%d: %.4f ms per step from the two step counts; model 5 x %.1f MB per step -> %.0f GB/s"
              % (K, Hh, Ww, step_ms, unit / 1e6, gbs))
        results.append({"K": K, "frame": [Hh, Ww], "hip_ms_per_step_marginal": round(step_ms, 4),
                        "model_mbytes_per_step": round(5 * unit / 1e6, 1), "hip_gbs": round(gbs, 1)})
        del scores
        torch.cuda.empty_cache()
    line = json.dumps({"crf_gauss": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(r.get("routes_agree", True) for r in results):
        raise SystemExit("the two routes differ by more than %.0e" % ROUTES_BAR)


if __name__ == "__main__":
    main()
