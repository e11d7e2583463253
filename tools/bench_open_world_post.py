"""Measurement tool (GPU box): the open-world post-processing of one 1024 x 2048 frame, fused against the three calls.

    timeout -k 10 300 python3 tools/bench_open_world_post.py [--height 1024 --width 2048] [--iters 20] [--reps 5] [--out F.json]

One process, one frame of 1 x 16 x H x W logits plus H x W x 16 features.  For N in 0 / 1 / 3 prototypes it times
  fused   dml_open_world_post (one pass + the normalisation of the score map)
  three   dml_argmax_msp + dml_dissum_score + dml_novel_relabel (N = 1; the relabel is left out for N = 0, and has no
          counterpart for N = 3)
through the C ABI on preallocated outputs (what utils.open_world_post / argmax_msp / dissum_score / novel_relabel
launch; the wrappers' allocations would put the host, not the GPU, on the clock at these sizes).  A repetition is
--iters calls back to back between two hipEvents, divided by --iters, after a warm-up; fused and three alternate per
repetition so that they see the same clocks, and the calls rotate between two input sets (536 MB) so that none finds
its inputs in the 256 MB last-level cache.  The spread is max - min over the --reps repetitions.  GB/s is the bytes a call has to move
(inputs once, outputs once, the score map read and written once more by the normalisation) over its time, next to the
8 TB/s HBM roof.  Prints one line per case and then one JSON line.
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=2048)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from dmlnet import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    Hh, Ww, C, K = a.height, a.width, 16, 16
    px = Hh * Ww
    g = torch.Generator(device="cuda").manual_seed(7)
    protos_all = torch.randn(3, C, generator=g, device="cuda")
    sets = []
    for _ in range(2):
        feats = protos_all[0] + 0.4 * torch.randn(1, Hh, Ww, C, generator=g, device="cuda")
        lg = -2.0 * torch.randn(1, K, Hh, Ww, generator=g, device="cuda").abs() - 0.3
        sets.append((lg, feats))
    labels = torch.arange(K, K + 3, dtype=torch.int64, device="cuda")
    preds = torch.empty((1, Hh, Ww), dtype=torch.int64, device="cuda")
    msp = torch.empty((1, Hh, Ww), dtype=torch.float32, device="cuda")
    score = torch.empty((1, Hh, Ww), dtype=torch.float32, device="cuda")
    work = torch.empty(2, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fused(N, s):
        lg, feats = sets[s]
        _lib.check(lib.dml_open_world_post(lg.data_ptr(), feats.data_ptr() if N else None, protos_all.data_ptr() if N else None,
                                           labels.data_ptr() if N else None, preds.data_ptr(), msp.data_ptr(),
                                           score.data_ptr(), work.data_ptr(), 1, C, K, Hh, Ww, N, -1.5, 1, 1000.0, 0, st),
                   "dml_open_world_post")

    def three(N, s):
        lg, feats = sets[s]
        _lib.check(lib.dml_argmax_msp(lg.data_ptr(), preds.data_ptr(), msp.data_ptr(), 1, K, Hh, Ww, st), "dml_argmax_msp")
        _lib.check(lib.dml_dissum_score(lg.data_ptr(), score.data_ptr(), work.data_ptr(), 1, K, Hh, Ww, 1000.0, 0, st),
                   "dml_dissum_score")
        if N:
            _lib.check(lib.dml_novel_relabel(feats.data_ptr(), lg.data_ptr(), protos_all.data_ptr(), preds.data_ptr(), 1, C,
                                             K, Hh, Ww, -1.5, K, st), "dml_novel_relabel")

    # bytes: logits (+ features) read, preds int64 + msp + score written, score read and written by the normalisation
    out_bytes = px * (8 + 4 + 4 + 8)
    fused_bytes = {N: px * K * 4 + (px * C * 4 if N else 0) + out_bytes for N in (0, 1, 3)}
    three_bytes = {0: 2 * px * K * 4 + out_bytes, 1: 3 * px * K * 4 + px * C * 4 + out_bytes + px * 8}

    def time_calls(fn, N):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            fn(N, it & 1)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    res = {"frame": [Hh, Ww], "C": C, "K": K, "iters": a.iters, "reps": a.reps, "roof_gbs": ROOF_GBS, "cases": {}}
    for N in (0, 1, 3):
        calls = [("fused", fused, fused_bytes[N])] + ([("three", three, three_bytes[N])] if N in three_bytes else [])
        for it in range(6):
            for _, fn, _ in calls:
                fn(N, it & 1)
        torch.cuda.synchronize()
        reps = {name: [] for name, _, _ in calls}
        for _ in range(a.reps):
            for name, fn, _ in calls:
                reps[name].append(time_calls(fn, N))
        case = {}
        for name, _, nbytes in calls:
            med = float(np.median(reps[name]))
            case[name] = {"ms_reps": [round(v, 4) for v in reps[name]], "ms": round(med, 4),
                          "spread_ms": round(max(reps[name]) - min(reps[name]), 4), "mbytes": round(nbytes / 1e6, 1),
                          "gbs": round(nbytes / med / 1e6, 1), "of_roof": round(nbytes / med / 1e6 / ROOF_GBS, 3)}
            print("N=%d %-5s %.4f ms (spread %.4f over %d reps)  %.1f MB  %.0f GB/s = %.0f %% of the %g TB/s roof"
                  % (N, name, med, case[name]["spread_ms"], a.reps, nbytes / 1e6, case[name]["gbs"],
                     100 * case[name]["of_roof"], ROOF_GBS / 1e3))
        if "three" in case:
            case["three_over_fused"] = round(case["three"]["ms"] / case["fused"]["ms"], 3)
        res["cases"]["N=%d" % N] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
