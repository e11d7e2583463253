"""Measurement tool (one MI355X): the per-class ECDF certainty score of one frame, its two streaming kernels against the same
definition composed from torch operators and against the "EDS + MMSP" score.

    timeout -k 10 600 python3 tools/bench_ecdf_score.py [--iters 20] [--reps 5] [--out profiles/ecdf_score_bench.json]

One process, one MI355X.  Frames of 13 x 720 x 1280 (2048 bins, clip 400) and 19 x 1024 x 2048 (1024 bins, clip 1000): negative
squared distances of random features to the prototypes 3 e_k, labels that equal the prediction on 60 % of the pixels.  Two kinds of
features:
  iid      independent per pixel, mean distance sum 0.85 clip: every lane of a wave looks up another table row, the worst case
  smooth   drawn at 1/8 of the resolution and resized bilinearly, as a segmentation head's logits are: neighbouring pixels fall into
           the same or neighbouring bins
It times
  collect          dml_ecdf_collect through the C ABI into a preallocated histogram (what EcdfCalibrator.update launches)
  collect_torch    the same definition from torch operators: sum, argmax, the bin by multiply / int / clamp / where, one bincount
                   of class * NB + bin over the matching pixels, added to the histogram
  score            dml_ecdf_score through the C ABI against the calibrator's hard table
  score_torch      softmax, sum, the same bin, a gather of the table's rows, multiply and sum
  dissum_msp       dml_dissum_msp_score on the same logits (the neighbour the score should keep up with)
A repetition is --iters calls back to back between two events, divided by --iters, after a warm-up; the calls rotate through enough
copies of the inputs (more than 320 MB) that none finds its input in the 256 MB last-level cache.  Reported per row: the median over
--reps repetitions, the spread (max - min) and bytes / time for the traffic models
  collect   (4 K + 8) bytes per pixel: K logits and one int64 label           score      (4 K + 4): K logits, one float out
  dissum_msp (4 K + 24): K logits, the two maps written and read, one float out (as DESIGN.md 7f counts it)
Before timing, the composed routes are compared with the kernels.  torch sums the classes in another order, so a few sums fall into
the neighbouring bin: at most 1e-3 of the counted pixels may sit in another cell and at most 1e-3 of the scores may differ by more
than 1e-4 (the hard table jumps from the cut to 1), and the median difference must be below 1e-5.  Prints one line per row and then
one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CACHE_BYTES = 320 << 20


def make_frame(kind, K, Hh, Ww, clip, g):
    sigma = float(np.sqrt((0.85 * clip - 9.0 * K) / K ** 2))
    if kind == "smooth":                                               # bilinear weights shrink the deviation to about 2/3
        small = 1.5 * sigma * torch.randn(1, K, (Hh + 7) // 8, (Ww + 7) // 8, generator=g, device="cuda")
        f = torch.nn.functional.interpolate(small, size=(Hh, Ww), mode="bilinear", align_corners=False)
    else:
        f = sigma * torch.randn(1, K, Hh, Ww, generator=g, device="cuda")
    lg = -((f * f).sum(dim=1, keepdim=True) - 6.0 * f + 9.0)
    pred = lg.argmax(dim=1)
    other = torch.randint(0, K, pred.shape, generator=g, device="cuda")
    lab = torch.where(torch.rand(pred.shape, generator=g, device="cuda") < 0.6, pred, other)
    return lg.contiguous(), lab.contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    import utils
    from dmlnet import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(7)

    def timed(fn, n_sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            fn(it % n_sets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    rows = []
    for (kind, K, Hh, Ww, NB, clip) in (("iid", 13, 720, 1280, 2048, 400.0), ("smooth", 13, 720, 1280, 2048, 400.0),
                                        ("iid", 19, 1024, 2048, 1024, 1000.0), ("smooth", 19, 1024, 2048, 1024, 1000.0)):
        n = Hh * Ww
        n_sets = CACHE_BYTES // (4 * K * n) + 2
        sets = [make_frame(kind, K, Hh, Ww, clip, g) for _ in range(n_sets)]
        cal = utils.EcdfCalibrator(K, clip, nbins=NB)
        for lg, lab in sets:
            cal.update(lg, lab)
        table = cal.table("hard")
        Kp = table.shape[1]
        inv_w = float(np.float32(NB) / np.float32(clip))
        hist = torch.zeros((K, NB), dtype=torch.int64, device="cuda")
        hist_t = torch.zeros((K, NB), dtype=torch.int64, device="cuda")
        conf = torch.empty((1, Hh, Ww), dtype=torch.float32, device="cuda")
        work = torch.empty(4 + 2 * n, dtype=torch.float32, device="cuda")

        def bins_of(lg):
            s = -lg.sum(dim=1)
            b = (s * inv_w).to(torch.int64).clamp_(max=NB - 1)
            b = torch.where(s >= clip, torch.full_like(b, NB - 1), b)
            return torch.where(s <= 0, torch.zeros_like(b), b)

        def collect(s):
            lg, lab = sets[s]
            _lib.check(lib.dml_ecdf_collect(lg.data_ptr(), lab.data_ptr(), hist.data_ptr(), 1, K, Hh, Ww, 0, clip, NB, st),
                       "dml_ecdf_collect")

        def collect_torch(s):
            lg, lab = sets[s]
            ok = lab == lg.argmax(dim=1)
            idx = (lab * NB + bins_of(lg))[ok]
            hist_t.view(-1).add_(torch.bincount(idx, minlength=K * NB))

        def score(s):
            _lib.check(lib.dml_ecdf_score(sets[s][0].data_ptr(), table.data_ptr(), conf.data_ptr(), 1, K, Hh, Ww, 0, Kp, clip, NB,
                                          st), "dml_ecdf_score")

        def score_torch(s):
            lg = sets[s][0]
            rows_ = table[bins_of(lg)][..., :K]                         # [1, H, W, K]
            return (torch.softmax(lg, dim=1) * rows_.permute(0, 3, 1, 2)).sum(dim=1)

        def dissum_msp(s):
            _lib.check(lib.dml_dissum_msp_score(sets[s][0].data_ptr(), conf.data_ptr(), work.data_ptr(), 1, K, Hh, Ww, 0, clip, 0.2,
                                                50.0, 0, st), "dml_dissum_msp_score")

        collect(0)
        collect_torch(0)
        score(0)
        ref = score_torch(0)
        torch.cuda.synchronize()
        tot, tot_t = int(hist.sum()), int(hist_t.sum())
        moved = int((hist - hist_t).abs().sum()) // 2
        off = int(((conf - ref).abs() > 1e-4).sum())                   # pixels whose sum torch puts into the neighbouring bin
        diff = float((conf - ref).abs().median())
        if abs(tot - tot_t) > 1e-3 * tot or moved > 1e-3 * tot or off > 1e-3 * n or not diff < 1e-5:
            raise SystemExit("%s K=%d: the composed routes differ: %d / %d counted, %d moved, %d scores off, median %g"
                             % (kind, K, tot, tot_t, moved, off, diff))
        del ref
        res = {}
        for name, fn in (("collect", collect), ("collect_torch", collect_torch), ("score", score), ("score_torch", score_torch),
                         ("dissum_msp", dissum_msp)):
            for s in range(n_sets):
                fn(s)
            torch.cuda.synchronize()
            reps = [timed(fn, n_sets) for _ in range(a.reps)]
            res[name] = {"ms": round(float(np.median(reps)), 5), "spread_ms": round(max(reps) - min(reps), 5)}
        res["collect"]["gbs"] = round((4 * K + 8) * n / res["collect"]["ms"] / 1e6, 1)
        res["score"]["gbs"] = round((4 * K + 4) * n / res["score"]["ms"] / 1e6, 1)
        res["dissum_msp"]["gbs"] = round((4 * K + 24) * n / res["dissum_msp"]["ms"] / 1e6, 1)
        row = {"input": kind, "frame": [K, Hh, Ww], "bins": NB, "clip": clip, "counted": tot, "moved_by_torch_order": moved,
               "scores_off_by_torch_order": off, "score_median_diff_vs_torch": diff, **res,
               "collect_torch_over_collect": round(res["collect_torch"]["ms"] / res["collect"]["ms"], 2),
               "score_torch_over_score": round(res["score_torch"]["ms"] / res["score"]["ms"], 2),
               "score_over_dissum_msp": round(res["score"]["ms"] / res["dissum_msp"]["ms"], 3)}
        rows.append(row)
        print("%-6s %2d x %4d x %4d, %4d bins:  collect %.4f ms (+-%.4f, %6.1f GB/s)  torch %.4f ms (x%.1f) |  score %.4f ms (+-%.4f, "
              "%6.1f GB/s)  torch %.4f ms (x%.1f)  dissum_msp %.4f ms (+-%.4f, %6.1f GB/s)  score / dissum_msp %.3f"
              % (kind, K, Hh, Ww, NB, res["collect"]["ms"], res["collect"]["spread_ms"], res["collect"]["gbs"], res["collect_torch"]["ms"],
                 row["collect_torch_over_collect"], res["score"]["ms"], res["score"]["spread_ms"], res["score"]["gbs"],
                 res["score_torch"]["ms"], row["score_torch_over_score"], res["dissum_msp"]["ms"], res["dissum_msp"]["spread_ms"],
                 res["dissum_msp"]["gbs"], row["score_over_dissum_msp"]), flush=True)
        del sets
    line = json.dumps({"iters": a.iters, "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
