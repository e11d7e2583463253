"""Measurement tool (GPU box): the pooled OOD histogram of one frame against two yardsticks that are not the code under test.

    timeout -k 10 600 python3 tools/bench_pooled_ood.py [--iters 20] [--reps 5] [--out F.json]

One process.  Frames of 720 x 1280 and of 1024 x 2048, NB = 256, 4096 and 8192 bins of [0, 1], two kinds of input:
  spread        confidences uniform over the range, 7 % of the pixels anomalous
  contended     90 % of the pixels in a single bin (what the hard ECDF certainty produces: most pixels score exactly 1), the rest
                spread: the case in which same-address LDS atomics serialise
It times
  update        dml_pooled_ood_update through the C ABI onto a preallocated state (what PooledOodMeasures.update launches),
                without a mask (12 bytes per pixel) and with one (13)
  torch         the same definition from torch operators on the same GPU: the bin as clamp / multiply / truncate, the row from
                torch.isin, one torch.bincount over row * NB + bin added onto the state; its state is first checked against the
                call's wherever float32 rounding of the bin agrees (the torch route is allowed to differ on edge pixels: counted)
  sweep         dml_open_set_sweep on the same frame with T = 9 and 14 classes: the neighbouring streaming counter, which reads 20
                bytes per pixel
  finalize      dml_pooled_ood_finalize on the accumulated state
A repetition is --iters calls back to back between two events, divided by --iters, after a warm-up; the calls rotate through enough
copies of the inputs (more than 320 MB) that none finds its input in the 256 MB last-level cache.  Reported per row: the median over
--reps repetitions, the spread (max - min), bytes / time for the traffic model, and the ratios torch / update, update / sweep and
contended / spread.  Prints one line per row and then one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CACHE_BYTES = 320 << 20
OUT_LABEL, N_CLASSES = 13, 14


def make_inputs(kind, n, g):
    label = torch.randint(0, N_CLASSES, (n,), generator=g, device="cuda")           # 1 in 14 is the anomaly id: 7 %
    pred = torch.randint(0, N_CLASSES, (n,), generator=g, device="cuda")
    conf = torch.rand(n, generator=g, device="cuda")
    if kind == "contended":
        hot = torch.rand(n, generator=g, device="cuda") < 0.9
        conf[hot] = 1.0
        label[hot] = 1
    mask = (torch.rand(n, generator=g, device="cuda") < 0.9).to(torch.uint8)
    return conf, label, mask, pred


def torch_update(conf, label, out_t, NB, state):
    """the definition from torch operators (no mask, range [0, 1]); NaN is not handled: the inputs have none"""
    b = (conf.clamp(0.0, 1.0) * float(NB)).to(torch.int64).clamp_(max=NB - 1)
    row = (~torch.isin(label, out_t)).to(torch.int64)
    state[:2 * NB] += torch.bincount(row * NB + b, minlength=2 * NB)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from dmlnet import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(7)
    out_lab = (ctypes.c_int64 * 1)(OUT_LABEL)
    out_t = torch.tensor([OUT_LABEL], device="cuda")
    T = 9
    tt = (ctypes.c_float * T)(*[float(v) for v in np.linspace(0.1, 0.9, T)])

    def timed(fn, n_sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            fn(it % n_sets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def measure(fn, n_sets):
        for s in range(n_sets):
            fn(s)
        torch.cuda.synchronize()
        reps = [timed(fn, n_sets) for _ in range(a.reps)]
        return {"ms": round(float(np.median(reps)), 5), "spread_ms": round(max(reps) - min(reps), 5)}

    rows = []
    for (Hh, Ww) in ((720, 1280), (1024, 2048)):
        n = Hh * Ww
        for kind in ("spread", "contended"):
            n_sets = CACHE_BYTES // (20 * n) + 2
            sets = [make_inputs(kind, n, g) for _ in range(n_sets)]
            cube = torch.zeros((N_CLASSES, N_CLASSES, T + 1), dtype=torch.int64, device="cuda")

            def sweep(s):
                conf, label, _, pred = sets[s]
                _lib.check(lib.dml_open_set_sweep(conf.data_ptr(), pred.data_ptr(), label.data_ptr(), n, tt, T, out_lab, 1, N_CLASSES,
                                                  OUT_LABEL, cube.data_ptr(), None, 0, st), "dml_open_set_sweep")

            sweep_res = measure(sweep, n_sets)
            for NB in (256, 4096, 8192):
                state = torch.zeros(2 * NB + _lib.POOLED_OOD_COUNTERS, dtype=torch.int64, device="cuda")
                tstate = torch.zeros_like(state)
                result = torch.zeros(8, dtype=torch.float64, device="cuda")

                def update(s, masked=False):
                    conf, label, mask, _ = sets[s]
                    _lib.check(lib.dml_pooled_ood_update(conf.data_ptr(), label.data_ptr(), mask.data_ptr() if masked else None, n,
                                                         out_lab, 1, 0.0, 1.0, NB, state.data_ptr(), st), "dml_pooled_ood_update")

                def composed(s):
                    torch_update(sets[s][0], sets[s][1], out_t, NB, tstate)

                def finalize(s):
                    _lib.check(lib.dml_pooled_ood_finalize(state.data_ptr(), NB, 0.95, result.data_ptr(), st), "dml_pooled_ood_finalize")

                update(0)
                composed(0)
                torch.cuda.synchronize()
                hs, ht = state.cpu().numpy()[:2 * NB], tstate.cpu().numpy()[:2 * NB]
                moved = int(np.abs(hs - ht).sum()) // 2                   # pixels the torch route put into a neighbouring bin
                if hs.sum() != n or ht.sum() != n or hs[:NB].sum() != ht[:NB].sum() or moved > n // 1000:
                    raise SystemExit("%s %dx%d NB=%d: the torch route's histogram differs from the call's (%d pixels moved)"
                                     % (kind, Hh, Ww, NB, moved))
                res = {"update": measure(update, n_sets), "update_mask": measure(lambda s: update(s, True), n_sets),
                       "torch": measure(composed, n_sets), "finalize": measure(finalize, n_sets)}
                res["update"]["gbs"] = round(12 * n / res["update"]["ms"] / 1e6, 1)
                res["update_mask"]["gbs"] = round(13 * n / res["update_mask"]["ms"] / 1e6, 1)
                row = {"frame": [Hh, Ww], "NB": NB, "input": kind, **res, "sweep": dict(sweep_res, gbs=round(20 * n / sweep_res["ms"] / 1e6, 1)),
                       "torch_over_update": round(res["torch"]["ms"] / res["update"]["ms"], 2),
                       "update_over_sweep": round(res["update"]["ms"] / sweep_res["ms"], 2), "torch_moved_pixels": moved}
                rows.append(row)
                print("%-9s %4dx%-4d NB=%4d  update %.4f ms (+-%.4f, %6.1f GB/s)  masked %.4f ms (%6.1f GB/s)  torch %.4f ms  "
                      "sweep %.4f ms (+-%.4f)  finalize %.4f ms  torch/update %.2f  update/sweep %.2f"
                      % (kind, Hh, Ww, NB, res["update"]["ms"], res["update"]["spread_ms"], res["update"]["gbs"],
                         res["update_mask"]["ms"], res["update_mask"]["gbs"], res["torch"]["ms"], sweep_res["ms"],
                         sweep_res["spread_ms"], res["finalize"]["ms"], row["torch_over_update"], row["update_over_sweep"]), flush=True)
            del sets
    # the issue's two expectations, on what was measured
    by = {(tuple(r["frame"]), r["NB"], r["input"]): r for r in rows}
    keys = [(f, NB) for f in ((720, 1280), (1024, 2048)) for NB in (256, 4096, 8192)]
    cont = [{"frame": list(f), "NB": NB,
             "contended_over_spread": round(by[(f, NB, "contended")]["update"]["ms"] / by[(f, NB, "spread")]["update"]["ms"], 2),
             "difference_ms": round(by[(f, NB, "contended")]["update"]["ms"] - by[(f, NB, "spread")]["update"]["ms"], 5),
             "spread_of_repeats_ms": max(by[(f, NB, "contended")]["update"]["spread_ms"], by[(f, NB, "spread")]["update"]["spread_ms"])}
            for f, NB in keys]
    summary = {"iters": a.iters, "reps": a.reps, "rows": rows, "contended_vs_spread": cont,
               "max_update_over_sweep": max(r["update_over_sweep"] for r in rows),
               "min_torch_over_update": min(r["torch_over_update"] for r in rows)}
    print("update / sweep at most %.2f; torch / update at least %.2f; contended / spread: %s"
          % (summary["max_update_over_sweep"], summary["min_torch_over_update"], [c["contended_over_spread"] for c in cont]))
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
