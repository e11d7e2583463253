"""Measurement tool (GPU box): the open-set threshold sweep of one frame, one launch against the composed route.

    timeout -k 10 600 python3 tools/bench_open_sweep.py [--iters 20] [--reps 5] [--no-model] [--out F.json]

One process.  Frames of 720 x 1280 with 14 classes and of 1024 x 2048 with 20, T = 1, 9 and 12 thresholds, three kinds of input:
  uniform       labels, predictions and confidences uniform at random
  concentrated  90 % of the pixels in one (label, prediction, top bin) cell, the rest uniform: what an evaluation frame looks
                like, and the case in which same-address LDS atomics serialise
  model         (720 x 1280 only, skipped with --no-model) the prediction, the `dissum` confidence and the label of one frame of
                `eval_ood_traditional.py --synthetic`, through the real model
It times
  sweep         dml_open_set_sweep through the C ABI into a preallocated cube (what OpenSetSweepMetrics.update launches)
  sweep+pred    the same call also writing open_pred for the middle threshold
  composed      the route without it, labels remapped once outside the clock: per threshold torch.where(conf >= t, pred, unknown)
                and dml_confusion_update into that threshold's matrix
A repetition is --iters calls back to back between two events, divided by --iters, after a warm-up; the calls rotate through enough
copies of the inputs (more than 320 MB) that none finds its input in the 256 MB last-level cache.  Reported per row: the median over
--reps repetitions, the spread (max - min), bytes / time for the traffic model of 20 bytes per pixel (28 with open_pred), and the
ratio composed / sweep.  Before timing, the matrices derived from the cube are compared with the composed route's: they must be
equal.  Prints one line per row and then one JSON line.
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


def thresholds_for(T):
    return [0.5] if T == 1 else [float(v) for v in np.linspace(0.1, 0.9, T)]


def make_inputs(kind, n, nc, g):
    label = torch.randint(0, nc, (n,), generator=g, device="cuda")
    pred = torch.randint(0, nc, (n,), generator=g, device="cuda")
    conf = torch.rand(n, generator=g, device="cuda")
    if kind == "concentrated":
        hot = torch.rand(n, generator=g, device="cuda") < 0.9
        label[hot], pred[hot], conf[hot] = 1, 1, 0.95
    return conf, pred, label


def model_frame(height, width):
    """conf, pred, label of the first frame of `eval_ood_traditional.py --synthetic --ood dissum` (bf16)"""
    import eval_ood_traditional as E
    import models
    import utils
    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights="")
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, weights="", use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).cuda().eval()
    seg.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(7)
    imgs = [torch.randn(1, 3, h, w, generator=g).cuda() for h, w in E.resized_shapes(height, width)]
    coarse = torch.randint(0, 14, ((height + 31) // 32, (width + 31) // 32), generator=g)
    lab = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:height, :width].contiguous().cuda()
    scores, ft1 = models.evaluate_multiscale(seg, imgs, (height, width))
    pred = utils.argmax_msp(scores)[0]
    conf = E.confidence(scores, "dissum", False, feats=ft1)
    torch.cuda.synchronize()
    return conf.reshape(-1).clone(), pred.reshape(-1).clone(), lab.reshape(-1).clone()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-model", action="store_true")
    p.add_argument("--out", default="")
    a = p.parse_args()
    from dmlnet import _lib
    from metrics.open_set import cube_to_matrix
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
    for (Hh, Ww, nc) in ((720, 1280, 14), (1024, 2048, 20)):
        n, u = Hh * Ww, nc - 1
        kinds = ["uniform", "concentrated"] + ([] if a.no_model or (Hh, Ww) != (720, 1280) else ["model"])
        for kind in kinds:
            n_sets = CACHE_BYTES // (20 * n) + 2
            if kind == "model":
                one = model_frame(Hh, Ww)
                sets = [tuple(t.clone() for t in one) for _ in range(n_sets)]
            else:
                sets = [make_inputs(kind, n, nc, g) for _ in range(n_sets)]
            out_lab = (ctypes.c_int64 * 1)(u)
            remapped = [s[2] for s in sets]                              # out_labels = (unknown_id,): the remap is the identity
            open_pred = torch.empty(n, dtype=torch.int64, device="cuda")
            unknown = torch.full((n,), u, dtype=torch.int64, device="cuda")
            for T in (1, 9, 12):
                ts = thresholds_for(T)
                tt = (ctypes.c_float * T)(*ts)
                tf = [float(np.float32(t)) for t in ts]
                cube = torch.zeros((nc, nc, T + 1), dtype=torch.int64, device="cuda")
                hists = torch.zeros((T, nc, nc), dtype=torch.int64, device="cuda")

                def sweep(s, write=False):
                    conf, pred, label = sets[s]
                    _lib.check(lib.dml_open_set_sweep(conf.data_ptr(), pred.data_ptr(), label.data_ptr(), n, tt, T, out_lab, 1, nc, u,
                                                      cube.data_ptr(), open_pred.data_ptr() if write else None, T // 2, st),
                               "dml_open_set_sweep")

                def composed(s):
                    conf, pred, _ = sets[s]
                    for i in range(T):
                        op = torch.where(conf >= tf[i], pred, unknown)
                        _lib.check(lib.dml_confusion_update(remapped[s].data_ptr(), op.data_ptr(), hists[i].data_ptr(), n, nc, st),
                                   "dml_confusion_update")

                sweep(0)
                composed(0)
                torch.cuda.synchronize()
                host = cube.cpu().numpy()
                same = all(np.array_equal(cube_to_matrix(host, i, u), hists[i].cpu().numpy()) for i in range(T))
                if not same:
                    raise SystemExit("%s %dx%d T=%d: the cube's matrices differ from the composed route's" % (kind, Hh, Ww, T))
                res = {}
                for name, fn in (("sweep", sweep), ("sweep_pred", lambda s: sweep(s, True)), ("composed", composed)):
                    for s in range(n_sets):
                        fn(s)
                    torch.cuda.synchronize()
                    reps = [timed(fn, n_sets) for _ in range(a.reps)]
                    res[name] = {"ms": round(float(np.median(reps)), 5), "spread_ms": round(max(reps) - min(reps), 5)}
                res["sweep"]["gbs"] = round(20 * n / res["sweep"]["ms"] / 1e6, 1)
                res["sweep_pred"]["gbs"] = round(28 * n / res["sweep_pred"]["ms"] / 1e6, 1)
                row = {"frame": [Hh, Ww], "n_classes": nc, "T": T, "input": kind, **res,
                       "composed_over_sweep": round(res["composed"]["ms"] / res["sweep"]["ms"], 2)}
                rows.append(row)
                print("%-12s %4dx%-4d K+1=%2d T=%2d  sweep %.4f ms (+-%.4f, %6.1f GB/s)  sweep+pred %.4f ms (%6.1f GB/s)  "
                      "composed %.4f ms  composed/sweep %.2f"
                      % (kind, Hh, Ww, nc, T, res["sweep"]["ms"], res["sweep"]["spread_ms"], res["sweep"]["gbs"],
                         res["sweep_pred"]["ms"], res["sweep_pred"]["gbs"], res["composed"]["ms"], row["composed_over_sweep"]),
                      flush=True)
            del sets
    # the issue's two expectations, on what was measured
    by = {(tuple(r["frame"]), r["T"], r["input"]): r for r in rows}
    conc = [round(by[(f, T, "concentrated")]["sweep"]["ms"] / by[(f, T, "uniform")]["sweep"]["ms"], 2)
            for f in ((720, 1280), (1024, 2048)) for T in (1, 9, 12)]
    summary = {"iters": a.iters, "reps": a.reps, "rows": rows, "concentrated_over_uniform": conc,
               "min_composed_over_sweep_T9": min(r["composed_over_sweep"] for r in rows if r["T"] == 9)}
    print("concentrated / uniform (sweep): %s; smallest composed / sweep at T = 9: %.2f"
          % (conc, summary["min_composed_over_sweep_T9"]))
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
