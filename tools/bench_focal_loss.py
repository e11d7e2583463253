"""Measurement tool (GPU box): the focal loss, utils.FocalLoss against the route a user had before it, and what its
materialised gradient costs the train step.

    timeout -k 10 900 python3 tools/bench_focal_loss.py [--iters 20] [--reps 5] [--train-step] [--out F.json]

One process.  Logits of 16 x 16 x 768 x 768 (the train step's) and 4 x 19 x 1024 x 2048 (Cityscapes frames, every class), labels
with about 15 % ignored.  For each shape it times, forward + backward through the Python entry points with their allocations:
  focal     utils.FocalLoss(alpha=0.25, gamma=2): dml_focal_loss_fwd + _finalize + _bwd, four launches
  composed  the reference's statements (utils/loss.py:7-23) with torch operators and autograd on the device:
                ce = F.cross_entropy(x, y, reduction='none', ignore_index=255); pt = torch.exp(-ce)
                loss = (alpha * (1 - pt) ** gamma * ce).mean()
  ce        utils.CrossEntropyLoss() with its gradient materialised (dml_loss_fwd + _finalize + _bwd): the existing kernels
and the focal forward alone (no gradient asked for); "backward" is the difference.  A repetition is --iters calls back to back
between two events, divided by --iters, after a warm-up; the calls rotate through input sets so that none finds its input in
the 256 MB last-level cache (one set is larger than it).  The spread is max - min over the repetitions.  The traffic model is
4 K + 8 bytes per pixel forward (the logits and the labels once) and 8 K + 8 backward (logits and labels read, the gradient
written); the TB/s figures are that model over the measured times.  The focal and the composed route are compared with the
float64 definition of tests/focal_cases.py on a 1 x K x 64 x 64 corner of the first set.

--train-step: additionally runs main_embedding.py --synthetic --dtype f16x2 --batch_size 16 --crop_size 768 as child processes,
alternating --loss_type focal_loss (materialised gradient, unfused head backward) and cross_entropy (fused head backward),
--pairs times each, and reports ms per step from the driver's own images / s lines (the first interval of a run is dropped).
Prints one line per measurement and then one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open-world-semantic-segmentation_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((16, 16, 768, 768), (4, 19, 1024, 2048))
ALPHA, GAMMA = 0.25, 2.0
LLC_BYTES = 256 << 20


def composed(x, y):
    ce = F.cross_entropy(x, y, reduction="none", ignore_index=255)
    pt = torch.exp(-ce)
    return (ALPHA * (1 - pt) ** GAMMA * ce).mean()


def make_set(B, K, Hh, Ww, g):
    """negative squared distances of f = 3 e_t + noise to the prototypes 3 e_k (the generator of tests/focal_cases.py, on the
    device): t is the label on about 80 % of the pixels, about 15 % of the labels are ignored"""
    n = B * Hh * Ww
    y = torch.randint(0, K, (n,), generator=g, device="cuda")
    t = torch.where(torch.rand(n, generator=g, device="cuda") < 0.8, y, torch.randint(0, K, (n,), generator=g, device="cuda"))
    f = torch.randn(n, K, generator=g, device="cuda")
    f.scatter_add_(1, t[:, None], torch.full((n, 1), 3.0, device="cuda"))
    lg = -((f * f).sum(1, keepdim=True) - 6.0 * f + 9.0)
    y = torch.where(torch.rand(n, generator=g, device="cuda") < 0.15, torch.full_like(y, 255), y)
    return lg.view(B, Hh * Ww, K).transpose(1, 2).contiguous().view(B, K, Hh, Ww), y.view(B, Hh, Ww)


def driver_step_ms(loss_type, itrs, interval):
    args = [sys.executable, os.path.join(PKG, "main_embedding.py"), "--synthetic", "--dtype", "f16x2", "--batch_size", "16",
            "--crop_size", "768", "--loss_type", loss_type, "--total_itrs", str(itrs), "--print_interval", str(interval)]
    if loss_type == "focal_loss":
        args += ["--focal_alpha", str(ALPHA), "--focal_gamma", str(GAMMA)]
    r = subprocess.run(args, capture_output=True, text=True, cwd=PKG, timeout=600)
    if r.returncode != 0:
        raise SystemExit("main_embedding.py --loss_type %s failed:\n%s" % (loss_type, r.stdout[-1000:] + r.stderr[-2000:]))
    rates = [float(ln.split("Loss=")[1].split(",")[1].split()[0]) for ln in r.stdout.splitlines() if "Loss=" in ln]
    return [16e3 / v for v in rates[1:]]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--train-step", action="store_true")
    p.add_argument("--pairs", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    import utils
    import focal_cases as FC
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    focal, ce = utils.FocalLoss(alpha=ALPHA, gamma=GAMMA, ignore_index=255), utils.CrossEntropyLoss(ignore_index=255)

    def fwd_bwd(crit):
        def fn(s):
            x = s[0].requires_grad_(True)
            x.grad = None
            crit(x, s[1]).backward()
            return x.grad
        return fn

    def fwd_only(s):
        return focal(s[0].requires_grad_(False), s[1])

    def timed(fn, sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(a.iters):
            fn(sets[it % len(sets)])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    results = []
    for B, K, Hh, Ww in SHAPES:
        set_bytes = 4 * B * K * Hh * Ww
        sets = [make_set(B, K, Hh, Ww, g) for _ in range(LLC_BYTES // set_bytes + 2)]
        routes = {"focal": fwd_bwd(focal), "composed": fwd_bwd(composed), "ce": fwd_bwd(ce), "focal_fwd": fwd_only}
        # both routes against the float64 definition on a corner of the first set
        cx, cy = sets[0][0][:1, :, :64, :64].contiguous(), sets[0][1][:1, :64, :64].contiguous()
        ref = FC.focal_ref(cx.cpu().numpy(), cy.cpu().numpy(), ALPHA, GAMMA, True, 255)
        ratio = {}
        for what, crit in (("focal", focal), ("composed", composed)):
            grad = fwd_bwd(crit)((cx.clone(), cy)).cpu().numpy().astype(np.float64)
            pos = ref["grad_bar"] > 0
            ratio[what] = float((np.abs(grad - ref["grad"])[pos] / ref["grad_bar"][pos]).max())
        for fn in routes.values():                                      # warm-up over every set
            for s in sets:
                fn(s)
        torch.cuda.synchronize()
        reps = {what: [] for what in routes}
        for _ in range(a.reps):                                         # the routes alternate within a repetition
            for what, fn in routes.items():
                reps[what].append(timed(fn, sets))
        ms = {what: float(np.median(v)) for what, v in reps.items()}
        spread = {what: float(max(v) - min(v)) for what, v in reps.items()}
        px = B * Hh * Ww
        fwd_bytes, bwd_bytes = px * (4 * K + 8), px * (8 * K + 8)
        bwd_ms = ms["focal"] - ms["focal_fwd"]
        res = {"shape": [B, K, Hh, Ww], "alpha": ALPHA, "gamma": GAMMA, "iters": a.iters, "reps": a.reps, "sets": len(sets),
               "ms": {k: round(v, 4) for k, v in ms.items()}, "spread_ms": {k: round(v, 4) for k, v in spread.items()},
               "composed_over_focal": round(ms["composed"] / ms["focal"], 2), "focal_over_ce": round(ms["focal"] / ms["ce"], 3),
               "model_mbytes": {"fwd": round(fwd_bytes / 1e6, 1), "bwd": round(bwd_bytes / 1e6, 1)},
               "model_tbs": {"fwd": round(fwd_bytes / (ms["focal_fwd"] * 1e-3) / 1e12, 3),
                             "bwd": round(bwd_bytes / (bwd_ms * 1e-3) / 1e12, 3),
                             "fwd_bwd": round((fwd_bytes + bwd_bytes) / (ms["focal"] * 1e-3) / 1e12, 3)},
               "worst_err_over_bar": {k: round(v, 4) for k, v in ratio.items()}}
        print("%d x %d x %d x %d: focal fwd+bwd %.4f ms (spread %.4f), forward alone %.4f ms, composed %.4f ms (spread %.4f), "
              "CrossEntropyLoss unfused %.4f ms (spread %.4f); composed / focal = %.2f, focal / ce = %.3f; model %.0f + %.0f MB -> "
              "forward %.2f TB/s, backward %.2f TB/s; worst err/bar focal %.3f composed %.3f"
              % (B, K, Hh, Ww, ms["focal"], spread["focal"], ms["focal_fwd"], ms["composed"], spread["composed"], ms["ce"],
                 spread["ce"], ms["composed"] / ms["focal"], ms["focal"] / ms["ce"], fwd_bytes / 1e6, bwd_bytes / 1e6,
                 res["model_tbs"]["fwd"], res["model_tbs"]["bwd"], ratio["focal"], ratio["composed"]))
        results.append(res)
        del sets, cx, cy
        torch.cuda.empty_cache()
    out = {"focal_loss": results}
    if a.train_step:
        runs = {"focal_loss": [], "cross_entropy": []}
        for _ in range(a.pairs):
            for loss_type in runs:
                step = driver_step_ms(loss_type, 40, 10)
                runs[loss_type].append([round(v, 3) for v in step])
                print("main_embedding.py f16x2 16 x 768 x 768 --loss_type %s: ms per step per interval of 10 %s" % (loss_type, step))
        med = {k: float(np.median([x for run in v for x in run])) for k, v in runs.items()}
        out["train_step"] = {"ms_per_step_intervals": runs, "median_ms": {k: round(v, 3) for k, v in med.items()},
                             "focal_minus_cross_entropy_ms": round(med["focal_loss"] - med["cross_entropy"], 3)}
        print("train step: focal_loss %.3f ms, cross_entropy (fused head backward) %.3f ms, difference %.3f ms"
              % (med["focal_loss"], med["cross_entropy"], med["focal_loss"] - med["cross_entropy"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(r["worst_err_over_bar"]["focal"] <= 1.0 for r in results):
        raise SystemExit("utils.FocalLoss left the bar of tests/focal_cases.py")


if __name__ == "__main__":
    main()
