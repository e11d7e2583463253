"""Measurement tool (GPU box): the Inter and Center terms of utils.DMLLoss(beta=, gamma=) -- dml_metric_fwd / _finalize / _bwd --
against the same definition composed from torch operators, and what the terms cost main_embedding.py's train step.

    timeout -k 10 900 python3 tools/bench_metric_terms.py [--iters 10] [--reps 5] [--train-step] [--fused-only] [--out F.json]

One process.  Logits [16, 16, 768, 768], features [16, 768, 768, 16] (the train step's), labels with about 15 % ignored pixels,
features 3 e_y + N(0, 0.3^2).  It times, through the C ABI on preallocated buffers (the terms alone, without the cross entropy):
  fwd         dml_metric_fwd + dml_metric_finalize (four launches + one)
  bwd         dml_metric_bwd: the feature gradient written, the Inter gradient added into a logit-gradient buffer in place
  fwd_bwd     both, back to back
and, with autograd on the device,
  vectorised  the definition with index_add_ for the class sums and counts, a gather for the means and for the own-class logit
  loop        the reference's route in this tool's words: per image `unique` with its host round trip, per class nonzero +
              index_select of logits and features, mean, squared deviations, the two accumulators over the pixel count (the
              features of an image as [H W, C]; the reference's own indexing raises)
A repetition is --iters calls back to back between two events, divided by --iters, after a warm-up (the loop route: 2 calls);
the calls rotate through two input sets, each larger than the 256 MB last-level cache.  The spread is max - min over the
repetitions.  Traffic model, bytes per pixel with K classes and C channels:
  forward   2 x 4 C (the features read twice) + 4 K (the logits once) + 3 x 8 (the labels per launch)
  backward  4 C read + 4 C written (features, their gradient) + 2 x 4 K (the logit gradient read and written) + 2 x 8 (labels)
the GB/s figures are that model over the measured times.  The fused route is compared with the float64 definition of
tests/metric_cases.py on a 1 x 64 x 64 corner of the first set.

--train-step: additionally runs main_embedding.py --synthetic --loss_type dml --dtype f16x2 --batch_size 16 --crop_size 768 as
child processes with and without --beta 1e-4 --gamma 1e-2, in an order that alternates, --pairs times each, and reports ms per
step from the driver's own img/s lines (the first interval of a run is dropped).  With the terms the loss gradient is
materialised and the head's unfused backward runs, so the difference is the terms PLUS the loss of the fused head backward.
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

B, HH, WW, K, C = 16, 768, 768, 16, 16
BETA, GAMMA, IGNORE = 1e-4, 1e-2, 255


def make_set(g):
    y = torch.randint(0, K, (B, HH, WW), generator=g, device="cuda")
    f = 0.3 * torch.randn(B, HH, WW, C, generator=g, device="cuda")
    f.scatter_add_(3, y[..., None], torch.full((B, HH, WW, 1), 3.0, device="cuda"))
    # logits = minus the squared distances to the prototypes 3 e_k, plane by plane (nothing of size B H W K C)
    lg = torch.empty(B, K, HH, WW, device="cuda")
    sq = (f * f).sum(-1)
    for k in range(K):
        lg[:, k] = -(sq - 6.0 * f[..., k] + 9.0)
    y = torch.where(torch.rand(B, HH, WW, generator=g, device="cuda") < 0.15, torch.full_like(y, IGNORE), y)
    return lg, f, y


def vectorised(lg, f, y):
    n, k, h, w = lg.shape
    N = h * w
    valid = (y != IGNORE).view(n, N)
    yc = torch.where(valid, y.view(n, N), torch.zeros_like(y.view(n, N)))
    idx = (yc + k * torch.arange(n, device=y.device)[:, None]).view(-1)
    ff = f.view(n * N, -1)
    vm = valid.view(-1, 1).to(f.dtype)
    sums = torch.zeros(n * k, ff.shape[1], device=f.device).index_add_(0, idx, ff * vm)
    cnt = torch.zeros(n * k, device=f.device).index_add_(0, idx, vm[:, 0])
    mu = sums / cnt.clamp(min=1)[:, None]
    d = (ff - mu[idx]) * vm
    center = (d * d).sum() / N
    lf = lg.view(n, k, N)
    own = lf.gather(1, yc[:, None, :])[:, 0]
    inter = ((lf.sum(1) - own) * valid).sum() / N
    return (BETA * inter + GAMMA * center) / n


def loop(lg, f, y):
    """the reference's route (utils/loss.py:46-79 there) in this tool's words, with its operators: a host round trip per image
    for the classes present, then per class two row gathers, a mean and three reductions"""
    batch, k = lg.shape[0], lg.shape[1]
    push = lg.new_zeros(())
    spread = lg.new_zeros(())
    for img in range(batch):
        flat_y = y[img].reshape(-1)
        pixel_logits = lg[img].permute(1, 2, 0).reshape(-1, k)                   # a pixel-major copy, as the reference makes
        pixel_feats = f[img].reshape(flat_y.numel(), -1)
        present, how_many = torch.unique(flat_y, return_counts=True)
        pixels = int(how_many.sum())                                            # device -> host, as np.unique is there
        for cls in (int(c) for c in present.tolist() if int(c) != IGNORE):
            rows = (flat_y == cls).nonzero().squeeze(1)
            lk = pixel_logits.index_select(0, rows)
            fk = pixel_feats.index_select(0, rows)
            dev = fk - fk.mean(dim=0)
            spread = spread + dev.pow(2).sum() / pixels
            push = push + (lk.sum() - lk[:, cls].sum()) / pixels
    return (BETA * push + GAMMA * spread) / batch


def driver_step_ms(extra, itrs, interval):
    args = [sys.executable, os.path.join(PKG, "main_embedding.py"), "--synthetic", "--loss_type", "dml", "--dtype", "f16x2",
            "--batch_size", "16", "--crop_size", "768", "--total_itrs", str(itrs), "--print_interval", str(interval)] + extra
    r = subprocess.run(args, capture_output=True, text=True, cwd=PKG, timeout=600)
    if r.returncode != 0:
        raise SystemExit("main_embedding.py %s failed:\n%s" % (extra, r.stdout[-1000:] + r.stderr[-2000:]))
    lines = [ln for ln in r.stdout.splitlines() if "Loss=" in ln]
    rates = [float(ln.split("Loss=")[1].split(",")[1].split()[0]) for ln in lines]
    losses = [float(ln.split("Loss=")[1].split(",")[0]) for ln in lines]
    return [16e3 / v for v in rates[1:]], losses


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--train-step", action="store_true")
    p.add_argument("--fused-only", action="store_true", help="skip the torch routes (for a kernel trace of the fused launches)")
    p.add_argument("--pairs", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    import metric_cases as MC
    from dmlnet import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(23)
    sets = [make_set(g) for _ in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.empty(2 * B + 3, dtype=torch.float64, device="cuda")
    work = torch.empty(_lib.metric_work_doubles(K, C), dtype=torch.float64, device="cuda")
    means = torch.empty(B, K, C, device="cuda")
    counts = torch.empty(B, K, dtype=torch.int32, device="cuda")
    term = torch.empty(1, device="cuda")
    gl = torch.zeros(B, K, HH, WW, device="cuda")
    gf = torch.empty(B, HH, WW, C, device="cuda")

    def fwd(s, shape=(B, HH, WW)):
        lg, f, y = s
        _lib.check(lib.dml_metric_fwd(lg.data_ptr(), f.data_ptr(), y.data_ptr(), means.data_ptr(), counts.data_ptr(), sums.data_ptr(),
                                      work.data_ptr(), shape[0], K, C, shape[1], shape[2], IGNORE, st), "dml_metric_fwd")
        _lib.check(lib.dml_metric_finalize(sums.data_ptr(), shape[0], BETA, GAMMA, float(shape[0]), term.data_ptr(), st),
                   "dml_metric_finalize")

    def bwd(s, shape=(B, HH, WW)):
        lg, f, y = s
        _lib.check(lib.dml_metric_bwd(f.data_ptr(), y.data_ptr(), means.data_ptr(), sums.data_ptr(), None, gl.data_ptr(), gf.data_ptr(),
                                      shape[0], K, C, shape[1], shape[2], IGNORE, BETA, GAMMA, float(shape[0]), st), "dml_metric_bwd")

    def both(s):
        fwd(s)
        bwd(s)

    def auto(fn):
        def run(s):
            lg, f, y = s
            lg.requires_grad_(True).grad = None
            f.requires_grad_(True).grad = None
            fn(lg, f, y).backward()
        return run

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(iters):
            fn(sets[it % len(sets)])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    # the fused route against the float64 definition on a corner of the first set
    corner = (sets[0][0][:1, :, :64, :64].contiguous(), sets[0][1][:1, :64, :64].contiguous(), sets[0][2][:1, :64, :64].contiguous())
    ref = MC.metric_ref(*(x.cpu().numpy() for x in corner), IGNORE, BETA, GAMMA)
    gl.zero_()
    fwd(corner, (1, 64, 64))
    bwd(corner, (1, 64, 64))
    torch.cuda.synchronize()
    got = gf.view(-1)[:64 * 64 * C].view(1, 64, 64, C).cpu().numpy().astype(np.float64)
    pos = ref["gf_bar"] > 0
    worst = float((np.abs(got - ref["gf"])[pos] / ref["gf_bar"][pos]).max())
    worst_term = float(abs(float(term.item()) - ref["term"]) / ref["term_bar"])
    gl.zero_()

    routes = {"fwd": (fwd, a.iters), "bwd": (bwd, a.iters), "fwd_bwd": (both, a.iters), "vectorised": (auto(vectorised), a.iters),
              "loop": (auto(loop), 2)}
    if a.fused_only:
        routes = {k: v for k, v in routes.items() if k in ("fwd", "bwd", "fwd_bwd")}
    for fn, _ in routes.values():
        for s in sets:
            fn(s)
    torch.cuda.synchronize()
    reps = {what: [] for what in routes}
    for _ in range(a.reps):
        for what, (fn, iters) in routes.items():
            reps[what].append(timed(fn, iters))
    ms = {what: float(np.median(v)) for what, v in reps.items()}
    spread = {what: float(max(v) - min(v)) for what, v in reps.items()}
    for what in ("vectorised", "loop"):                                 # --fused-only: not measured
        ms.setdefault(what, float("nan"))
        spread.setdefault(what, float("nan"))
    px = B * HH * WW
    fwd_bytes, bwd_bytes = px * (8 * C + 4 * K + 24), px * (8 * C + 8 * K + 16)
    gbs = lambda nbytes, t_ms: round(nbytes / (t_ms * 1e-3) / 1e9, 1)          # noqa: E731
    out = {"metric_terms": {"shape": [B, HH, WW], "K": K, "C": C, "iters": a.iters, "reps": a.reps,
                            "ms": {k: round(v, 4) for k, v in ms.items()}, "spread_ms": {k: round(v, 4) for k, v in spread.items()},
                            "vectorised_over_fused": round(ms["vectorised"] / ms["fwd_bwd"], 2),
                            "loop_over_fused": round(ms["loop"] / ms["fwd_bwd"], 2),
                            "model_mbytes": {"fwd": round(fwd_bytes / 1e6, 1), "bwd": round(bwd_bytes / 1e6, 1)},
                            "model_gbs": {"fwd": gbs(fwd_bytes, ms["fwd"]), "bwd": gbs(bwd_bytes, ms["bwd"]),
                                          "fwd_bwd": gbs(fwd_bytes + bwd_bytes, ms["fwd_bwd"])},
                            "worst_err_over_bar": {"feature_gradient": round(worst, 4), "term": round(worst_term, 4)}}}
    print("%d x %d x %d, K = C = %d: fused forward %.4f ms (spread %.4f), backward %.4f ms (spread %.4f), both %.4f ms (spread %.4f); "
          "vectorised torch %.4f ms (spread %.4f), per-image loop %.2f ms; vectorised / fused = %.2f, loop / fused = %.1f; model "
          "%.0f + %.0f MB -> forward %.0f GB/s, backward %.0f GB/s, both %.0f GB/s; worst err/bar feature gradient %.3f, term %.3f"
          % (B, HH, WW, K, ms["fwd"], spread["fwd"], ms["bwd"], spread["bwd"], ms["fwd_bwd"], spread["fwd_bwd"], ms["vectorised"],
             spread["vectorised"], ms["loop"], ms["vectorised"] / ms["fwd_bwd"], ms["loop"] / ms["fwd_bwd"], fwd_bytes / 1e6,
             bwd_bytes / 1e6, out["metric_terms"]["model_gbs"]["fwd"], out["metric_terms"]["model_gbs"]["bwd"],
             out["metric_terms"]["model_gbs"]["fwd_bwd"], worst, worst_term))
    del sets, gl, gf
    torch.cuda.empty_cache()
    if a.train_step:
        flags = {"with": ["--beta", str(BETA), "--gamma", str(GAMMA)], "without": []}
        runs, losses = {k: [] for k in flags}, {k: [] for k in flags}
        for pair in range(a.pairs):
            for w in (list(flags) if pair % 2 == 0 else list(flags)[::-1]):
                step, loss = driver_step_ms(flags[w], 40, 10)
                runs[w].append([round(v, 3) for v in step])
                losses[w].append(loss)
                print("main_embedding.py --loss_type dml f16x2 16 x 768 x 768 %s the terms: ms per step per interval of 10 %s, mean loss "
                      "per interval %s" % (w, step, loss))
        med = {k: float(np.median([x for run in v for x in run])) for k, v in runs.items()}
        out["train_step"] = {"ms_per_step_intervals": runs, "loss_per_interval": losses,
                             "median_ms": {k: round(v, 3) for k, v in med.items()},
                             "terms_and_unfused_head_ms": round(med["with"] - med["without"], 3)}
        print("train step: with --beta %g --gamma %g %.3f ms, without %.3f ms; the difference %.3f ms is the terms (%.3f ms above) plus "
              "the materialised loss gradient and the unfused head backward" % (BETA, GAMMA, med["with"], med["without"],
                                                                                 med["with"] - med["without"], ms["fwd_bwd"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if worst > 1.0 or worst_term > 1.0:
        raise SystemExit("the fused metric terms left the bar of tests/metric_cases.py")


if __name__ == "__main__":
    main()
