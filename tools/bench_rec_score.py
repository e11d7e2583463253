"""Measurement tool (GPU box): the reconstruction-consistency score of one frame, utils.rec_cosine_score +
utils.rec_confidence against the reference's statements composed from torch operators on the same GPU and inputs.

    timeout -k 10 600 python3 tools/bench_rec_score.py [--calls 5] [--torch_calls 2] [--reps 5] [--out F.json]

One process, one StreetHazards frame: label size 720 x 1280, the pyramid concats of its five resized copies (the sizes of
datasets.streethazards.resized_shapes over the encoder's stride of 8: 38 x 67 ... 71 x 125, 28 791 pixels) with C = 4096
channels, for the frame and for its reconstruction, in fp32 and in bf16, and 13 x 720 x 1280 scores.  It times
  hip    utils.rec_cosine_score(f1, f2, (180, 320)) (dml_rec_cosine, one launch) and utils.rec_confidence(scores, cos,
         prob="softmax") (dml_rec_confidence, one launch)
  torch  anomaly/eval_ood_rec.py:96-125,141-150 of the reference: two zero accumulators [1, 4096, 180, 320] fp32, per
         scale and input F.interpolate(bilinear) and `ft = ft + ft_temp / n`, then F.normalize twice, F.cosine_similarity,
         F.interpolate to the label size, the maximum of the softmax and the gate (a bf16 concat is converted with .float()
         in front of its interpolate).
Both routes run through Python as a caller gets them.  A repetition is --calls (--torch_calls) calls back to back between
two events, divided by the number of calls, after a warm-up call of each route; the figure is the median over --reps
repetitions and the spread their max - min.  The kernel's rate is one read of every source element of both inputs,
2 x 28 791 x 4096 elements, over the time of the cosine call.  The inputs are 943 MB in fp32 and 472 MB in bf16, both above
the 256 MB last-level cache.  If the composed route does not fit in memory that is reported instead of a ratio.  The two
routes are compared on every pixel.  Prints one line per measurement and then one JSON line.
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

FRAME, C, K, STRIDE = (720, 1280), 4096, 13, 8
THRESHOLD = 0.999
ROUTES_BAR = 4e-5                # each route may sit 2e-5 (tests/rec_cases.py's GPU_BAR) from the float64 definition


def torch_cosine(f1, f2, out_hw):
    n = len(f1)

    def accumulate(feats):
        ft = torch.zeros(feats[0].shape[0], feats[0].shape[-1], out_hw[0], out_hw[1], device=feats[0].device)
        for f in feats:
            ft_temp = F.interpolate(f.float().permute(0, 3, 1, 2), size=ft.shape[2:], mode="bilinear", align_corners=False)
            ft = ft + ft_temp / n
        return ft

    ft1, ft2 = F.normalize(accumulate(f1), dim=1), F.normalize(accumulate(f2), dim=1)
    return F.cosine_similarity(ft1, ft2, dim=1)


def torch_confidence(scores, cos, t):
    msp, _ = torch.max(F.softmax(scores, dim=1), dim=1)
    ft_dist = F.interpolate(cos.unsqueeze(1), size=scores.shape[2:], mode="bilinear", align_corners=False)[:, 0]
    return msp * (msp > t).float() + ft_dist * (msp <= t).float()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--torch_calls", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    import utils
    from datasets.streethazards import resized_shapes
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(12)
    out_hw = (int(FRAME[0] / 4), int(FRAME[1] / 4))
    scales = [(h // STRIDE, w // STRIDE) for h, w in resized_shapes(*FRAME)]
    pixels = sum(h * w for h, w in scales)
    scores = 9.0 * torch.randn(1, K, *FRAME, device="cuda", generator=g)      # about a fifth of the pixels above 0.999

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def measure(fn, calls):
        reps = [timed(fn, calls) for _ in range(a.reps)]
        return float(np.median(reps)), float(max(reps) - min(reps))

    results = []
    for dtype in (torch.float32, torch.bfloat16):
        name = "bf16" if dtype == torch.bfloat16 else "f32"
        f1 = [torch.randn(1, h, w, C, device="cuda", generator=g).to(dtype) for h, w in scales]
        f2 = [(t.float() + 0.7 * torch.randn(t.shape, device="cuda", generator=g)).to(dtype) for t in f1]
        src_bytes = 2 * pixels * C * f1[0].element_size()
        cos = utils.rec_cosine_score(f1, f2, out_hw)                           # warm-up, and the comparison
        conf = utils.rec_confidence(scores, cos, threshold=THRESHOLD, prob="softmax")
        torch.cuda.synchronize()
        cos_ms, cos_spread = measure(lambda: utils.rec_cosine_score(f1, f2, out_hw), a.calls)
        conf_ms, conf_spread = measure(lambda: utils.rec_confidence(scores, cos, threshold=THRESHOLD, prob="softmax"), a.calls)
        gbs = src_bytes / (cos_ms * 1e-3) / 1e9
        res = {"dtype": name, "frame": list(FRAME), "scales": scales, "C": C, "source_mbytes": round(src_bytes / 1e6, 1),
               "calls": a.calls, "torch_calls": a.torch_calls, "reps": a.reps,
               "hip": {"cosine_ms": round(cos_ms, 4), "cosine_spread_ms": round(cos_spread, 4), "confidence_ms": round(conf_ms, 4),
                       "confidence_spread_ms": round(conf_spread, 4), "ms": round(cos_ms + conf_ms, 4),
                       "cosine_source_gbs": round(gbs, 1)}}
        print("%s: hip cosine %.3f ms (spread %.3f; %.1f MB of sources once -> %.0f GB/s), confidence %.3f ms (spread %.3f)"
              % (name, cos_ms, cos_spread, src_bytes / 1e6, gbs, conf_ms, conf_spread))
        try:
            tcos = torch_cosine(f1, f2, out_hw)                                # warm-up, and the comparison
            tconf = torch_confidence(scores, tcos, THRESHOLD)
            torch.cuda.synchronize()
            near = (F.softmax(scores, dim=1).amax(1) - THRESHOLD).abs() <= ROUTES_BAR
            d_cos = float((cos - tcos).abs().max())
            d_conf = float(((conf - tconf).abs() * (~near)).max())
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tcos_ms, tcos_spread = measure(lambda: torch_cosine(f1, f2, out_hw), a.torch_calls)
            peak = torch.cuda.max_memory_allocated() - base
            tconf_ms, tconf_spread = measure(lambda: torch_confidence(scores, tcos, THRESHOLD), a.torch_calls)
            res["torch"] = {"cosine_ms": round(tcos_ms, 3), "cosine_spread_ms": round(tcos_spread, 3),
                            "confidence_ms": round(tconf_ms, 3), "confidence_spread_ms": round(tconf_spread, 3),
                            "ms": round(tcos_ms + tconf_ms, 3), "cosine_peak_temporaries_mbytes": round(peak / 1e6, 1)}
            res["torch_over_hip"] = {"cosine": round(tcos_ms / cos_ms, 2), "confidence": round(tconf_ms / conf_ms, 2),
                                     "both": round((tcos_ms + tconf_ms) / (cos_ms + conf_ms), 2)}
            res["routes_max_abs_diff"] = {"cos": d_cos, "conf": d_conf}
            res["routes_agree"] = d_cos <= ROUTES_BAR and d_conf <= ROUTES_BAR
            print("%s: torch cosine %.3f ms (spread %.3f, %.0f MB of temporaries at its peak), confidence %.3f ms (spread %.3f); "
                  "torch / hip = %.2f (cosine), %.2f (confidence), %.2f (both); routes differ by at most %.2e (cos), %.2e (conf)"
                  % (name, tcos_ms, tcos_spread, peak / 1e6, tconf_ms, tconf_spread, tcos_ms / cos_ms, tconf_ms / conf_ms,
                     (tcos_ms + tconf_ms) / (cos_ms + conf_ms), d_cos, d_conf))
            del tcos, tconf
        except torch.cuda.OutOfMemoryError:
            res["torch"] = "the composed route does not fit in memory"
            print("%s: the composed torch route does not fit in memory" % name)
        results.append(res)
        del f1, f2, cos, conf
        torch.cuda.empty_cache()
    line = json.dumps({"rec_score": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(r.get("routes_agree", True) for r in results):
        raise SystemExit("the two routes differ by more than %.0e" % ROUTES_BAR)


if __name__ == "__main__":
    main()
