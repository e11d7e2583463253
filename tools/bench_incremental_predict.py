"""Measurement tool (GPU box): the incremental model's merged prediction, fused against the per-head route.

    timeout -k 10 900 python3 tools/bench_incremental_predict.py [--iters 10] [--reps 5] [--out profiles/incremental_predict.json]

One process, the self-distillation model (16 + 17 prototypes, synthetic weights, eval mode).  Per configuration -- 1024 x 2048
batch 1 and 768 x 768 batch 16, each in f16x2 and bf16 -- it times
  fused   model.predict(x): the prediction plan, one dml_incremental_predict over the low-resolution embeddings
  heads   model(x) (a dml_upsample_dist_fwd per head: full-resolution logits and features) + the merge of
          test_self_distillation.py:292-297 with torch (an argmax per head, one masked assignment)
A repetition is --iters calls back to back between two device events, divided by --iters, after a warm-up of both routes;
the two routes alternate per repetition so that they see the same clocks.  The spread is (max - min) / median over the
--reps repetitions of one route; `ratio` = median heads / median fused.  Before timing, the two routes' predictions are
compared (share of differing pixels: they differ only where a head's two largest logits are within float32 rounding).
Prints one line per configuration and writes one JSON file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = [(1, 1024, 2048), (16, 768, 768)]
MODES = {"f16x2": (torch.float32, "f16x2"), "bf16": (torch.bfloat16, None)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "incremental_predict.json"))
    a = p.parse_args()
    import helpers as H
    import network
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    model = network.deeplabv3plus_embedding_self_distillation_resnet101(num_classes=16, output_stride=16,
                                                                        pretrained_backbone=False)
    model.load_state_dict(H.synth_state_dict(H.shapes_of(model), seed=5))
    model.to(dev).eval()

    def fused(x):
        return model.predict(x)

    def heads(x):
        lg, _, _ = model(x)
        pred = lg[0].max(dim=1)[1]
        pred[lg[1].max(dim=1)[1] == 16] = 16
        return pred

    def timed(fn, x):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    results = []
    with torch.no_grad():
        for mode, (dtype, products) in MODES.items():
            model.set_compute_dtype(dtype, fp32_products=products)
            for (B, Hh, Ww) in CONFIGS:
                x = torch.randn(B, 3, Hh, Ww, generator=torch.Generator().manual_seed(11)).to(dev)
                pf, ph = fused(x), heads(x)
                differ = (pf != ph).double().mean().item()
                for _ in range(2):
                    fused(x), heads(x)
                torch.cuda.synchronize()
                tf, th = [], []
                for _ in range(a.reps):
                    tf.append(timed(fused, x))
                    th.append(timed(heads, x))
                mf, mh = float(np.median(tf)), float(np.median(th))
                rec = dict(mode=mode, batch=B, height=Hh, width=Ww, fused_ms=mf, heads_ms=mh, ratio=mh / mf,
                           fused_spread=(max(tf) - min(tf)) / mf, heads_spread=(max(th) - min(th)) / mh,
                           fused_reps_ms=tf, heads_reps_ms=th, differing_pixel_share=differ,
                           overridden_share=(pf == 16).double().mean().item(), iters=a.iters)
                results.append(rec)
                print("%-5s %2d x %4d x %4d: fused %8.3f ms (spread %.1f %%)  heads %8.3f ms (spread %.1f %%)  ratio %.3f  "
                      "differing pixels %.2e" % (mode, B, Hh, Ww, mf, 100 * rec["fused_spread"], mh, 100 * rec["heads_spread"],
                                                 rec["ratio"], differ), flush=True)
                model._engine.plans.clear()             # the next configuration's plans need the memory
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/bench_incremental_predict.py", device=torch.cuda.get_device_name(0), results=results), fh,
                  indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
