#!/usr/bin/env python3
"""Incremental few-shot open-world evaluation with one, two or three (up to 8) novel classes: test_embedding.py's
evaluation step (test_embedding.py:225-653 of the reference) with the 16+2 / 16+3 rules the reference keeps commented
out at :509-530 and the shot extraction of :413-425.  test_embedding.py stays the single-prototype driver it was; with
one --prototype_json file (or none) this driver computes what that one computes, through one call per frame
(utils.open_world_post: argmax, max-softmax score, dissum map and relabel in one pass) instead of three.  Images are
sharded round-robin over ranks; the only collectives are the two sums at the very end.

    python eval_open_world.py --synthetic --num_images 4 --prototype_json car.json truck.json bus.json [--novel_only]
    python eval_open_world.py --synthetic --num_images 4 --extract_prototypes 13 14 15 --shots_out DIR

Prototype j is class num_classes + j; --extract_prototypes writes DIR/prototype_<id>.json, the lists of shots that
--prototype_json reads.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import network  # noqa: E402
import utils  # noqa: E402
from dmlnet import parallel  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="deeplabv3plus_embedding_resnet101")
    p.add_argument("--num_classes", type=int, default=16)
    p.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    p.add_argument("--ckpt", default=None)
    p.add_argument("--prototype_json", default=None, nargs="+",
                   help="k-shot prototype vectors (prototype_car_5_shot.json), one file per novel class: prototype j is "
                        "class num_classes + j")
    p.add_argument("--novel_only", action="store_true",
                   help="compare the novel-class distances only with each other and the threshold (:510-511,:520-522), "
                        "not with the known classes' logits (:445)")
    p.add_argument("--extract_prototypes", type=int, nargs="+", default=None, metavar="ID",
                   help="collect one shot per frame and class id (:413-425) instead of evaluating; needs --shots_out")
    p.add_argument("--shots_out", default=None, metavar="DIR", help="where prototype_<id>.json files go")
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=2048)
    p.add_argument("--num_images", type=int, default=4)
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"],
                   help="bf16: bf16 storage (throughput mode); f32: exact fp32 MFMA (the reference's arithmetic); f16x2 / f32x3: fp32 tensors with the convolution products on the fp16 / bf16 matrix cores (fp32-accurate splits, bench.py's headline is f16x2)")
    return p


def main():
    o = build_parser().parse_args()
    if o.extract_prototypes and not o.shots_out:
        raise SystemExit("--extract_prototypes needs --shots_out DIR")
    if not o.synthetic:
        raise SystemExit("only --synthetic data is available (datasets are outside the hot path)")
    rank, local, world = parallel.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(1)              # without --ckpt every rank must still build the same (random-init) model
    model = getattr(network, o.model)(num_classes=o.num_classes, output_stride=o.output_stride,
                                      pretrained_backbone=False)
    if o.ckpt:
        model.load_state_dict(torch.load(o.ckpt, map_location="cpu")["model_state"])    # :748-749
    model.to(dev).eval()                                                                # :773
    model.set_compute_dtype(torch.bfloat16 if o.dtype == "bf16" else torch.float32,
                            fp32_products={"f32": "exact", "f32x3": "bf16x3", "f16x2": "f16x2"}.get(o.dtype))
    if o.prototype_json:
        protos = []
        for f in o.prototype_json:                                                      # :245-258
            with open(f) as fh:
                protos.append(utils.mean_prototype(json.load(fh)))
        protos = np.stack(protos)
    else:
        protos = np.full((1, o.num_classes), 0.1)
    n_novel = protos.shape[0]
    new_labels = [o.num_classes + j for j in range(n_novel)]
    import anom_utils
    import metrics as metrics_mod
    seg_metrics = metrics_mod.StreamSegMetrics(o.num_classes + n_novel)                # 16 known classes + the novel ones
    shots = {c: [] for c in (o.extract_prototypes or [])}
    aurocs, auprs, fprs = [], [], []
    n, t0 = 0, None
    with torch.no_grad():
        for i in range(rank, o.num_images, world):
            g = torch.Generator().manual_seed(4321 + i)
            img = torch.randn(1, 3, o.height, o.width, generator=g).to(dev)
            # synthetic ground truth: blocky train ids, the block-classes from num_classes up play the unknown objects
            coarse = torch.randint(0, o.num_classes + n_novel, (1, (o.height + 63) // 64, (o.width + 63) // 64), generator=g)
            target = coarse.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :o.height, :o.width].contiguous().to(dev)
            outputs, centers, features = model(img)                                     # :337
            if shots:                                                                   # :413-425
                for c, shot in utils.extract_prototypes(features, target, list(shots)).items():
                    if shot is not None:
                        shots[c].append((i, shot))
                continue
            # :339-342 (argmax, msp), :349-350,365 (dissum), :428-445 / :509-522 (relabel): one pass
            preds, msp, score = utils.open_world_post(outputs, features, protos, new_labels, thresh=-1.5,
                                                      vs_known=not o.novel_only, clip=1000.0, inclusive=False)
            seg_metrics.update(target, preds)                                           # :455 (metrics.update), on the device
            # pixel-level OOD measures of the anomaly score (eval_ood_traditional.py:128-148; the reference's `conf`
            # is a confidence, i.e. minus the anomaly score)
            res = anom_utils.eval_ood_measure(-score.reshape(-1).float(), target.reshape(-1), new_labels)
            if res is not None:
                aurocs.append(res[0]); auprs.append(res[1]); fprs.append(res[2])
            if t0 is None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            else:
                n += 1
    torch.cuda.synchronize()
    if shots:
        # rank 0 collects the (frame, shot) pairs of every rank and writes one file per class, in frame order: the list
        # mean_prototype reads, the same file whatever the number of ranks
        if world > 1:
            import torch.distributed as dist
            parts = [None] * world
            dist.all_gather_object(parts, shots)
            shots = {c: sum((part[c] for part in parts), []) for c in shots}
        if rank == 0:
            os.makedirs(o.shots_out, exist_ok=True)
            for c, v in shots.items():
                path = os.path.join(o.shots_out, "prototype_%d.json" % c)
                with open(path, "w") as fh:
                    json.dump([shot for _, shot in sorted(v)], fh)
                print("class %d: %d shots -> %s" % (c, len(v), path))
        return
    n_meas = len(aurocs)
    if world > 1:
        # every rank has scored its shard of the images: sum the confusion matrix and the per-image measures (sum,
        # count) over the ranks, so that rank 0 reports the whole evaluation set, as the reference's single process does
        import torch.distributed as dist
        seg_metrics.all_reduce()
        tot = torch.tensor([float(np.sum(aurocs)), float(np.sum(auprs)), float(np.sum(fprs)), float(n_meas)],
                           dtype=torch.float64, device=dev)
        dist.all_reduce(tot)
        n_meas = int(tot[3].item())
        mean_meas = (tot[:3] / max(n_meas, 1)).tolist()
    else:
        mean_meas = [float(np.mean(v)) if v else float("nan") for v in (aurocs, auprs, fprs)]
    if rank == 0:
        results = seg_metrics.get_results()
        print(seg_metrics.to_str(results))
        print("Class IoU (%d classes, the last %d novel):" % (o.num_classes + n_novel, n_novel))
        for c in range(o.num_classes + n_novel):
            print("  %2d: %f" % (c, results["Class IoU"][c]))
        if n_meas:          # frames without a novel-class pixel have no OOD measures (anom_utils.eval_ood_measure -> None)
            anom_utils.print_measures(mean_meas[0], mean_meas[1], mean_meas[2], "dissum")
    if n:
        print("rank %d: %.2f img/s at %dx%d (%d novel-class pixels in the last image, score mean %.4f)"
              % (rank, n / (time.perf_counter() - t0), o.height, o.width, int((preds >= o.num_classes).sum()),
                 float(score.mean())))


if __name__ == "__main__":
    main()
