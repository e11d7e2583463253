"""Reconstruction-consistency open-set evaluation of the anomaly sub-project on the MI355X path (reference:
anomaly/eval_ood_rec.py, `evaluate` :63-199 and `main` :201-252, with config/test_ood_rec.yaml).

Every frame comes with a reconstruction of itself (`DATASET.rec_dataset`, a second tree of images; producing them is not
part of the reference either).  Both go through the same multi-scale model; the decoder's 4096-channel pyramid concat of
the two (`ft = ppm_out.clone()`, models.py:632 of the reference) is averaged over the scales at a quarter of the label
size, normalised and compared by cosine similarity (:96-125,143-146), and that map, resized to the label size, is the
confidence wherever the maximum score does not exceed a threshold (:141,147-150, t = 0.999).
`models.evaluate_multiscale_rec` returns the frame's scores and the cosine map, `utils.rec_confidence` the confidence:
two kernels where the reference holds two 4096 x H/4 x W/4 accumulators (944 MB each at 720 x 1280) and rewrites them
for every scale.  As the reference stands this driver cannot run: the decoder's live `return` hands back the
13-channel embedding, which does not add into the accumulators the driver allocates; the pyramid concat is what those
accumulators' 4096 channels mean.

`--rec_prob logit` (the default) is the reference's literal `msp = max(tmp_scores)` on its un-softmaxed scores, which are
negative squared distances: with the threshold of 0.999 the gate never opens and the confidence is the cosine map alone.
`--rec_prob softmax` takes the maximum softmax probability, what the name and the 0.999 intend.  `--ood msp` is :137-139,
the maximum score itself, and needs no reconstruction.
`eval_ood_measure`, the arg-max and the pixel accuracy / IoU meters run on the device as in eval_ood_traditional.py, whose
summary this driver prints.  Data: the reference's command line (`--cfg FILE`, `--gpu`, `--ood`, `--exclude_back` and
trailing `KEY VALUE` overrides, `DATASET.rec_dataset` among them) on two StreetHazards-layout trees, or `--synthetic`
frames whose reconstruction differs from the frame exactly on the anomaly-labelled blocks.
"""
import argparse
import os
import time

import numpy as np
import torch

import anom_utils
import eval_ood_traditional as T
import metrics as metrics_mod
import models
import utils

# the reference's t = 0.999 (:149) and its literal maximum of the scores (:141); main() puts --rec_threshold / --rec_prob here
REC = {"threshold": 0.999, "prob": "logit"}

# eval_ood_traditional's keys plus the tree of reconstructions (anomaly/config/defaults.py:15 of the reference)
CFG_DEFAULTS = dict(T.CFG_DEFAULTS)
CFG_DEFAULTS["DATASET.rec_dataset"] = "./data"


def load_cfg(cfg_file, overrides):
    """eval_ood_traditional.load_cfg over this driver's defaults"""
    cfg = T.load_cfg(cfg_file, overrides)
    for k, v in CFG_DEFAULTS.items():
        cfg.setdefault(k, v)
    return cfg


def confidence(scores, cos, ood, exclude_back=False):
    """:127-150.  scores [1, K, H, W], cos [1, Hq, Wq] on the device -> conf [H, W] on the device."""
    if ood == "msp":
        return T.confidence(scores, "maxlogit", exclude_back)
    if ood == "rec":
        return utils.rec_confidence(scores, cos, threshold=REC["threshold"], prob=REC["prob"],
                                    first_class=1 if exclude_back else 0)[0]
    raise NotImplementedError("--ood %s" % ood)


def evaluate(segmentation_module, frames, num_class, ood, out_labels, exclude_back=False, pooled=None):
    """frames: iterable of (img_resized_list, img_resized_list_rec, seg_label int64 [H, W]) on the device.  pooled: an
    anom_utils.PooledOodMeasures that is given every frame's `conf` and `seg_label` as well (results under "pooled")."""
    seg_metrics = metrics_mod.StreamSegMetrics(num_class)
    aurocs, auprs, fprs, times = [], [], [], []
    known = num_class
    for imgs, imgs_rec, seg_label in frames:
        torch.cuda.synchronize()
        tic = time.perf_counter()
        seg_size = tuple(seg_label.shape)
        if ood == "rec":
            scores, cos = models.evaluate_multiscale_rec(segmentation_module, imgs, imgs_rec, seg_size)
        else:
            scores, cos = models.evaluate_multiscale(segmentation_module, imgs, seg_size)[0], None
        known = scores.shape[1]
        pred = utils.argmax_msp(scores)[0]
        conf = confidence(scores, cos, ood, exclude_back)
        res = anom_utils.eval_ood_measure(conf, seg_label, out_labels)
        if res is not None:
            aurocs.append(res[0]); auprs.append(res[1]); fprs.append(res[2])
        seg_metrics.update(seg_label[None], pred)
        if pooled is not None:
            pooled.update(conf, seg_label)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - tic)
    r = {"auroc": float(np.mean(aurocs)) if aurocs else float("nan"),
         "aupr": float(np.mean(auprs)) if auprs else float("nan"),
         "fpr": float(np.mean(fprs)) if fprs else float("nan"),
         "seg": seg_metrics.get_results(), "sec_per_frame": float(np.mean(times[1:] or times)),
         "known_iou": T.known_class_iou(seg_metrics, known)}
    if pooled is not None:
        r["pooled"] = pooled.get_results()
    return r


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ood", default="rec", choices=["rec", "msp"])
    p.add_argument("--rec_threshold", type=float, default=REC["threshold"],
                   help="--ood rec: the maximum score above which it replaces the cosine map (the reference's t = 0.999)")
    p.add_argument("--rec_prob", default=REC["prob"], choices=["logit", "softmax"],
                   help="--ood rec: the maximum of the scores themselves (the reference's statement; the gate never opens on "
                        "its negative distances) or of their softmax")
    p.add_argument("--exclude_back", action="store_true")
    T.add_pooled_arguments(p)
    p.add_argument("--out_label", type=int, default=13, help="cfg.OOD.out_labels: the anomaly id of StreetHazards")
    p.add_argument("--num_images", type=int, default=4)
    p.add_argument("--height", type=int, default=720)
    p.add_argument("--width", type=int, default=1280)
    p.add_argument("--encoder_weights", default="")
    p.add_argument("--decoder_weights", default="")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"],
                   help="as eval_ood_traditional.py: bf16 storage, exact fp32, or fp32 tensors with split products")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--cfg", default="", metavar="FILE", help="yaml config of the reference (read only when given)")
    p.add_argument("--gpu", type=int, default=0, help="gpu to use")
    p.add_argument("--workers", type=int, default=0,
                   help="decode threads per reader of the real-data run (default: min(16, CPUs this process may use))")
    p.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (real-data run)")
    return p


def synthetic_frames(num_images, height, width, out_label, device, seed=7):
    """Random copies as in eval_ood_traditional.py's --synthetic run and a label map of 32 x 32 blocks; the reconstruction
    is the frame with the pixels of the anomaly-labelled blocks replaced by other noise, so that the cosine map carries
    the anomaly and the three OOD numbers are not degenerate."""
    g = torch.Generator().manual_seed(seed)
    shapes = T.resized_shapes(height, width)
    for _ in range(num_images):
        imgs = [torch.randn(1, 3, h, w, generator=g).to(device) for h, w in shapes]
        coarse = torch.randint(0, 14, ((height + 31) // 32, (width + 31) // 32), generator=g)
        lab = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:height, :width].contiguous()
        anomalous = (lab == out_label)[None, None].float()
        recs = []
        for img, (h, w) in zip(imgs, shapes):
            mask = torch.nn.functional.interpolate(anomalous, size=(h, w), mode="nearest").bool().to(device)
            recs.append(torch.where(mask, torch.randn(1, 3, h, w, generator=g).to(device), img))
        yield imgs, recs, lab.to(device)


def main():
    opts = build_parser().parse_args()
    REC.update(threshold=opts.rec_threshold, prob=opts.rec_prob)
    device = torch.device("cuda", opts.gpu)
    torch.cuda.set_device(device)
    torch.manual_seed(304)
    cfg = None if opts.synthetic else load_cfg(opts.cfg, opts.opts)
    num_class = 13 if cfg is None else int(cfg["DATASET.num_class"])
    enc_w, dec_w = opts.encoder_weights, opts.decoder_weights
    if cfg is not None:
        enc_w = enc_w or os.path.join(cfg["DIR"], "encoder_" + cfg["VAL.checkpoint"])
        dec_w = dec_w or os.path.join(cfg["DIR"], "decoder_" + cfg["VAL.checkpoint"])
        if not (os.path.exists(enc_w) and os.path.exists(dec_w)):
            raise SystemExit("checkpoint does not exist: %s / %s" % (enc_w, dec_w))
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights=enc_w)
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=num_class,
                                            weights=dec_w, use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).to(device).eval()
    seg.set_compute_dtype(torch.bfloat16 if opts.dtype == "bf16" else torch.float32,
                          fp32_products={"f32": "exact", "f32x3": "bf16x3", "f16x2": "f16x2"}.get(opts.dtype))
    if cfg is not None:
        run_dataset(seg, cfg, opts, num_class, device)
        return
    frames = synthetic_frames(opts.num_images, opts.height, opts.width, opts.out_label, device)
    pooled = T.make_pooled(opts, (opts.out_label,))
    r = evaluate(seg, frames, 14, opts.ood, (opts.out_label,), opts.exclude_back, pooled=pooled)
    print("mean auroc = ", r["auroc"], "mean aupr = ", r["aupr"], " mean fpr = ", r["fpr"])          # :199
    if pooled is not None:
        T.print_pooled(r["pooled"], pooled, opts.pooled_curve)
    print("Mean IoU: %.4f, Accuracy: %.2f%%, Inference Time: %.4fs" % (r["seg"]["Mean IoU"], 100.0 * r["seg"]["Overall Acc"],
                                                                        r["sec_per_frame"]))


def run_dataset(seg, cfg, opts, num_class, device):
    """The reference's `main` + summary (:192-199,221-252): two readers over the same list, zipped."""
    from datasets.streethazards import StreetHazardsReader
    kw = dict(img_sizes=tuple(cfg["DATASET.imgSizes"]), img_max_size=cfg["DATASET.imgMaxSize"],
              padding_constant=cfg["DATASET.padding_constant"], workers=opts.workers or None, device=device)
    reader = StreetHazardsReader(cfg["DATASET.root_dataset"], cfg["DATASET.list_val"], **kw)
    reader_rec = StreetHazardsReader(cfg["DATASET.root_dataset"], cfg["DATASET.list_val"],
                                     rec_dataset=cfg["DATASET.rec_dataset"], **kw)
    print("# samples: {}".format(len(reader)))
    frames = ((imgs, imgs_rec, seg_label) for (imgs, seg_label), (imgs_rec, _) in zip(reader, reader_rec))
    tic = time.perf_counter()
    pooled = T.make_pooled(opts, (opts.out_label,))
    r = evaluate(seg, frames, num_class + 1, opts.ood, (opts.out_label,), opts.exclude_back, pooled=pooled)
    wall = time.perf_counter() - tic
    for i, iou in enumerate(r["known_iou"]):
        print("class [{}], IoU: {:.4f}".format(i, iou))
    print("[Eval Summary]:")
    print("Mean IoU: {:.4f}, Accuracy: {:.2f}%, Inference Time: {:.4f}s"
          .format(r["known_iou"].mean(), 100.0 * r["seg"]["Overall Acc"], r["sec_per_frame"]))
    print("mean auroc = ", r["auroc"], "mean aupr = ", r["aupr"], " mean fpr = ", r["fpr"])
    if pooled is not None:
        T.print_pooled(r["pooled"], pooled, opts.pooled_curve)
    print("Wall clock: {:.2f} frames/s ({} frames, {} decode workers per reader); model only: {:.2f} frames/s"
          .format(len(reader) / wall, len(reader), reader.workers, 1.0 / r["sec_per_frame"]))
    print("Evaluation Done!")


if __name__ == "__main__":
    main()
