"""Open-set evaluation driver of the anomaly sub-project on the MI355X path (reference: anomaly/eval_ood_traditional.py,
`evaluate` :150-560 and `main` :563-640, with config/test_ood_street.yaml: resnet50dilated + ppm_deepsup_embedding,
13 classes, imgSizes (300, 375, 450, 525, 600), imgMaxSize 1000, padding_constant 8).

Per frame: the resized copies go through `models.evaluate_multiscale` (the loop of :198-210, mean folded into the
upsample kernel, scales concurrent), `pred = argmax` (:218), the confidence map of `--ood`
(:275-340: msp | maxlogit | dissum | background; :302-305,434-435,447-448: dissum_msp -- the paper's "EDS + MMSP", the
normalised distance sum d and the normalised maximum softmax q mixed as c d + (1 - c) q under the gate
c = 1 / (1 + exp(mix_slope (d - mix_threshold))), which the reference computes on every dissum frame and then overwrites
with a leftover `conf = dis_sum` at :450; one kernel pair, utils.dissum_msp_score, and no copy for --exclude_back;
and :511-530: knn -- the sum, over the 8 x 8 pixels down-right and the
8 x 8 pixels up-left of each pixel, of the cosine similarity between its embedding `ft1` and theirs, 0 beyond the image
border: the reference's 128 rounds of zero-filled shifted copies in one kernel, utils.knn_cosine_score; its plt.figure /
imshow / show calls and its resize of the map to segSize, the identity on a map that already has that size, are not
reproduced; and :492-510: crf-gauss -- a dense CRF on the scores whose only pairwise term is a spatial Gaussian
(sxy = 3, Potts compat = 3, 100 mean-field steps), conf = the largest marginal: the reference copies the scores to the host
and runs pydensecrf's lattice on one CPU thread, here each step is two 1-D blurs and a softmax on the device,
utils.dense_crf_gauss, with the intended geometry (the reference passes (h, w) where DenseCRF2D takes (width, height)) and
no copy for --exclude_back (the reference stops at setUnaryEnergy with it).  The other CRF variant, `crf`, is not offered:
its bilateral kernel over the 13-channel scores needs a 15-dimensional lattice filter, which is not separable; and `ecdf`
-- the calibrated score the reference keeps commented in DeepLabV3Plus-Pytorch/main_embedding.py:106-113,172-226,249-260 and
test_embedding.py:155-163,361-364: a fit pass, `calibrate`, counts the distance sums of the correctly predicted pixels of
known-class frames into one histogram per class on the device, and conf = sum_cl softmax_cl * Certainty(E_cl(distance sum))
with those empirical CDFs, utils.EcdfCalibrator; the only confidence here that is not normalised per frame, so that a value
means the same on every frame), then
`eval_ood_measure`
(:128-148) and the pixel accuracy / IoU meters (:548-556) -- all on the device; nothing but the three OOD numbers and
the confusion counts per frame reaches the host.  `--pooled` adds the same three measures over all pixels of the run at once
(anom_utils.PooledOodMeasures: every frame's confidence and label streamed into one histogram on the device) and the confidence
threshold that reaches the recall level, beside the means of the per-frame figures.
Data: a StreetHazards-layout tree from disk (the reference's command line: `--cfg FILE`, `--gpu`, `--ood`,
`--exclude_back` and trailing `KEY VALUE` overrides; datasets/streethazards.py decodes on host threads and resizes /
normalises on the device, bit for bit the reference's ValDataset tensors), or `--synthetic` frames.
"""
import argparse
import ast
import contextlib
import os
import time

import numpy as np
import torch

import anom_utils
import metrics as metrics_mod
import models
import utils

IMG_SIZES, IMG_MAX_SIZE, PADDING_CONSTANT = (300, 375, 450, 525, 600), 1000, 8
# the gate of `--ood dissum_msp`: the reference's Coefficient_map(dis_sum, 0.2) with lamda = 50 (:104-106,447); main() puts
# --mix_threshold / --mix_slope here
MIX = {"threshold": 0.2, "slope": 50.0}
# `--ood crf-gauss`: the reference's addPairwiseGaussian(sxy=3, compat=3) and inference(100) (:501,504); main() puts
# --crf_sxy / --crf_compat / --crf_iters here
CRF = {"sxy": 3.0, "compat": 3.0, "iters": 100}
# `--ood ecdf`: the certainty of the reference's two commented `Certainty` bodies (DeepLabV3Plus-Pytorch/main_embedding.py:106-113:
# hard, E if E <= 0.15 else 1; test_embedding.py:155-163: a sigmoid of slope 50 around the mixture threshold), on the driver's
# `dissum` clip; main() puts --ecdf_mode / --ecdf_cut / --ecdf_slope / --ecdf_bins / --ecdf_clip here, and the calibration itself
# (utils.EcdfCalibrator, from calibrate() or --ecdf_load) under "calibrator", set and put back by use_calibrator(): confidence() and
# evaluate() keep their signatures
ECDF = {"mode": "hard", "cut": 0.15, "slope": 50.0, "bins": 1024, "clip": 400.0, "calibrator": None}
# `--pooled`: the anom_utils.PooledOodMeasures that evaluate() also feeds, set and put back by use_pooled(); None: no pooled measures
POOLED = {"measures": None}


def resized_shapes(h, w):
    """dataset.py's TestDataset sizes: short side -> each of IMG_SIZES, long side <= IMG_MAX_SIZE, both rounded up to a
    multiple of PADDING_CONSTANT."""
    from datasets.streethazards import resized_shapes as shapes
    return shapes(h, w, IMG_SIZES, IMG_MAX_SIZE, PADDING_CONSTANT)


def confidence(scores, ood, exclude_back=False, feats=None):
    """:275-340, :434-448, :492-530.  scores [1, K, H, W] on the device -> conf [H, W] on the device.  `knn` reads the
    embedding feats [1, C, H, W] instead of the scores (the reference's `ft1`), so --exclude_back does not touch it.
    `dissum_msp` takes its gate from MIX, `crf-gauss` its kernel width, strength and step count from CRF; both skip the
    background class inside the kernel.  `ecdf` is the calibrated score: sum_cl softmax_cl * Certainty(E_cl(distance sum)) with
    the per-class ECDFs of ECDF["calibrator"] (utils.EcdfCalibrator, filled by calibrate()) and the certainty of ECDF; it is
    not normalised per frame."""
    if ood == "ecdf":
        cal = ECDF["calibrator"]
        if cal is None:
            raise ValueError("--ood ecdf needs a calibration: `with use_calibrator(calibrate(...)):` or utils.EcdfCalibrator.load")
        if cal.first_class != (1 if exclude_back else 0):
            raise ValueError("the calibration starts at class %d: exclude_back does not match it" % cal.first_class)
        return cal.score(scores, mode=ECDF["mode"], cut=ECDF["cut"], slope=ECDF["slope"])[0]
    if ood == "knn":
        if feats is None:
            raise ValueError("--ood knn scores the embedding: pass feats")
        return utils.knn_cosine_score(feats)[0]
    if ood == "dissum_msp":
        return utils.dissum_msp_score(scores, clip=400.0, threshold=MIX["threshold"], slope=MIX["slope"],
                                      first_class=1 if exclude_back else 0)[0]
    if ood == "crf-gauss":
        return utils.dense_crf_gauss(scores, sxy=CRF["sxy"], compat=CRF["compat"], iters=CRF["iters"],
                                     first_class=1 if exclude_back else 0)[0]
    tmp = scores[:, 1:].contiguous() if exclude_back else scores
    if ood == "msp":
        return utils.argmax_msp(tmp)[1][0]
    if ood == "maxlogit":
        preds = utils.argmax_msp(tmp)[0]
        return tmp.gather(1, preds.unsqueeze(1))[0, 0]
    if ood == "dissum":
        return utils.dissum_score(tmp, clip=400.0, inclusive=True)[0]
    if ood == "background":
        return tmp[0, 0]
    raise NotImplementedError("--ood %s" % ood)


@contextlib.contextmanager
def use_calibrator(calibrator):
    """`with use_calibrator(cal): evaluate(..., ood="ecdf")`: the calibration confidence() and evaluate() score with inside the block;
    what was set before comes back on the way out, also after an exception, so that no device-holding object stays behind in
    the module's settings"""
    previous = ECDF["calibrator"]
    ECDF["calibrator"] = calibrator
    try:
        yield calibrator
    finally:
        ECDF["calibrator"] = previous


@contextlib.contextmanager
def use_pooled(pooled):
    """`with use_pooled(anom_utils.PooledOodMeasures(...)): r = evaluate(...)`: the dataset-level accumulator evaluate() feeds
    inside the block (None: none, and evaluate() does what it does without one); what was set before comes back on the way out.
    It travels here, as the calibration does, because evaluate()'s positional signature is pinned."""
    previous = POOLED["measures"]
    POOLED["measures"] = pooled
    try:
        yield pooled
    finally:
        POOLED["measures"] = previous


def calibrate(segmentation_module, frames, num_known, exclude_back=False, max_frames=0, calibrator=None):
    """The fit pass of `--ood ecdf` (the collection loop the reference keeps commented at main_embedding.py:177-197, without its
    1-in-500 subsampling): frames as evaluate() takes them, known-class frames by intent; each goes through the same multi-scale
    forward and every pixel whose label equals its prediction is counted into the calibrator's per-class histogram on the
    device.  max_frames caps the frames read (0: all).  -> utils.EcdfCalibrator"""
    cal = calibrator
    for i, (imgs, seg_label) in enumerate(frames):
        if max_frames and i >= max_frames:
            break
        scores, _ = models.evaluate_multiscale(segmentation_module, imgs, tuple(seg_label.shape))
        if cal is None:
            cal = utils.EcdfCalibrator(scores.shape[1], ECDF["clip"], ECDF["bins"], first_class=1 if exclude_back else 0)
        cal.update(scores, seg_label[None])
    if cal is None:
        cal = utils.EcdfCalibrator(num_known, ECDF["clip"], ECDF["bins"], first_class=1 if exclude_back else 0)
    return cal


def evaluate(segmentation_module, frames, num_class, ood, out_labels, exclude_back=False, open_set_thresholds=None):
    """frames: iterable of (img_resized_list, seg_label int64 [H, W]) on the device.  open_set_thresholds: score the
    open-set prediction (:537-549, `pred[conf < thre] = out_labels[0]`) at each of them as well (:155-156,599-607) and
    return the per-threshold results under "open_set".  Inside `with use_pooled(p):` the anom_utils.PooledOodMeasures `p` is
    given every frame's `conf` and `seg_label` as well, and its dataset-level results come back under "pooled"."""
    pooled = POOLED["measures"]
    seg_metrics = metrics_mod.StreamSegMetrics(num_class)
    sweep = metrics_mod.OpenSetSweepMetrics(num_class, open_set_thresholds, out_labels[0], out_labels) \
        if open_set_thresholds else None
    aurocs, auprs, fprs, times = [], [], [], []
    known = num_class
    for imgs, seg_label in frames:
        torch.cuda.synchronize()
        tic = time.perf_counter()
        seg_size = tuple(seg_label.shape)
        scores, ft1 = models.evaluate_multiscale(segmentation_module, imgs, seg_size)
        known = scores.shape[1]
        pred = utils.argmax_msp(scores)[0]
        conf = confidence(scores, ood, exclude_back, feats=ft1)
        res = anom_utils.eval_ood_measure(conf, seg_label, out_labels)
        if res is not None:
            aurocs.append(res[0]); auprs.append(res[1]); fprs.append(res[2])
        seg_metrics.update(seg_label[None], pred)
        if sweep is not None:
            sweep.update(seg_label, pred, conf)
        if pooled is not None:
            pooled.update(conf, seg_label)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - tic)
    r = {"auroc": float(np.mean(aurocs)) if aurocs else float("nan"),
         "aupr": float(np.mean(auprs)) if auprs else float("nan"),
         "fpr": float(np.mean(fprs)) if fprs else float("nan"),
         "seg": seg_metrics.get_results(), "sec_per_frame": float(np.mean(times[1:] or times)),
         "known_iou": known_class_iou(seg_metrics, known)}
    if sweep is not None:
        r["open_set"] = sweep.get_results()
    if pooled is not None:
        r["pooled"] = pooled.get_results()
    return r


def print_open_set(results):
    """the per-threshold table and the threshold with the best open-set mean IoU (the reference picks its best threshold
    the same way, by its unknown IoU, :645-653)"""
    print(metrics_mod.OpenSetSweepMetrics.to_str(results), end="")
    best = results[int(np.nanargmax([x["Mean IoU"] for x in results]))]
    print("Best open-set Mean IoU: %.4f at threshold %.4f" % (best["Mean IoU"], best["Threshold"]))


def add_pooled_arguments(p):
    """--pooled and its settings, shared with eval_ood_rec.py"""
    p.add_argument("--pooled", action="store_true",
                   help="also report AUROC / AUPR / FPR over all pixels of the run at once (anom_utils.PooledOodMeasures) beside "
                        "the means of the per-frame figures, and the confidence threshold that reaches the recall level")
    p.add_argument("--pooled_bins", type=int, default=4096, help="--pooled: bins of the confidence histogram, 1 .. 8192")
    p.add_argument("--pooled_range", type=float, nargs=2, default=(0.0, 1.0), metavar=("LO", "HI"),
                   help="--pooled: the confidence range the bins divide.  The default suits msp, dissum, dissum_msp, ecdf, "
                        "crf-gauss and rec; maxlogit, background and knn are not confined to [0, 1] and need their own range")
    p.add_argument("--pooled_curve", default="", metavar="FILE.npz",
                   help="--pooled: write the cumulative curve (tp, fp, bin edges) to FILE.npz")


def make_pooled(opts, out_labels):
    """the accumulator of a --pooled run, None without the flag"""
    if not opts.pooled:
        return None
    return anom_utils.PooledOodMeasures(out_labels, lo=opts.pooled_range[0], hi=opts.pooled_range[1], bins=opts.pooled_bins)


def print_pooled(res, pooled, curve_file=""):
    """the line after `mean auroc = ...`: the pooled measures, the AUROC interval binning leaves, the threshold at the recall
    level and the pixels outside the range; then the curve file"""
    if res is None:
        c = pooled.counters()
        print("pooled: no OOD pixel or only OOD pixels were counted (frames = %d, nan = %d, masked = %d)"
              % (c["frames"], c["n_nan"], c["n_masked"]))
    else:
        print("pooled auroc = ", res["auroc"], "pooled aupr = ", res["aupr"], " pooled fpr = ", res["fpr"],
              " auroc bounds = [%.9f, %.9f]" % res["auroc_bounds"],
              " threshold at recall %g = %.9g" % (pooled.recall_level, res["threshold"]),
              " below range = %d above range = %d nan = %d" % (res["n_below"], res["n_above"], res["n_nan"]))
        outside, seen = res["n_below"] + res["n_above"], res["positives"] + res["negatives"]
        if outside > 0.01 * seen:
            print("WARNING: %d of %d pixels (%.2f%%) lie outside --pooled_range [%g, %g]; they were counted in its end bins"
                  % (outside, seen, 100.0 * outside / seen, pooled.lo, pooled.hi))
    if curve_file:
        tp, fp, edges = pooled.curve()
        np.savez(curve_file, tp=tp, fp=fp, edges=edges)


def known_class_iou(seg_metrics, known):
    """The reference's per-class IoU (utils.py intersectionAndUnion(pred, label, num_class) summed over frames, then
    intersection / (union + 1e-10)): the first `known` classes of the confusion matrix only -- the model's classes,
    not the anomaly label -- and a class that never occurs counts as 0.  Its mean is the reference's `Mean IoU`."""
    if seg_metrics.confusion_matrix is None:
        return np.zeros(known)
    counts = seg_metrics.confusion_matrix.cpu().numpy().astype(np.float64)
    tp = np.diag(counts)[:known]
    union = counts.sum(axis=1)[:known] + counts.sum(axis=0)[:known] - tp
    return tp / (union + 1e-10)


# the configuration keys the real-data run honours (anomaly/config/defaults.py of the reference for the defaults)
CFG_DEFAULTS = {
    "DATASET.root_dataset": "./data/",
    "DATASET.list_val": "./data/validation.odgt",
    "DATASET.list_calib": "./data/training.odgt",       # the reference's DATASET.list_train: known classes only
    "DATASET.num_class": 13,
    "DATASET.imgSizes": IMG_SIZES,
    "DATASET.imgMaxSize": IMG_MAX_SIZE,
    "DATASET.padding_constant": PADDING_CONSTANT,
    "DIR": "ckpt/ade20k-resnet50dilated-ppm_deepsup",
    "VAL.checkpoint": "epoch_20.pth",
}


def _decode_value(v):
    """yacs' _decode_cfg_value: strings that are Python literals become those literals"""
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


def load_cfg(cfg_file, overrides):
    """Flat "SECTION.key" -> value: the defaults, then the yaml file (read only when given), then KEY VALUE pairs."""
    cfg = dict(CFG_DEFAULTS)
    if cfg_file:
        import yaml
        with open(cfg_file) as f:
            tree = yaml.safe_load(f) or {}

        def walk(node, prefix):
            for k, v in node.items():
                if isinstance(v, dict):
                    walk(v, prefix + k + ".")
                else:
                    cfg[prefix + k] = _decode_value(v)
        walk(tree, "")
    if len(overrides) % 2:
        raise SystemExit("overrides come in KEY VALUE pairs: %r" % (overrides,))
    for k, v in zip(overrides[0::2], overrides[1::2]):
        cfg[k] = _decode_value(v)
    return cfg


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ood", default="dissum", choices=["msp", "maxlogit", "dissum", "background", "knn",
                                                           "dissum_msp", "crf-gauss", "ecdf"])
    p.add_argument("--ecdf_mode", default=ECDF["mode"], choices=["hard", "sigmoid"],
                   help="--ood ecdf: the certainty of an ECDF value E -- hard: E if E <= --ecdf_cut else 1; sigmoid: "
                        "1 / (1 + exp(-ecdf_slope (E - E(threshold)))) around each class's Gaussian-mixture threshold")
    p.add_argument("--ecdf_cut", type=float, default=ECDF["cut"], help="--ood ecdf: the hard mode's cut (the reference's 0.15)")
    p.add_argument("--ecdf_slope", type=float, default=ECDF["slope"],
                   help="--ood ecdf: the sigmoid mode's steepness (the reference's coefficient = 50)")
    p.add_argument("--ecdf_bins", type=int, default=ECDF["bins"], help="--ood ecdf: bins of the per-class histograms, at most 2048")
    p.add_argument("--ecdf_clip", type=float, default=ECDF["clip"],
                   help="--ood ecdf: the distance sum at which the histograms end (the driver's dissum clip)")
    p.add_argument("--ecdf_calib", type=int, default=None, metavar="N",
                   help="--ood ecdf: calibrate on N frames first (synthetic run: N generated frames; real-data run: the first N "
                        "frames of DATASET.list_calib, 0 for all of them)")
    p.add_argument("--ecdf_load", default="", metavar="FILE", help="--ood ecdf: read the calibration from FILE instead")
    p.add_argument("--ecdf_save", default="", metavar="FILE", help="--ood ecdf: write the calibration to FILE")
    p.add_argument("--mix_threshold", type=float, default=MIX["threshold"],
                   help="--ood dissum_msp: the normalised distance sum at which the gate is 1/2 (the reference's 0.2)")
    p.add_argument("--mix_slope", type=float, default=MIX["slope"],
                   help="--ood dissum_msp: the gate's steepness (the reference's lamda = 50)")
    p.add_argument("--crf_sxy", type=float, default=CRF["sxy"],
                   help="--ood crf-gauss: the Gaussian's standard deviation in pixels (the reference's sxy = 3; at most 8)")
    p.add_argument("--crf_compat", type=float, default=CRF["compat"],
                   help="--ood crf-gauss: the Potts strength of the pairwise term (the reference's compat = 3)")
    p.add_argument("--crf_iters", type=int, default=CRF["iters"],
                   help="--ood crf-gauss: mean-field steps (the reference's inference(100))")
    p.add_argument("--exclude_back", action="store_true")
    p.add_argument("--open_set_thresholds", type=float, nargs="+", default=None, metavar="T",
                   help="also score the open-set prediction (pixels whose confidence is below T become --out_label) at each "
                        "of these increasing thresholds, at most 12; the reference's sweep is 0.1 ... 0.9 on a confidence "
                        "normalised to [0, 1]")
    add_pooled_arguments(p)
    p.add_argument("--out_label", type=int, default=13, help="cfg.OOD.out_labels: the anomaly id of StreetHazards")
    p.add_argument("--num_images", type=int, default=4)
    p.add_argument("--height", type=int, default=720)
    p.add_argument("--width", type=int, default=1280)
    p.add_argument("--encoder_weights", default="")
    p.add_argument("--decoder_weights", default="")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"],
                   help="bf16: bf16 storage (throughput mode); f32: exact fp32 MFMA (the reference's arithmetic); f16x2 / f32x3: fp32 tensors with the convolution products on the fp16 / bf16 matrix cores (fp32-accurate splits, bench.py's headline is f16x2)")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--cfg", default="", metavar="FILE", help="yaml config of the reference (read only when given)")
    p.add_argument("--gpu", type=int, default=0, help="gpu to use")
    p.add_argument("--workers", type=int, default=0,
                   help="decode threads of the real-data run (default: min(16, CPUs this process may use))")
    p.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides (real-data run)")
    return p


def check_ecdf_source(opts):
    """`--ood ecdf` needs its calibration from somewhere: --ecdf_load FILE or --ecdf_calib N"""
    if opts.ood == "ecdf" and not opts.ecdf_load and opts.ecdf_calib is None:
        raise SystemExit("--ood ecdf needs a calibration: --ecdf_calib N (fit on N frames first) or --ecdf_load FILE")
    if opts.ood == "ecdf" and not opts.ecdf_load and opts.synthetic and opts.ecdf_calib < 1:
        raise SystemExit("--synthetic --ood ecdf generates its calibration frames: --ecdf_calib N with N >= 1")


def ecdf_calibrator(seg, opts, frames, num_known):
    """the calibrator of a `--ood ecdf` run: loaded from --ecdf_load, or fitted on `frames` (a callable, so that nothing is built
    when the file is there); written to --ecdf_save when asked, and reported per class"""
    if opts.ood != "ecdf":
        return None
    if opts.ecdf_load:
        cal = utils.EcdfCalibrator.load(opts.ecdf_load)
        want_first = 1 if opts.exclude_back else 0
        if cal.num_classes != num_known or cal.first_class != want_first:
            raise SystemExit("%s holds %d classes from class %d on; this run has %d from %d on"
                             % (opts.ecdf_load, cal.num_classes, cal.first_class, num_known, want_first))
        ECDF.update(bins=cal.nbins, clip=cal.clip)
    else:
        cal = calibrate(seg, frames(), num_known, opts.exclude_back, max_frames=opts.ecdf_calib)
    if opts.ecdf_save:
        cal.save(opts.ecdf_save)
    print("ECDF calibration: %d pixels, per class %s" % (int(cal.counts().sum()), cal.counts().tolist()))
    return cal


def main():
    opts = build_parser().parse_args()
    MIX.update(threshold=opts.mix_threshold, slope=opts.mix_slope)
    CRF.update(sxy=opts.crf_sxy, compat=opts.crf_compat, iters=opts.crf_iters)
    ECDF.update(mode=opts.ecdf_mode, cut=opts.ecdf_cut, slope=opts.ecdf_slope, bins=opts.ecdf_bins, clip=opts.ecdf_clip)
    check_ecdf_source(opts)
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
    g = torch.Generator().manual_seed(7)
    shapes = resized_shapes(opts.height, opts.width)

    def frames():
        for _ in range(opts.num_images):
            imgs = [torch.randn(1, 3, h, w, generator=g).to(device) for h, w in shapes]
            coarse = torch.randint(0, 14, ((opts.height + 31) // 32, (opts.width + 31) // 32), generator=g)
            lab = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:opts.height, :opts.width].contiguous()
            yield imgs, lab.to(device)

    def calib_frames():
        # known classes only, from a generator of its own: the evaluation frames are the same with and without --ood ecdf
        gc = torch.Generator().manual_seed(11)
        for _ in range(opts.ecdf_calib):
            imgs = [torch.randn(1, 3, h, w, generator=gc).to(device) for h, w in shapes]
            coarse = torch.randint(0, 13, ((opts.height + 31) // 32, (opts.width + 31) // 32), generator=gc)
            lab = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:opts.height, :opts.width].contiguous()
            yield imgs, lab.to(device)

    pooled = make_pooled(opts, (opts.out_label,))
    with use_calibrator(ecdf_calibrator(seg, opts, calib_frames, num_class)), use_pooled(pooled):
        r = evaluate(seg, frames(), 14, opts.ood, (opts.out_label,), opts.exclude_back, opts.open_set_thresholds)
    print("mean auroc = ", r["auroc"], "mean aupr = ", r["aupr"], " mean fpr = ", r["fpr"])          # :587-589
    if pooled is not None:
        print_pooled(r["pooled"], pooled, opts.pooled_curve)
    print("Mean IoU: %.4f, Accuracy: %.2f%%, Inference Time: %.4fs" % (r["seg"]["Mean IoU"], 100.0 * r["seg"]["Overall Acc"],
                                                                        r["sec_per_frame"]))
    if "open_set" in r:
        print_open_set(r["open_set"])


def run_dataset(seg, cfg, opts, num_class, device):
    """The reference's `main` + summary (eval_ood_traditional.py:520-560,563-600) on a StreetHazards-layout tree."""
    from datasets.streethazards import StreetHazardsReader
    reader = StreetHazardsReader(cfg["DATASET.root_dataset"], cfg["DATASET.list_val"],
                                 img_sizes=tuple(cfg["DATASET.imgSizes"]), img_max_size=cfg["DATASET.imgMaxSize"],
                                 padding_constant=cfg["DATASET.padding_constant"], workers=opts.workers or None,
                                 device=device)
    print("# samples: {}".format(len(reader)))

    def calib_frames():
        return StreetHazardsReader(cfg["DATASET.root_dataset"], cfg["DATASET.list_calib"],
                                   img_sizes=tuple(cfg["DATASET.imgSizes"]), img_max_size=cfg["DATASET.imgMaxSize"],
                                   padding_constant=cfg["DATASET.padding_constant"], workers=opts.workers or None, device=device,
                                   max_sample=opts.ecdf_calib if opts.ecdf_calib else -1)

    pooled = make_pooled(opts, (opts.out_label,))
    with use_calibrator(ecdf_calibrator(seg, opts, calib_frames, num_class)), use_pooled(pooled):
        tic = time.perf_counter()
        r = evaluate(seg, reader, num_class + 1, opts.ood, (opts.out_label,), opts.exclude_back, opts.open_set_thresholds)
        wall = time.perf_counter() - tic
    for i, iou in enumerate(r["known_iou"]):
        print("class [{}], IoU: {:.4f}".format(i, iou))
    print("[Eval Summary]:")
    print("Mean IoU: {:.4f}, Accuracy: {:.2f}%, Inference Time: {:.4f}s"
          .format(r["known_iou"].mean(), 100.0 * r["seg"]["Overall Acc"], r["sec_per_frame"]))
    print("mean auroc = ", r["auroc"], "mean aupr = ", r["aupr"], " mean fpr = ", r["fpr"])
    if pooled is not None:
        print_pooled(r["pooled"], pooled, opts.pooled_curve)
    print("Wall clock: {:.2f} frames/s ({} frames, {} decode workers); model only: {:.2f} frames/s"
          .format(len(reader) / wall, len(reader), reader.workers, 1.0 / r["sec_per_frame"]))
    if "open_set" in r:
        print_open_set(r["open_set"])
    print("Evaluation Done!")


if __name__ == "__main__":
    main()
