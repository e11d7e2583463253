#!/usr/bin/env python3
"""Evaluation of the incremental few-shot model (test_self_distillation.py:225-420 of the reference, `validate`) on the
MI355X path: the merged prediction of the base head and the `--novel_cls` incremental heads in one fused pass
(model.predict: no full-resolution logits exist), the ground truth relabelled on the device with the reference's table
(:351-354: the held-out class 13 -> 16, every id above moves down, 254 -> 255; the 16+2 / 16+3 tables it keeps commented out
at :356-370 for --novel_cls 2 / 3) and the confusion matrix kept on the device.

    python test_self_distillation.py --synthetic --height 1024 --width 2048 --num_images 4 --novel_cls 1 --test_only \\
        [--ckpt X.pth] [--save_val_results]

The reference's flags that mean something here: --model --num_classes --output_stride --ckpt --novel_cls --test_only
--save_val_results --gpu_id --batch_size (images per predict call).  Input as in test_embedding.py / eval_open_world.py of
this package: --synthetic --height --width --num_images --dtype.  Accepted and ignored, so that the reference's command
lines parse: --data_root --dataset --separable_conv --total_itrs --lr --lr_policy --step_size --crop_val --val_batch_size
--crop_size --continue_training --loss_type --weight_decay --random_seed --print_interval --val_interval --download --year
--enable_vis --vis_port --vis_env --vis_num_samples.

--save_val_results writes results/<n>_pred.png and results/<n>_target.png (Cityscapes.decode_target on the device, one
copy to the host per image); the reference's matplotlib overlay is left out.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import network  # noqa: E402
from datasets import Cityscapes  # noqa: E402

HELD_OUT = (13, 14, 15)      # the classes the incremental heads learn, in the order of the heads (README of the reference)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="deeplabv3plus_embedding_self_distillation_resnet101")
    p.add_argument("--num_classes", type=int, default=16)
    p.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    p.add_argument("--ckpt", default=None)
    p.add_argument("--novel_cls", type=int, default=1, help="number of incremental heads merged into the prediction")
    p.add_argument("--test_only", action="store_true", help="the only mode of this driver (training: main_self_distillation.py)")
    p.add_argument("--save_val_results", action="store_true", help='write the predictions and targets to "./results"')
    p.add_argument("--gpu_id", default="0")
    p.add_argument("--batch_size", type=int, default=1, help="images per predict call")
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=2048)
    p.add_argument("--num_images", type=int, default=4)
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"],
                   help="bf16: bf16 storage (throughput mode); f32: exact fp32 MFMA (the reference's arithmetic); f16x2 / f32x3: fp32 tensors with the convolution products on the fp16 / bf16 matrix cores")
    # the reference's parser, for its command lines; none of these changes anything here
    for flag, kw in (("--data_root", {}), ("--dataset", {}), ("--total_itrs", {}), ("--lr", {}), ("--lr_policy", {}),
                     ("--step_size", {}), ("--val_batch_size", {}), ("--crop_size", {}), ("--loss_type", {}),
                     ("--weight_decay", {}), ("--random_seed", {}), ("--print_interval", {}), ("--val_interval", {}),
                     ("--year", {}), ("--vis_port", {}), ("--vis_env", {}), ("--vis_num_samples", {})):
        p.add_argument(flag, default=None, help=argparse.SUPPRESS, **kw)
    for flag in ("--separable_conv", "--crop_val", "--continue_training", "--download", "--enable_vis"):
        p.add_argument(flag, action="store_true", help=argparse.SUPPRESS)
    return p


def synthetic_batch(first, count, height, width, n_ids, device):
    """Seeded frames and blocky ground truth in the id space the dataset hands the reference's validate(): n_ids train ids
    (the held-out classes still at 13, ...), with one block in sixteen unlabelled (255)."""
    imgs, labs = [], []
    for i in range(first, first + count):
        g = torch.Generator().manual_seed(4321 + i)
        imgs.append(torch.randn(3, height, width, generator=g))
        coarse = torch.randint(0, n_ids, ((height + 63) // 64, (width + 63) // 64), generator=g)
        coarse[torch.rand(coarse.shape, generator=g) < 1.0 / 16] = 255
        labs.append(coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:height, :width])
    return torch.stack(imgs).to(device), torch.stack(labs).contiguous().to(device)


def build_model(o):
    if o.novel_cls == 1 or "self_distillation" not in o.model:
        return getattr(network, o.model)(num_classes=o.num_classes, output_stride=o.output_stride, pretrained_backbone=False)
    # a 16+2 / 16+3 checkpoint: the factory's signature is the reference's (one incremental head); the class takes the count
    from network import modeling
    return modeling._segm_resnet("deeplabv3plus_embedding_self_distillation", "resnet101", o.num_classes, o.output_stride,
                                 False, cls_novel=o.novel_cls)


def main(argv=None):
    o = build_parser().parse_args(argv)
    if not o.synthetic:
        raise SystemExit("only --synthetic data is available (datasets are outside the hot path)")
    if not 0 <= o.novel_cls <= len(HELD_OUT):
        raise SystemExit("--novel_cls must be 0 .. %d" % len(HELD_OUT))
    dev = torch.device("cuda", int(str(o.gpu_id).split(",")[0]))
    torch.cuda.set_device(dev)
    torch.manual_seed(1)
    model = build_model(o)
    if o.ckpt:
        model.load_state_dict(torch.load(o.ckpt, map_location="cpu")["model_state"])
    model.to(dev).eval()
    model.set_compute_dtype(torch.bfloat16 if o.dtype == "bf16" else torch.float32,
                            fp32_products={"f32": "exact", "f32x3": "bf16x3", "f16x2": "f16x2"}.get(o.dtype))
    multi = hasattr(model, "classifier_list")
    n_novel = o.novel_cls if multi else 0
    base = model.base_classes if multi else o.num_classes
    n_eval = base + n_novel
    import metrics as metrics_mod
    seg_metrics = metrics_mod.StreamSegMetrics(n_eval)
    lut = None
    if n_novel:
        lut = torch.from_numpy(Cityscapes.eval_relabel_lut(list(HELD_OUT[:n_novel]), [base + j for j in range(n_novel)])
                               .astype(np.int64)).to(dev)
    if o.save_val_results:
        os.makedirs("results", exist_ok=True)
        from PIL import Image
    img_id = 0
    with torch.no_grad():
        for first in range(0, o.num_images, o.batch_size):
            images, labels = synthetic_batch(first, min(o.batch_size, o.num_images - first), o.height, o.width, n_eval, dev)
            preds = model.predict(images, novel_cls=n_novel) if multi else model.predict(images)       # :292-297
            targets = lut[labels] if lut is not None else labels                                       # :351-354
            seg_metrics.update(targets, preds)                                                          # :378
            if o.save_val_results:                                                                      # :384-392
                for k in range(images.shape[0]):
                    both = torch.stack([Cityscapes.decode_target(targets[k]), Cityscapes.decode_target(preds[k])])
                    both = both.to(torch.uint8).cpu().numpy()                                           # one copy per image
                    Image.fromarray(both[0]).save("results/%d_target.png" % img_id)
                    Image.fromarray(both[1]).save("results/%d_pred.png" % img_id)
                    img_id += 1
    torch.cuda.synchronize()
    print(seg_metrics.to_str(seg_metrics.get_results()))


if __name__ == "__main__":
    main()
