"""Teacher-student distillation driver: the recipe of the reference's main_distillation.py (:321-447) on the MI355X path,
in the style of main_self_distillation.py.  A frozen 16-class DMLNet `model_1` (the teacher, `--ckpt`) and a 17-class
`model_2` (the student, which takes over the checkpoint's keys outside `classifier`, :380-383) see the same batch; the
student trains under utils.CrossEntropyLoss_dis: CE / n plus `--dis_weight` times the feature-distillation term the
reference wrote behind an early `return` (utils/loss.py:104-117 there, coefficient 0.01; the default 0 is its live
behaviour).  What is reproduced:

  * optimizer: SGD on the student, backbone at 0.1 lr and classifier at lr (:335-338), PolyLR (:342);
  * labels: held-out class (train id 13, car) -> new id 16, ids above move down, composed into the crop kernel's label
    table as in main_self_distillation.py (the reference's `labels[labels == 0] = 16` at :423 is one of its mutually
    exclusive remaps);
  * `--pseudo_labels`: ignored pixels take the teacher's prediction (:428-430), inside the loss's forward launch;
  * the saved checkpoint is the student's, in the reference's keys (:357-363).

Not reproduced: the reference never calls model_1.eval(), so its teacher normalises with batch statistics and its running
statistics drift while it "teaches".  Here the teacher is frozen for good: eval(), requires_grad False, run under no_grad.
Data: `--synthetic` only, as main_embedding.py.  Without `--ckpt` the teacher is untrained: in eval() its features are orders of
magnitude from the student's, and `--dis_weight 0.01` then diverges within a few iterations -- such a run exercises
the path, it does not train.
"""
import argparse
import os
import time

import torch

import network
import utils
from datasets import Cityscapes
from dmlnet import parallel
from dmlnet.optim import FusedSGD


def get_argparser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="deeplabv3plus_embedding_resnet101", choices=["deeplabv3plus_embedding_resnet101"])
    p.add_argument("--num_classes", type=int, default=16, help="the teacher's; the student has one more")
    p.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    p.add_argument("--total_itrs", type=int, default=1000)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--batch_size", type=int, default=16, help="GLOBAL batch size, sharded over the ranks")
    p.add_argument("--crop_size", type=int, default=768)
    p.add_argument("--ckpt", default=None, help="checkpoint of the teacher")
    p.add_argument("--dis_weight", type=float, default=0.0,
                   help="weight of the feature-distillation term (0.01 is the coefficient of the reference's utils/loss.py:117)")
    p.add_argument("--pseudo_labels", action="store_true", help="ignored pixels take the teacher's prediction (:428-430)")
    p.add_argument("--save_dir", default="checkpoints")
    p.add_argument("--save_interval", type=int, default=0)
    p.add_argument("--print_interval", type=int, default=10)
    p.add_argument("--random_seed", type=int, default=1)
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--frame_height", type=int, default=1024)
    p.add_argument("--frame_width", type=int, default=2048)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "f16x2", "f32x3"],
                   help="bf16: bf16 storage (throughput mode); f32: exact fp32 MFMA (the reference's arithmetic); f16x2 / f32x3: fp32 tensors with the convolution products on the fp16 / bf16 matrix cores (fp32-accurate splits, bench.py's headline is f16x2)")
    return p


def main():
    opts = get_argparser().parse_args()
    if not opts.synthetic:
        raise SystemExit("only --synthetic data is available (datasets are outside the hot path)")
    rank, local, world = parallel.init_from_env()
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    torch.manual_seed(opts.random_seed)

    def make(num_classes):
        m = getattr(network, opts.model)(num_classes=num_classes, output_stride=opts.output_stride, pretrained_backbone=False)
        utils.set_bn_momentum(m.backbone, momentum=0.01)                           # :324, :329
        m.set_compute_dtype(torch.bfloat16 if opts.dtype == "bf16" else torch.float32,
                            fp32_products={"f32": "exact", "f32x3": "bf16x3", "f16x2": "f16x2"}.get(opts.dtype))
        return m

    model_1, model_2 = make(opts.num_classes), make(opts.num_classes + 1)          # :321, :326
    for p in model_1.parameters():
        p.requires_grad_(False)
    optimizer = FusedSGD([{"params": model_2.backbone.parameters(), "lr": 0.1 * opts.lr},
                          {"params": model_2.classifier.parameters(), "lr": opts.lr}],
                         lr=opts.lr, momentum=0.9, weight_decay=opts.weight_decay).bind(model_2)  # :335-338
    scheduler = utils.PolyLR(optimizer, opts.total_itrs, power=0.9)                # :342
    criterion = utils.CrossEntropyLoss_dis(ignore_index=255, alpha=0, beta=0, gamma=0, dis_weight=opts.dis_weight,
                                           novel_id=opts.num_classes, sync=True if world > 1 else None)   # :351

    cur_itrs = 0
    if opts.ckpt and os.path.isfile(opts.ckpt):                                    # :371-383
        ck = torch.load(opts.ckpt, map_location="cpu")
        model_1.load_state_dict(ck["model_state"])
        own = model_2.state_dict()
        own.update({k: v for k, v in ck["model_state"].items() if k in own and "classifier" not in k})
        model_2.load_state_dict(own)
    model_1.to(device).eval()
    model_2.to(device)
    if world > 1:
        model_2._engine.store.bind(device)
        model_2._engine.reducer = parallel.GradReducer(model_2._engine.store, bucket_mb=32.0, average=False)

    from utils import ext_transforms as et
    lo, hi = parallel.shard_range(opts.batch_size, rank, world)
    g = torch.Generator().manual_seed(1234 + rank)
    fh, fw = max(opts.crop_size, opts.frame_height), max(opts.crop_size, opts.frame_width)
    frames = torch.randint(0, 256, (hi - lo, fh, fw, 3), generator=g, dtype=torch.uint8).to(device)
    coarse = torch.randint(0, 34, (hi - lo, (fh + 63) // 64, (fw + 63) // 64), generator=g, dtype=torch.uint8)
    frame_labels = coarse.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :fh, :fw].contiguous().to(device)
    # raw id -> 17-id space of the shipped dataset (truck, bus unknown) -> car (13) becomes the novel class
    lut, lut_true = Cityscapes.label_luts([14, 15])
    lut = Cityscapes.eval_relabel_lut(held_out=13, new_id=opts.num_classes)[lut]
    transform = et.ExtCompose([
        et.ExtRandomCrop(size=(opts.crop_size, opts.crop_size)),
        et.ExtColorJitter(brightness=0.5, contrast=0.5, saturation=0.5),
        et.ExtRandomHorizontalFlip(),
        et.ExtToTensor(),
        et.ExtNormalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
    ], label_luts=(lut, lut_true))

    interval_loss, t0 = None, time.perf_counter()
    while cur_itrs < opts.total_itrs:
        model_2.train()                                                            # :416
        cur_itrs += 1
        images, labels, _ = transform(frames, frame_labels)
        optimizer.zero_grad()
        with torch.no_grad():
            outputs_1, _, features_1 = model_1(images)                             # :427
        outputs, centers, features_2 = model_2(images)                             # :429
        loss = criterion(outputs, labels, features_1, features_2,
                         teacher_logits=outputs_1 if opts.pseudo_labels else None)  # :428, :430, :434
        loss.backward()
        optimizer.step()
        scheduler.step()
        interval_loss = loss.detach() if interval_loss is None else interval_loss + loss.detach()
        if cur_itrs % opts.print_interval == 0:
            mean_loss = float(interval_loss) / opts.print_interval       # the D2H copy waits for the interval's kernels
            dt = time.perf_counter() - t0
            if rank == 0:
                print("Itrs %d/%d, Loss=%f, %.1f img/s" % (cur_itrs, opts.total_itrs, mean_loss,
                                                           opts.batch_size * opts.print_interval / dt))
            interval_loss, t0 = None, time.perf_counter()
        if opts.save_interval and cur_itrs % opts.save_interval == 0 and rank == 0:
            utils.mkdir(opts.save_dir)
            torch.save({"cur_itrs": cur_itrs, "model_state": model_2.state_dict(), "optimizer_state": optimizer.state_dict(),
                        "scheduler_state": scheduler.state_dict(), "best_score": 0.0},
                       os.path.join(opts.save_dir, "latest_%s_synthetic_os%d.pth" % (opts.model, opts.output_stride)))


if __name__ == "__main__":
    main()
