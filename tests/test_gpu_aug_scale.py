"""GPU: the scale / resize / pad / centre-crop transforms on the device (dml_aug_scale_window + the jitter kernels) bit-equal
to the reference's fixtures (g16) and to the CPU restatement (tests/scale_ref.py); the --scale_range path of the driver."""
import glob
import json
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import pil_resample as PR
import scale_ref as SR
from oracle import transforms_ref as TR

G16 = sorted(glob.glob(os.path.join(H.GOLDEN, "g16_scale_*.npz")))
IDS = [os.path.basename(p)[10:-4] for p in G16]
MEAN, STD = PR.MEAN, PR.STD
pytestmark = pytest.mark.gpu


def _et():
    import utils
    return utils.ext_transforms


@pytest.mark.parametrize("path", G16, ids=IDS)
def test_device_pipeline_matches_reference_fixture(path):
    """tolerance zero: integer arithmetic up to the fp32 normalisation"""
    g = np.load(path)
    tf = SR.build(_et(), json.loads(str(g["spec"])))
    random.seed(int(g["seed"]))
    img, lbl = tf(torch.from_numpy(g["img"]).cuda(), torch.from_numpy(g["lbl"]).cuda())
    torch.cuda.synchronize()
    assert img.dtype == torch.float32 and lbl.dtype == torch.int64
    assert np.array_equal(img.cpu().numpy(), g["out_img"])
    assert np.array_equal(lbl.cpu().numpy(), g["out_lbl"].astype(np.int64))


def test_device_pipeline_raw_ids_through_label_tables():
    """the padded label 0 is a raw id and goes through the table like any other pixel"""
    from datasets import Cityscapes
    from oracle import cityscapes_ref as CR
    g = np.load(G16[IDS.index("raw_ids")])
    tf = SR.build(_et(), json.loads(str(g["spec"])), label_luts=Cityscapes.label_luts([13, 14, 15]))
    random.seed(int(g["seed"]))
    img, lbl, lbl_true = tf(torch.from_numpy(g["img"]).cuda(), torch.from_numpy(g["lbl"]).cuda())
    torch.cuda.synchronize()
    assert (g["out_lbl"] == 0).any()
    want, want_true = CR.encode_target(g["out_lbl"], [13, 14, 15])
    assert np.array_equal(img.cpu().numpy(), g["out_img"])
    assert np.array_equal(lbl.cpu().numpy(), want) and np.array_equal(lbl_true.cpu().numpy(), want_true)


def _reference_batch(img, lbl, params, out):
    ri, rl = [], []
    for b, p in enumerate(params):
        wi, wl = SR.window(img[b], lbl[b], p["size"], p["oy"], p["ox"], out)
        a, c = TR.apply(wi, wl, {"i": 0, "j": 0, "ops": p["ops"], "flip": p["flip"]}, out, MEAN, STD)
        ri.append(a)
        rl.append(c)
    return np.stack(ri), np.stack(rl)


def test_device_batch_with_forced_parameters_vs_restatement():
    """one launch: a different scale per sample, scale 1, target size == crop size, a window over each of the four edges, two
    column segments (261 = 256 + 5), odd sizes; with / without labels, with / without label tables, a single 3-D frame"""
    et = _et()
    rs = np.random.RandomState(9)
    B, Hh, Ww, out = 7, 75, 301, (37, 261)
    base = rs.randint(0, 256, (B, (Hh + 3) // 4, (Ww + 3) // 4, 3)).astype(np.uint8)
    img = np.ascontiguousarray(np.repeat(np.repeat(base, 4, 1), 4, 2)[:, :Hh, :Ww]) ^ rs.randint(0, 16, (B, Hh, Ww, 3)).astype(np.uint8)
    img = np.ascontiguousarray(img)
    lbl = rs.randint(0, 34, (B, Hh, Ww)).astype(np.uint8)

    def P(size, oy, ox, ops=(), flip=False):
        return {"i": 0, "j": 0, "size": size, "oy": oy, "ox": ox, "out": out, "ops": list(ops), "flip": flip}
    params = [
        P((75, 301), 19, 20),                                   # scale exactly 1: both passes are the identity
        P((37, 261), 0, 0, [(1, 1.5)], True),                   # the target size equals the crop size
        P((150, 602), -9, 100, [(2, 0.5), (0, 1.5), (1, 0.5)]),  # scale 2, over the top edge
        P((150, 602), 130, 341, [(0, 0.73)], True),             # over the bottom edge (341 + 261 = 602: flush right)
        P((37, 150), 0, -60, [(1, 0.0), (2, 1.4999)]),           # scale 0.5: over the left AND the right edge
        P((113, 452), 90, 300, [(0, 1.0), (1, 1.0), (2, 1.0)], True),   # scale 1.5, over the bottom and right edges
        P((53, 301), -5, 0, [(1, 1.27)]),                        # the height alone changes, over the top edge
    ]
    tf = et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(out, pad_if_needed=True),
                        et.ExtColorJitter(0.5, 0.5, 0.5), et.ExtRandomHorizontalFlip(), et.ExtToTensor(),
                        et.ExtNormalize(MEAN, STD)])
    ri, rl = _reference_batch(img, lbl, params, out)
    dimg, dlbl = torch.from_numpy(img).cuda(), torch.from_numpy(lbl).cuda()
    oi, ol = tf(dimg, dlbl, params=params)
    torch.cuda.synchronize()
    for b in range(B):
        assert np.array_equal(oi[b].cpu().numpy(), ri[b]), "image %d" % b
        assert np.array_equal(ol[b].cpu().numpy(), rl[b].astype(np.int64)), "label %d" % b
    # without labels
    oi2, ol2 = tf(dimg, None, params=params)
    assert ol2 is None and torch.equal(oi2, oi)
    # with label tables
    from datasets import Cityscapes
    from oracle import cityscapes_ref as CR
    tfl = et.ExtCompose(tf.transforms, label_luts=Cityscapes.label_luts([13, 14, 15]))
    oi3, ol3, ot3 = tfl(dimg, dlbl, params=params)
    want, want_true = CR.encode_target(rl, [13, 14, 15])
    assert torch.equal(oi3, oi) and np.array_equal(ol3.cpu().numpy(), want) and np.array_equal(ot3.cpu().numpy(), want_true)
    # a single 3-D frame
    oi4, ol4 = tf(dimg[4], dlbl[4], params=[params[4]])
    assert oi4.shape == (3,) + out and torch.equal(oi4, oi[4]) and torch.equal(ol4, ol[4])
    # a window width that is not a multiple of four (byte stores, a ragged second column tile); a contrast op over a zero border
    out = (23, 67)
    odd = [P((75, 301), 3, 7), P((40, 160), -2, 100, [(1, 0.8)], True)]
    for p in odd:
        p["out"] = out
    oi5, ol5 = tf(dimg[:2], dlbl[:2], params=odd)
    ri5, rl5 = _reference_batch(img[:2], lbl[:2], odd, out)
    assert np.array_equal(oi5.cpu().numpy(), ri5)
    assert np.array_equal(ol5.cpu().numpy(), rl5.astype(np.int64))


def test_device_random_train_block_at_cityscapes_size():
    """1024 x 2048 frames, ExtRandomScale((0.5, 2)) + 768 crop with pad_if_needed, sampled: against the restatement"""
    et = _et()
    rs = np.random.RandomState(7)
    B, Hh, Ww, out = 4, 1024, 2048, (768, 768)
    base = rs.randint(0, 256, (B, Hh // 8, Ww // 8, 3)).astype(np.uint8)
    img = np.ascontiguousarray(np.repeat(np.repeat(base, 8, axis=1), 8, axis=2))
    img ^= rs.randint(0, 8, (B, Hh, Ww, 3)).astype(np.uint8)
    lbl = np.ascontiguousarray(np.repeat(np.repeat(rs.randint(0, 19, (B, Hh // 64, Ww // 64)).astype(np.uint8), 64, 1), 64, 2))
    tf = et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(out, pad_if_needed=True),
                        et.ExtColorJitter(0.5, 0.5, 0.5), et.ExtRandomHorizontalFlip(), et.ExtToTensor(),
                        et.ExtNormalize(MEAN, STD)])
    random.seed(2)
    params, size = tf.sample(B, Hh, Ww)
    params[0].update(size=(512, 1024), oy=-128, ox=100)          # scale 0.5: padded above and below
    oi, ol = tf(torch.from_numpy(img).cuda(), torch.from_numpy(lbl).cuda(), params=params)
    torch.cuda.synchronize()
    ri, rl = _reference_batch(img, lbl, params, out)
    assert size == out and np.array_equal(oi.cpu().numpy(), ri) and np.array_equal(ol.cpu().numpy(), rl.astype(np.int64))


def test_driver_scale_range_runs():
    """main_embedding.py --synthetic --scale_range: exit status 0 and finite losses (nothing about their trend)"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([H.ROOT, H.PKG]))
    cmd = [sys.executable, os.path.join(H.PKG, "main_embedding.py"), "--synthetic", "--scale_range", "0.5", "2.0",
           "--crop_size", "128", "--frame_height", "160", "--frame_width", "256", "--batch_size", "4", "--total_itrs", "6",
           "--print_interval", "1", "--num_classes", "16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=H.PKG)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"[Ll]oss[=: ]+([-+0-9.eEnaNifI]+)", r.stdout)]
    assert len(losses) >= 3, r.stdout[-2000:]
    assert all(math.isfinite(v) for v in losses), losses
