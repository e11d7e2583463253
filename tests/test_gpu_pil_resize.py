"""GPU: the evaluation input of the anomaly driver on the device -- dml_pil_resize_normalize bit-equal to the
reference's ValDataset fixture (g15) and to live Pillow + the reference transform, dml_segm_to_label, the StreetHazards
reader feeding `evaluate` exactly as CPU-prepared frames do, and the driver's real-data run from a config file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import pil_resample as P

pytestmark = pytest.mark.gpu


def _bits_equal(dev, ref):
    a = dev.detach().cpu().numpy()
    b = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_kernel_bit_equal_to_reference_fixture():
    import utils
    g = np.load(os.path.join(H.GOLDEN, "g15_streethazards.npz"))
    sizes = tuple(int(s) for s in g["img_sizes"])
    for i in range(int(g["n_frames"])):
        img, segm = g["img_%d" % i], g["segm_%d" % i]
        shapes = P.resized_shapes(*img.shape[:2], sizes, int(g["img_max_size"]), int(g["padding_constant"]))
        outs = utils.pil_resize_normalize(torch.from_numpy(img).cuda(), shapes)
        for k, o in enumerate(outs):
            assert _bits_equal(o[0], g["out_%d_%d" % (i, k)]), (i, k)
        lab = utils.segm_to_label(torch.from_numpy(segm).cuda())
        assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), g["seg_label_%d" % i])


def _pillow_inputs(img, shapes):
    Image = pytest.importorskip("PIL.Image")
    pil = Image.fromarray(img)
    return [P.img_transform(pil.resize((w, h), Image.BILINEAR)) for h, w in shapes]


def test_kernel_bit_equal_to_pillow_streethazards_sizes():
    import utils
    rs = np.random.RandomState(720)
    yy, xx = np.mgrid[0:720, 0:1280]
    img = np.clip(np.stack([(yy + xx) % 256, (3 * xx) % 256, (yy * 2) % 256], -1) + rs.randint(-40, 41, (720, 1280, 3)),
                  0, 255).astype(np.uint8)
    shapes = P.resized_shapes(720, 1280)
    refs = _pillow_inputs(img, shapes)
    outs = utils.pil_resize_normalize(torch.from_numpy(img).cuda(), shapes)
    torch.cuda.synchronize()
    for s, o, r in zip(shapes, outs, refs):
        assert tuple(o.shape) == (1, 3) + s and _bits_equal(o[0], r), s


def test_kernel_bit_equal_to_pillow_random_sizes():
    import utils
    rs = np.random.RandomState(15)
    for trial in range(24):
        h, w = (int(v) for v in rs.randint(1, 90, 2))
        img = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        shapes = []
        for k in range(int(rs.randint(1, 9))):                 # up to 8 scales in one launch
            kind = (trial + k) % 4
            if kind == 0:
                shapes.append((int(rs.randint(1, 4)), int(rs.randint(1, 4))))          # 1..3-pixel outputs
            elif kind == 1:
                shapes.append((h * 8, w * int(rs.randint(1, 9))))                     # up to x8
            elif kind == 2:
                shapes.append((max(1, h // 6), max(1, w // int(rs.randint(1, 7)))))   # down to /6
            else:
                shapes.append((int(rs.randint(1, 200)), int(rs.randint(1, 200))))
        frame = torch.from_numpy(img).cuda()
        outs = utils.pil_resize_normalize(frame, shapes)
        refs = _pillow_inputs(img, shapes)
        for s, o, r in zip(shapes, outs, refs):
            assert _bits_equal(o[0], r), (trial, (h, w), s)
    # an output view that is not 16-byte aligned is written with scalar stores, same values
    img = rs.randint(0, 256, (50, 70, 3), dtype=np.uint8)
    a = utils.pil_resize_normalize(torch.from_numpy(img).cuda(), [(33, 48)])[0]
    assert _bits_equal(a[0], _pillow_inputs(img, [(33, 48)])[0])


def test_segm_to_label():
    import utils
    segm = torch.arange(256, dtype=torch.uint8).repeat(7, 3)
    lab = utils.segm_to_label(segm.cuda())
    assert lab.dtype == torch.int64 and lab.shape == segm.shape
    assert torch.equal(lab.cpu(), segm.long() - 1)
    assert utils.segm_to_label(torch.zeros((0, 5), dtype=torch.uint8, device="cuda")).numel() == 0
    with pytest.raises(TypeError):
        utils.segm_to_label(segm)


def _write_tree(root, frames, seed):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(seed)
    recs, data = [], []
    os.makedirs(os.path.join(root, "images", "test", "t5"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations", "test", "t5"), exist_ok=True)
    for i, (h, w) in enumerate(frames):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.clip(np.stack([(yy * 3 + xx) % 256, (xx * 5) % 256, (yy * 7) % 256], -1) + rs.randint(-50, 51, (h, w, 3)),
                      0, 255).astype(np.uint8)
        coarse = rs.randint(1, 15, ((h + 15) // 16, (w + 15) // 16))              # 1..14 -> labels 0..13 (13: anomaly)
        segm = coarse.repeat(16, 0).repeat(16, 1)[:h, :w].astype(np.uint8)
        segm[:2, :3] = 0                                                          # a few unlabeled pixels (-1)
        fi, fs = "images/test/t5/%d.png" % i, "annotations/test/t5/%d.png" % i
        Image.fromarray(img).save(os.path.join(root, fi))
        Image.fromarray(segm, mode="L").save(os.path.join(root, fs))
        recs.append({"fpath_img": fi, "fpath_segm": fs, "height": h, "width": w, "dbName": "StreetHazards"})
        data.append((img, segm))
    odgt = os.path.join(root, "test.odgt")
    with open(odgt, "w") as f:
        f.write(json.dumps(recs) + "\n")
    return odgt, data


def _model(enc_w="", dec_w="", dtype="bf16"):
    import models
    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights=enc_w)
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, weights=dec_w,
                                            use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).cuda().eval()
    seg.set_compute_dtype(torch.bfloat16 if dtype == "bf16" else torch.float32,
                          fp32_products={"f32": "exact"}.get(dtype))
    return seg


def _cpu_frames(data, sizes, max_size):
    for img, segm in data:
        shapes = P.resized_shapes(*img.shape[:2], sizes, max_size, 8)
        imgs, lab = P.eval_inputs(img, segm, shapes)
        yield [t.cuda() for t in imgs], lab.cuda()


def _same_results(a, b):
    for k in ("auroc", "aupr", "fpr"):
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k
    for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
        np.testing.assert_array_equal(a["seg"][k], b["seg"][k])
    np.testing.assert_array_equal(np.array(list(a["seg"]["Class IoU"].values())),
                                  np.array(list(b["seg"]["Class IoU"].values())))
    np.testing.assert_array_equal(a["known_iou"], b["known_iou"])


def test_reader_feeds_evaluate_exactly_as_cpu_prepared_frames(tmp_path):
    import eval_ood_traditional as E
    from datasets.streethazards import StreetHazardsReader
    sizes, max_size = (48, 64, 80), 160
    odgt, data = _write_tree(str(tmp_path), [(72, 128), (65, 97), (72, 128), (80, 80), (72, 128)], seed=3)
    seg = _model(dtype="f32")
    reader = StreetHazardsReader(str(tmp_path), odgt, img_sizes=sizes, img_max_size=max_size, workers=2)
    # the reader's tensors themselves
    for (imgs, lab), (img, segm) in zip(reader, data):
        ref_imgs, ref_lab = P.eval_inputs(img, segm, P.resized_shapes(*img.shape[:2], sizes, max_size, 8))
        assert len(imgs) == len(ref_imgs) and all(_bits_equal(a[0], b[0]) for a, b in zip(imgs, ref_imgs))
        assert torch.equal(lab.cpu(), ref_lab)
    assert len(reader.decode_seconds) == len(data)
    r_dev = E.evaluate(seg, reader, 14, "dissum", (13,))
    r_cpu = E.evaluate(seg, _cpu_frames(data, sizes, max_size), 14, "dissum", (13,))
    _same_results(r_dev, r_cpu)
    assert not np.isnan(r_dev["auroc"]) and r_dev["known_iou"].shape == (13,)


def test_driver_real_data_run_from_config(tmp_path):
    import eval_ood_traditional as E
    import models
    sizes, max_size = (48, 64), 120
    root = tmp_path / "streethazards"
    odgt, data = _write_tree(str(root), [(72, 128), (72, 128), (61, 90)], seed=4)
    ck = tmp_path / "ckpt"
    ck.mkdir()
    torch.manual_seed(11)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048)
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, use_softmax=True)
    torch.save(enc.state_dict(), str(ck / "encoder_epoch_t.pth"))
    torch.save(dec.state_dict(), str(ck / "decoder_epoch_t.pth"))
    del enc, dec
    cfg = tmp_path / "street.yaml"
    cfg.write_text('DATASET:\n  root_dataset: "nowhere"\n  list_val: "nowhere.odgt"\n  num_class: 13\n'
                   '  imgSizes: (300, 375)\n  imgMaxSize: 1000\n  padding_constant: 8\n'
                   'MODEL:\n  arch_encoder: "resnet50dilated"\n  fc_dim: 2048\nVAL:\n  checkpoint: "epoch_t.pth"\n'
                   'DIR: "nowhere"\n')
    cmd = [sys.executable, "eval_ood_traditional.py", "--cfg", str(cfg), "--gpu", "0", "--ood", "dissum",
           "DATASET.root_dataset", str(root), "DATASET.list_val", odgt, "DIR", str(ck),
           "DATASET.imgSizes", "(48, 64)", "DATASET.imgMaxSize", str(max_size)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=H.PKG, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    seg = _model(str(ck / "encoder_epoch_t.pth"), str(ck / "decoder_epoch_t.pth"))
    ref = E.evaluate(seg, _cpu_frames(data, sizes, max_size), 14, "dissum", (13,))
    for i, iou in enumerate(ref["known_iou"]):
        assert "class [{}], IoU: {:.4f}".format(i, iou) in lines
    assert "[Eval Summary]:" in lines
    summ = [ln for ln in lines if ln.startswith("Mean IoU: ")]
    assert len(summ) == 1 and summ[0].startswith("Mean IoU: {:.4f}, Accuracy: {:.2f}%, Inference Time: ".format(
        ref["known_iou"].mean(), 100.0 * ref["seg"]["Overall Acc"]))
    oods = [ln for ln in lines if ln.startswith("mean auroc = ")]
    assert len(oods) == 1
    f = oods[0].split()
    assert float(f[3]) == ref["auroc"] and float(f[7]) == ref["aupr"] and float(f[11]) == ref["fpr"], oods[0]
    assert any(ln.startswith("Wall clock: ") for ln in lines)
