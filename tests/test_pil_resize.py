"""CPU: the numpy restatement of Pillow's BILINEAR resampler (tests/pil_resample.py) against live Pillow and the
reference's ValDataset fixture (g15), the product's host coefficient tables (utils/image_resize.py) against the
restatement, and the StreetHazards list parsing / target sizes (datasets/streethazards.py).  No kernels run here."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import pil_resample as P


def _size_pairs(n, seed):
    rs = np.random.RandomState(seed)
    pairs = []
    for k in range(n):
        src = int(rs.randint(1, 97))
        kind = k % 5
        if kind == 0:
            dst = 1                                          # 1-pixel outputs
        elif kind == 1:
            dst = src * 8                                    # x8 upscales
        elif kind == 2:
            dst = max(1, src // 6)                           # x6 downscales
            src = dst * 6 + int(rs.randint(0, 6))
        else:
            dst = int(rs.randint(1, 129))
        pairs.append((src, dst))
    return pairs


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(1)
    hs, ws = _size_pairs(300, 2), _size_pairs(300, 3)
    for k, ((h, H_), (w, W_)) in enumerate(zip(hs, ws)):
        if k % 3 == 0:
            a = rs.randint(0, 256, (h, w), dtype=np.uint8)                      # 'L' (the annotation mode)
        else:
            a = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((W_, H_), Image.BILINEAR))
        got = P.resize(a, (H_, W_))
        assert got.shape == ref.shape and np.array_equal(got, ref), (h, w, H_, W_)


def test_restatement_equals_live_pillow_streethazards_sizes():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(4)
    a = rs.randint(0, 256, (720, 1280, 3), dtype=np.uint8)
    for s in P.resized_shapes(720, 1280):
        ref = np.asarray(Image.fromarray(a).resize((s[1], s[0]), Image.BILINEAR))
        assert np.array_equal(P.resize(a, s), ref), s


def test_restatement_reproduces_reference_fixture():
    g = np.load(os.path.join(H.GOLDEN, "g15_streethazards.npz"))
    sizes = tuple(int(s) for s in g["img_sizes"])
    for i in range(int(g["n_frames"])):
        img, segm = g["img_%d" % i], g["segm_%d" % i]
        shapes = P.resized_shapes(*img.shape[:2], sizes, int(g["img_max_size"]), int(g["padding_constant"]))
        imgs, lab = P.eval_inputs(img, segm, shapes)
        for k, t in enumerate(imgs):
            ref = g["out_%d_%d" % (i, k)]
            assert t[0].numpy().shape == ref.shape
            assert np.array_equal(t[0].numpy().view(np.uint32), ref.view(np.uint32)), (i, k)
        assert lab.dtype == torch.int64 and np.array_equal(lab.numpy(), g["seg_label_%d" % i])
    # the fixture covers both directions
    ups = downs = 0
    for i in range(int(g["n_frames"])):
        h = g["img_%d" % i].shape[0]
        k = 0
        while "out_%d_%d" % (i, k) in g.files:
            H_ = g["out_%d_%d" % (i, k)].shape[1]
            ups, downs, k = ups + (H_ > h), downs + (H_ < h), k + 1
    assert ups > 0 and downs > 0


def test_product_tables_equal_restatement():
    from utils.image_resize import resample_coeffs
    pairs = _size_pairs(200, 5) + [(720, s) for s in (304, 376, 456, 528, 568)] + \
        [(1280, s) for s in (536, 672, 800, 936, 1000)] + [(1, 1), (1, 9), (9, 1), (720, 720)]
    for src, dst in pairs:
        b, k = resample_coeffs(src, dst)
        rb, rk = P.coeffs(src, dst)
        assert b.dtype == np.int32 and k.dtype == np.int32
        assert np.array_equal(b, rb) and np.array_equal(k, rk), (src, dst)
        assert k.shape[1] == 2 * int(np.ceil(max(src / dst, 1.0))) + 1


def test_band_rows_fit_the_workgroup():
    from utils.image_resize import _band_rows, resample_coeffs
    for src, dst in [(720, 304), (720, 568), (37, 296), (600, 100), (255, 1)]:
        vb, _ = resample_coeffs(src, dst)
        band, rows = _band_rows(vb)
        for y0 in range(0, dst, band):
            y1 = min(y0 + band, dst) - 1
            assert vb[y1, 0] + vb[y1, 1] - vb[y0, 0] <= rows <= 256
    with pytest.raises(ValueError):
        _band_rows(resample_coeffs(600, 1)[0])


def test_odgt_parsing_matches_reference(tmp_path):
    from datasets.streethazards import parse_odgt
    recs = [{"fpath_img": "images/test/t5/%d.png" % i, "fpath_segm": "annotations/test/t5/%d.png" % i,
             "height": 720, "width": 1280, "dbName": "StreetHazards"} for i in range(5)]
    p = tmp_path / "test.odgt"
    # the first line is one JSON list; later lines are ignored, as json.loads(...)[0] in the reference does
    p.write_text(json.dumps(recs) + "\n" + json.dumps(recs[:1]) + "\n")
    assert parse_odgt(str(p)) == recs
    assert parse_odgt(str(p), max_sample=2) == recs[:2]
    assert parse_odgt(str(p), start_idx=1, end_idx=3) == recs[1:3]
    assert parse_odgt(recs) == recs
    empty = tmp_path / "empty.odgt"
    empty.write_text("[]\n")
    with pytest.raises(AssertionError):
        parse_odgt(str(empty))


def test_resized_shapes_streethazards():
    from datasets.streethazards import resized_shapes
    import eval_ood_traditional as E
    want = [(304, 536), (376, 672), (456, 800), (528, 936), (568, 1000)]
    assert resized_shapes(720, 1280) == want
    assert E.resized_shapes(720, 1280) == want
    assert P.resized_shapes(720, 1280) == want
    for h, w in [(37, 53), (1024, 2048), (600, 400)]:
        assert resized_shapes(h, w) == P.resized_shapes(h, w)


def test_driver_config_merge(tmp_path):
    import eval_ood_traditional as E
    y = tmp_path / "c.yaml"
    y.write_text('DATASET:\n  root_dataset: "a"\n  imgSizes: (20, 30)\n  num_class: 13\nMODEL:\n  fc_dim: 2048\n'
                 'VAL:\n  checkpoint: "epoch_1.pth"\nDIR: "./ck"\n')
    cfg = E.load_cfg(str(y), ["DATASET.imgMaxSize", "90", "DIR", "elsewhere"])
    assert cfg["DATASET.root_dataset"] == "a" and cfg["DATASET.imgSizes"] == (20, 30)
    assert cfg["DATASET.imgMaxSize"] == 90 and cfg["DIR"] == "elsewhere" and cfg["VAL.checkpoint"] == "epoch_1.pth"
    assert cfg["DATASET.padding_constant"] == 8
    assert E.load_cfg("", [])["DATASET.imgSizes"] == (300, 375, 450, 525, 600)
