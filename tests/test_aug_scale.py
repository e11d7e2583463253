"""Scale / resize / pad / centre-crop transforms, CPU side: the restatement (tests/scale_ref.py) against the reference's
fixtures (g16) and live Pillow, and the product's host logic (utils/ext_transforms.py sampler, utils/scale_window.py tables)
against the restatement."""
import glob
import json
import os
import random

import numpy as np
import pytest
from PIL import Image

import helpers as H  # noqa: F401  (path setup)
import pil_resample as PR
import scale_ref as SR

G16 = sorted(glob.glob(os.path.join(H.GOLDEN, "g16_scale_*.npz")))
IDS = [os.path.basename(p)[10:-4] for p in G16]
MEAN, STD = PR.MEAN, PR.STD
JIT = ["ExtColorJitter", {"brightness": 0.5, "contrast": 0.5, "saturation": 0.5}]
FLIP = ["ExtRandomHorizontalFlip", {}]
TAIL = [["ExtToTensor", {}], ["ExtNormalize", {"mean": MEAN, "std": STD}]]


def _fixture(path):
    g = np.load(path)
    return g, int(g["seed"]), json.loads(str(g["spec"]))


def test_fixture_set_is_complete():
    assert len(G16) == 14 and {"train_down", "train_up", "train_onepad", "scale", "resize_int", "resize_pair",
                               "resize_center_wide", "crop_padding", "raw_ids"} <= set(IDS)
    for p in G16:
        assert os.path.getsize(p) <= 14956                   # the largest g9_aug fixture


@pytest.mark.parametrize("path", G16, ids=IDS)
def test_restatement_reproduces_reference_fixture(path):
    """bit-exact, including the order of `random` draws: the fixture stores only the seed"""
    g, seed, spec = _fixture(path)
    img, lbl, _ = SR.run(spec, g["img"], g["lbl"], random.Random(seed))
    assert img.dtype == np.float32 and np.array_equal(img, g["out_img"])
    assert np.array_equal(lbl, g["out_lbl"])


def test_fixtures_cover_the_padding_cases():
    def trace(name):
        g, seed, spec = _fixture(G16[IDS.index(name)])
        return SR.run(spec, g["img"], g["lbl"], random.Random(seed))[2], spec[1][1]["size"]
    t, (th, tw) = trace("train_down")
    hs, ws = t["size"]
    q = int((1 + tw - ws) / 2)
    assert ws < tw and hs + 2 * q < th                       # both pad_if_needed stages fire
    t, (th, tw) = trace("train_up")
    assert t["size"][0] >= th and t["size"][1] >= tw and t["oy"] >= 0 and t["ox"] >= 0
    t, (th, tw) = trace("train_onepad")
    hs, ws = t["size"]
    assert ws < tw and hs + 2 * int((1 + tw - ws) / 2) >= th
    t, _ = trace("resize_center_wide")
    assert t["ox"] < 0 <= t["oy"] and t["size"] == (24, 33)


def _size_pairs(rs, n, lo, hi):
    """n (in, out) pairs: in in [lo, hi], out = int(in * scale) with a scale in [0.5, 2] that keeps out >= 1."""
    out = []
    while len(out) < n:
        a = int(rs.randint(lo, hi + 1))
        b = int(a * rs.uniform(0.5, 2.0))
        if b >= 1:
            out.append((a, b))
    return out


def test_nearest_restatement_equals_live_pillow():
    rs = np.random.RandomState(16)
    hp, wp = _size_pairs(rs, 240, 2, 600), _size_pairs(rs, 240, 2, 600)
    ran = 0
    for (h, hs), (w, ws) in zip(hp, wp):
        # both axes at once on a thin strip: the row rule on [h, 3], the column rule on [3, w]
        for shape, size in (((h, 3), (hs, 3)), ((3, w), (3, ws))):
            a = rs.randint(0, 256, shape).astype(np.uint8)
            want = np.array(Image.fromarray(a).resize(size[::-1], Image.NEAREST))
            assert np.array_equal(SR.resize_nearest(a, size), want), (shape, size)
        ran += 1
    assert ran == 240
    # 2-D, both axes change
    for k in range(40):
        (h, hs), (w, ws) = hp[k], wp[k]
        h, w = min(h, 90), min(w, 90)
        hs, ws = max(1, min(hs, 120)), max(1, min(ws, 120))
        a = rs.randint(0, 256, (h, w)).astype(np.uint8)
        assert np.array_equal(SR.resize_nearest(a, (hs, ws)), np.array(Image.fromarray(a).resize((ws, hs), Image.NEAREST)))


def test_bilinear_restatement_equals_live_pillow():
    rs = np.random.RandomState(17)
    ran = 0
    for (h, hs), (w, ws) in zip(_size_pairs(rs, 220, 1, 48), _size_pairs(rs, 220, 1, 64)):
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        want = np.array(Image.fromarray(a).resize((ws, hs), Image.BILINEAR))
        assert np.array_equal(PR.resize(a, (hs, ws)), want), (h, w, hs, ws)
        ran += 1
    assert ran == 220


SPECS = {
    "train": [["ExtRandomScale", {"scale_range": [0.5, 2.0]}], ["ExtRandomCrop", {"size": [24, 32], "pad_if_needed": True}],
              JIT, FLIP] + TAIL,
    "train_small": [["ExtRandomScale", {"scale_range": [0.5, 0.7]}], ["ExtRandomCrop", {"size": 30, "pad_if_needed": True}],
                    JIT, FLIP] + TAIL,
    # 32 x 44 -> 16 x 22; width pad 5 -> 26 x 32: the padded size equals the crop size, no crop draw
    "no_draw": [["ExtScale", {"scale": 0.5}], ["ExtRandomCrop", {"size": [26, 32], "pad_if_needed": True}], JIT, FLIP] + TAIL,
    "padding": [["ExtRandomCrop", {"size": [20, 28], "padding": 3}], JIT, FLIP] + TAIL,
    "padding_both": [["ExtResize", {"size": [20, 30]}], ["ExtRandomCrop", {"size": 29, "padding": 2, "pad_if_needed": True}],
                     FLIP] + TAIL,
    "crop_val": [["ExtResize", {"size": 24}], ["ExtCenterCrop", {"size": 24}]] + TAIL,
    "center_big": [["ExtCenterCrop", {"size": [37, 31]}], FLIP] + TAIL,
    "scale_only": [["ExtScale", {"scale": 1.3}]] + TAIL,
    "random_scale_only": [["ExtRandomScale", {"scale_range": [0.6, 1.4]}], JIT] + TAIL,
}


def _et():
    import utils
    return utils.ext_transforms


@pytest.mark.parametrize("name", sorted(SPECS))
def test_product_sampler_draws_like_the_restatement(name):
    et, spec = _et(), SPECS[name]
    tf = SR.build(et, spec)
    assert tf.windowed
    rs = np.random.RandomState(3)
    img, lbl = rs.randint(0, 256, (32, 44, 3)).astype(np.uint8), rs.randint(0, 19, (32, 44)).astype(np.uint8)
    B = 1 if name == "random_scale_only" else 3
    for seed in (1, 2, 3, 15, 99, 1234):
        random.seed(seed)
        got, out = tf.sample(B, 32, 44)
        rng = random.Random(seed)
        for b in range(B):
            t = SR.run(spec, img, lbl, rng)[2]
            assert {k: got[b][k] for k in ("size", "oy", "ox", "ops", "flip", "out")} == \
                {k: (tuple(t[k]) if k in ("size", "out") else t[k]) for k in ("size", "oy", "ox", "ops", "flip", "out")}
            assert tuple(out) == tuple(t["out"])
        assert random.random() == rng.random()               # the same number of draws consumed
    if name == "no_draw":
        assert got[0]["size"] == (16, 22) and (got[0]["oy"], got[0]["ox"]) == (-5, -5) and got[0]["i"] == got[0]["j"] == 0


def _restated_tables(h, w, hs, ws, oy, ox, th, tw):
    """Per window row / column: (first source index, taps, weights) and the NEAREST index, from the loop-by-loop tables."""
    def axis(n_in, n_out, origin, extent):
        if n_in == n_out:
            bounds, kk = [(v, 1) for v in range(n_out)], [[1 << 22] for _ in range(n_out)]
        else:
            bounds, kk = PR.coeffs(n_in, n_out)
        near = SR.nearest_index(n_in, n_out) if n_in != n_out else list(range(n_out))
        rows = []
        for v in range(origin, origin + extent):
            if 0 <= v < n_out:
                n = int(bounds[v][1])
                rows.append((int(bounds[v][0]), n, [int(c) for c in kk[v][:n]], int(near[v])))
            else:
                rows.append((None, 0, [], -1))
        return rows
    return axis(w, ws, ox, tw), axis(h, hs, oy, th)


def _check_tables(h, w, hs, ws, oy, ox, th, tw):
    from utils import scale_window as SW
    tabs = SW.window_tables(h, w, hs, ws, oy, ox, th, tw)
    SW.validate(tabs, h, w)
    hb, hk, vb, vk, lr, lc = tabs
    assert all(t.dtype == np.int32 for t in tabs)
    cols, rows = _restated_tables(h, w, hs, ws, oy, ox, th, tw)
    for want, b, k, near in ((cols, hb, hk, lc), (rows, vb, vk, lr)):
        assert b.shape == (len(want), 2) and k.shape[0] == len(want) and near.shape == (len(want),)
        for v, (first, n, coef, idx) in enumerate(want):
            assert int(b[v, 1]) == n and int(near[v]) == idx
            if n:
                assert int(b[v, 0]) == first and [int(c) for c in k[v, :n]] == coef
            assert not k[v, n:].any()
    return tabs


def _emulate(tabs, img, lbl):
    """What the kernel computes from the tables, in numpy: horizontal pass, uint8, vertical pass, uint8; label gather."""
    hb, hk, vb, vk, lr, lc = tabs
    th, tw = vb.shape[0], hb.shape[0]
    inter = np.zeros((img.shape[0], tw, 3), np.int64)
    for x in range(tw):
        acc = np.full((img.shape[0], 3), 1 << 21, np.int64)
        for q in range(hb[x, 1]):
            acc += img[:, hb[x, 0] + q].astype(np.int64) * int(hk[x, q])
        inter[:, x] = np.clip(acc >> 22, 0, 255)
    out = np.zeros((th, tw, 3), np.uint8)
    ol = np.zeros((th, tw), np.uint8)
    for y in range(th):
        acc = np.full((tw, 3), 1 << 21, np.int64)
        for q in range(vb[y, 1]):
            acc += inter[vb[y, 0] + q] * int(vk[y, q])
        out[y] = np.clip(acc >> 22, 0, 255)
        if lr[y] >= 0:
            ok = lc >= 0
            ol[y, ok] = lbl[lr[y], lc[ok]]
    return out, ol


@pytest.mark.parametrize("path", G16, ids=IDS)
def test_host_tables_equal_the_restatement_on_fixtures(path):
    g, seed, spec = _fixture(path)
    h, w = g["img"].shape[:2]
    t = SR.run(spec, g["img"], g["lbl"], random.Random(seed))[2]
    (hs, ws), (th, tw) = t["size"], t["out"]
    tabs = _check_tables(h, w, hs, ws, t["oy"], t["ox"], th, tw)
    wi, wl = SR.window(g["img"], g["lbl"], (hs, ws), t["oy"], t["ox"], (th, tw))
    ei, el = _emulate(tabs, g["img"], g["lbl"])
    assert np.array_equal(ei, wi) and np.array_equal(el, wl)


def test_host_tables_equal_the_restatement_on_random_windows():
    from utils import scale_window as SW
    rs = np.random.RandomState(21)
    ran = 0
    for trial in range(60):
        h, w = int(rs.randint(5, 40)), int(rs.randint(5, 50))
        sc = [0.5, 1.0, 2.0][trial] if trial < 3 else float(rs.uniform(0.5, 2.0))
        hs, ws = max(1, int(h * sc)), max(1, int(w * sc))
        if trial % 7 == 3:
            ws = w                                           # one axis keeps its size
        th, tw = int(rs.randint(1, 45)), int(rs.randint(1, 70))
        oy, ox = int(rs.randint(-12, hs + 4)), int(rs.randint(-12, ws + 4))
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        lbl = rs.randint(0, 256, (h, w)).astype(np.uint8)
        tabs = _check_tables(h, w, hs, ws, oy, ox, th, tw)
        wi, wl = SR.window(img, lbl, (hs, ws), oy, ox, (th, tw))
        ei, el = _emulate(tabs, img, lbl)
        assert np.array_equal(ei, wi) and np.array_equal(el, wl), (h, w, hs, ws, oy, ox, th, tw)
        ran += 1
    assert ran == 60
    # the packed batch: records first, every offset inside the buffer, one band height for all samples
    wins = [(20, 28, -3, -2), (64, 88, 10, 30), (32, 44, 0, 0), (16, 22, -6, -9)]
    buf, band, rows = SW.pack(wins, 32, 44, 28, 36)
    assert buf.dtype == np.int32 and band in (16, 8, 4, 2, 1) and 1 <= rows <= 256
    head = buf[:len(wins) * 8].reshape(len(wins), 8)
    for b, win in enumerate(wins):
        tabs = SW.window_tables(32, 44, *win, 28, 36)
        for f, t in enumerate(tabs):
            assert np.array_equal(buf[head[b, f]:head[b, f] + t.size], t.reshape(-1))
        assert (head[b, 6], head[b, 7]) == (tabs[1].shape[1], tabs[3].shape[1])
        y0 = np.arange(0, 28, band)
        y1 = np.minimum(y0 + band, 28) - 1
        assert int((tabs[2][y1, 0] + tabs[2][y1, 1] - tabs[2][y0, 0]).max()) <= rows
    # scale 0.5 (support 2, at most five taps per row): a 16-row band spans at most 2 * 15 + 5 source rows
    band, rows = SW.band_rows([SW.window_tables(1024, 2048, 512, 1024, -128, -100, 768, 768)[2]])
    assert band == 16 and rows <= 35
    bad = [t.copy() for t in SW.window_tables(32, 44, 20, 28, 0, 0, 20, 28)]
    bad[0][5, 0] = 43
    with pytest.raises(ValueError):
        SW.validate(bad, 32, 44)
    bad = [t.copy() for t in SW.window_tables(32, 44, 20, 28, 0, 0, 20, 28)]
    bad[4][2] = 32
    with pytest.raises(ValueError):
        SW.validate(bad, 32, 44)


def test_nearest_product_table_equals_the_restatement():
    from utils import scale_window as SW
    rs = np.random.RandomState(5)
    for n_in, n_out in _size_pairs(rs, 300, 1, 2100):
        assert SW.nearest_index(n_in, n_out).tolist() == SR.nearest_index(n_in, n_out)


def test_unsupported_arguments_raise():
    et = _et()
    n = et.ExtNormalize(MEAN, STD)
    for cls, args in ((et.ExtRandomScale, ((0.5, 2.0),)), (et.ExtScale, (0.5,)), (et.ExtResize, (24,))):
        cls(*args, interpolation=2)
        for bad in (0, 3, 1):                                # NEAREST, BICUBIC, LANCZOS
            with pytest.raises(NotImplementedError):
                cls(*args, interpolation=bad)
    with pytest.raises(NotImplementedError):
        et.ExtRandomCrop(8, padding=(1, 2, 3, 4))
    for seq in ([et.ExtRandomCrop(8), et.ExtScale(0.5), et.ExtToTensor(), n],
                [et.ExtScale(0.5), et.ExtResize(8), et.ExtToTensor(), n],
                [et.ExtRandomCrop(8), et.ExtCenterCrop(8), et.ExtToTensor(), n],
                [et.ExtColorJitter(0.5), et.ExtCenterCrop(8), et.ExtToTensor(), n],
                [et.ExtScale(0.5), et.ExtToTensor()],
                [et.ExtToTensor(), et.ExtRandomCrop(4), n]):
        with pytest.raises(NotImplementedError):
            et.ExtCompose(seq)
    with pytest.raises(NotImplementedError):
        et.ExtColorJitter(hue=0.1)
    tf = et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtColorJitter(0.5), et.ExtToTensor(), n])
    with pytest.raises(ValueError):
        tf.sample(2, 32, 44)
    assert len(tf.sample(1, 32, 44)[0]) == 1
    assert not hasattr(et, "ExtPad") and not hasattr(et, "ExtRandomRotation")


def test_sequences_without_new_stages_keep_their_parameters():
    et = _et()
    n = et.ExtNormalize(MEAN, STD)
    for seq in ([et.ExtRandomCrop(size=(20, 28)), et.ExtColorJitter(0.5, 0.5, 0.5), et.ExtRandomHorizontalFlip(),
                 et.ExtToTensor(), n],
                [et.ExtRandomCrop(20, padding=0, pad_if_needed=False), et.ExtToTensor(), n],
                [et.ExtToTensor(), n]):
        tf = et.ExtCompose(seq)
        assert not tf.windowed
        random.seed(4)
        got, _ = tf.sample(3, 28, 36)
        assert all(set(p) == {"i", "j", "ops", "flip"} for p in got)
    assert et.ExtCompose([et.ExtRandomCrop(20, pad_if_needed=True), et.ExtToTensor(), n]).windowed
