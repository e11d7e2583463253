"""GPU: dml_incremental_predict, the prediction plan behind model.predict and the test_self_distillation.py driver.

Kernel cases (tests/incremental_cases.py): the C ABI against the fp64 rule on DECIDED pixels -- top-two gap of every head above
64 eps32 sum|terms|, at most 1 % of a case excluded -- with zero mismatches allowed; constructed pixels, exact ties, the
optional per-head maps, misaligned / odd-length outputs, pad columns that must never be read, and every documented error code
with the output untouched.  Model: predict(x) against the same merge applied with torch to that model's own model(x) logits,
on the pixels those logits decide."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import incremental_cases as IC

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def st():
    return torch.cuda.current_stream().cuda_stream


def run_kernel(heads, B, h, w, Hh, Ww, maps=True, shift=0, sentinel=-7):
    """preds [B,H,W] (int64, on the host), per-head maps or None.  shift = 1: preds starts 8 bytes off a 16-byte boundary."""
    from dmlnet import _lib
    lib = _lib.load()
    es = [hd["e"].to(dev()).contiguous() for hd in heads]
    tab = (_lib.PredictHead * len(heads))(*[_lib.PredictHead(e.data_ptr(), hd["C"], hd["K"], hd["ld"], hd["novel_id"])
                                            for e, hd in zip(es, heads)])
    n_px = B * Hh * Ww
    buf = torch.full((n_px + shift + 2,), sentinel, dtype=torch.int64, device=dev())
    preds = buf[shift:shift + n_px]
    assert preds.data_ptr() % 16 == 8 * shift
    am = torch.full((len(heads), B, Hh, Ww), 255, dtype=torch.uint8, device=dev()) if maps else None
    rc = lib.dml_incremental_predict(tab, len(heads), preds.data_ptr(), am.data_ptr() if maps else None, B, h, w, Hh, Ww, st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert (buf[:shift] == sentinel).all() and (buf[shift + n_px:] == sentinel).all(), "wrote outside preds"
    return preds.cpu().reshape(B, Hh, Ww), (am.cpu().long() if maps else None)


def check_case(heads, ref, shape, **kw):
    h, w, Hh, Ww, B = shape
    preds, am = run_kernel(heads, B, h, w, Hh, Ww, **kw)
    dec = ref["decided"]
    bad = int((preds[dec] != ref["pred"][dec]).sum())
    print("%r: %d / %d pixels decided, %d mismatches" % (shape, int(dec.sum()), dec.numel(), bad))
    assert bad == 0
    if am is not None:
        for i, a in enumerate(ref["argmax"]):
            assert torch.equal(am[i][dec], a[dec]), "per-head map %d" % i
    return preds


@pytest.mark.parametrize("c", IC.CASES, ids=IC.case_id)
def test_kernel_matches_fp64_rule(c):
    seed, shape, hs = c
    heads, ref = IC.case(seed, shape, hs)
    with_maps = check_case(heads, ref, shape)
    h, w, Hh, Ww, B = shape
    without, none = run_kernel(heads, B, h, w, Hh, Ww, maps=False)              # NULL per-head maps are accepted
    assert none is None and torch.equal(with_maps, without)
    shifted, _ = run_kernel(heads, B, h, w, Hh, Ww, maps=False, shift=1)       # single first pixel, pairs after it
    assert torch.equal(with_maps, shifted)


@pytest.mark.parametrize("ld_extra", [4, 1], ids=["vector-rows", "scalar-rows"])
def test_padding_columns_are_never_read(ld_extra):
    shape, hs = (5, 7, 18, 27, 2), ((16, 17, 18), (16, 24, 24), (0, 16, 17))
    heads, ref = IC.case(IC.SEED, shape, hs, ld_extra=ld_extra)
    assert all(torch.isnan(hd["e"][..., hd["C"]:]).all() and hd["ld"] > hd["C"] for hd in heads)
    padded = check_case(heads, ref, shape)
    tight, _ = run_kernel(IC.make_heads(IC.SEED, shape, hs), 2, 5, 7, 18, 27)
    assert torch.equal(padded, tight)


def test_k_equal_c_plus_one_uses_the_zero_row():
    shape, hs = (3, 5, 12, 20, 2), ((33,), (32,), (0,))
    heads, ref = IC.case(IC.SEED, shape, hs)
    preds = check_case(heads, ref, shape)
    assert (preds == 32).any()


def onto(protos, C):
    """[n_px] prototype indices -> embedding [1,1,n_px,C] set exactly onto 3 I rows"""
    e = torch.zeros(1, 1, len(protos), C)
    for i, k in enumerate(protos):
        e[0, 0, i, k] = 3.0
    return e


def test_constructed_pixels_merge_rule():
    # h = w = H = W sizes: nothing interpolates.  pixels: heads 1 and 2 both fire | head 2 says 16 (head 1's id, not its
    # own) | head 1 fires alone | nothing fires
    a0, a1, a2 = [3, 3, 3, 3], [16, 5, 16, 4], [17, 16, 2, 6]
    heads = [dict(e=onto(a0, 16), C=16, K=16, ld=16, novel_id=0), dict(e=onto(a1, 24), C=24, K=17, ld=24, novel_id=16),
             dict(e=onto(a2, 24), C=24, K=18, ld=24, novel_id=17)]
    preds, am = run_kernel(heads, 1, 1, 4, 1, 4)
    assert preds.reshape(-1).tolist() == [17, 3, 16, 3]
    assert [am[i].reshape(-1).tolist() for i in range(3)] == [a0, a1, a2]
    ref = IC.reference(heads, 1, 4)
    assert ref["decided"].all() and torch.equal(ref["pred"], preds)
    # the order of the heads is the order of the overrides: with the two incremental heads swapped head 1's 16 comes last
    swapped = [heads[0], heads[2], heads[1]]
    p2, _ = run_kernel(swapped, 1, 1, 4, 1, 4)
    assert p2.reshape(-1).tolist() == [16, 3, 16, 3]


def test_exact_ties_take_the_lowest_index():
    hs = ((16, 17, 18), (16, 24, 24), (0, 16, 17))
    heads = [dict(e=torch.zeros(2, 3, 5, C), C=C, K=K, ld=C, novel_id=i) for K, C, i in zip(*hs)]
    preds, am = run_kernel(heads, 2, 3, 5, 12, 20)
    assert (preds == 0).all() and (am == 0).all()               # all-zero embedding: every logit is -9, every head says 0
    e = torch.zeros(2, 3, 5, 16)
    e[..., 3] = 1.5
    e[..., 7] = 1.5                                             # equidistant from prototypes 3 and 7
    preds, am = run_kernel([dict(e=e, C=16, K=16, ld=16, novel_id=0)], 2, 3, 5, 13, 19)
    assert (preds == 3).all() and (am == 3).all()


def test_error_codes_leave_preds_untouched():
    from dmlnet import _lib
    lib = _lib.load()
    e = torch.zeros(1, 2, 2, 40, device=dev())
    preds = torch.full((64,), -7, dtype=torch.int64, device=dev())

    def call(heads=((16, 16, 16, 16),), n=None, p=None, tab_null=False, B=1, h=2, w=2, Hh=4, Ww=4, e_ptr=e.data_ptr()):
        tab = (_lib.PredictHead * max(len(heads), 1))(*[_lib.PredictHead(e_ptr, *hd) for hd in heads])
        return lib.dml_incremental_predict(None if tab_null else tab, len(heads) if n is None else n,
                                           preds.data_ptr() if p is None else p, None, B, h, w, Hh, Ww, st())
    EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
    assert call(tab_null=True) == EINVAL
    assert lib.dml_incremental_predict((_lib.PredictHead * 1)(_lib.PredictHead(e.data_ptr(), 16, 16, 16, 0)), 1, None, None,
                                       1, 2, 2, 4, 4, st()) == EINVAL
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL
    for kw in (dict(B=0), dict(h=0), dict(w=0), dict(Hh=0), dict(Ww=0), dict(B=-1), dict(Hh=-4)):
        assert call(**kw) == EINVAL, kw
    assert call(e_ptr=None) == EINVAL
    assert call(heads=((0, 16, 16, 0),)) == EINVAL              # C <= 0
    assert call(heads=((16, 0, 16, 0),)) == EINVAL              # K <= 0
    assert call(heads=((16, 16, 12, 0),)) == EINVAL             # ld < C
    assert call(heads=((16, 16, 16, 0),) * 5) == EUNSUPPORTED   # n > 4
    assert call(heads=((36, 16, 40, 0),)) == EUNSUPPORTED       # C > 32
    assert call(heads=((32, 34, 32, 0),)) == EUNSUPPORTED       # K > 33
    assert call(heads=((16, 18, 16, 0),)) == EUNSUPPORTED       # K > C + 1
    assert call(heads=((16, 16, 16, 0), (16, 18, 16, 17))) == EUNSUPPORTED
    assert call(p=preds.data_ptr() + 4) == EALIGN
    torch.cuda.synchronize()
    assert (preds == -7).all()
    # the limits themselves pass; on a zero embedding the zero row of a K = C + 1 head is the nearest prototype
    assert call(heads=((16, 17, 16, 0),)) == 0
    torch.cuda.synchronize()
    assert (preds[:16] == 16).all() and (preds[16:] == -7).all()
    assert call(heads=((32, 33, 40, 0),)) == 0
    torch.cuda.synchronize()
    assert (preds[:16] == 32).all() and (preds[16:] == -7).all()


@pytest.mark.parametrize("padded", [False, True], ids=["c17-scalar-rows", "c24-vector-rows"])
def test_g17_fixture(padded):
    g = H.load_golden("g17_incremental")
    e0, e1 = torch.from_numpy(g["e0"]), torch.from_numpy(g["e1"])
    C1 = 17
    if padded:                                                   # as the engine carries it: 17 -> 24 channels, zeros beyond
        e1 = torch.cat([e1, torch.zeros(2, 16, 16, 7)], -1)
        C1 = 24
    heads = [dict(e=e0, C=16, K=16, ld=16, novel_id=0), dict(e=e1, C=C1, K=17, ld=C1, novel_id=16)]
    preds, _ = run_kernel(heads, 2, 16, 16, 64, 64)
    dec, want = torch.from_numpy(g["decided"]).bool(), torch.from_numpy(g["pred"]).long()
    assert int((preds[dec] != want[dec]).sum()) == 0
    assert (preds == 16).double().mean() >= 0.01


# ---------------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------------
def decided_by_model(logits, feats):
    """the margin of incremental_cases on the model's own float32 outputs: A from the features it returns"""
    dec = None
    for lg, ft in zip(logits, feats):
        f = ft.double().abs()
        A = (f ** 2).sum(-1) + 6.0 * f.max(-1).values + 9.0
        d = IC.decided_from_logits(lg.double(), A)
        dec = d if dec is None else dec & d
    return dec


def torch_merge(logits, novel_ids):
    return IC.merge([IC.first_max(lg.double().cpu()) for lg in logits], novel_ids)


@pytest.fixture(scope="module")
def sd_model():
    import network
    m = network.deeplabv3plus_embedding_self_distillation_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
    m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=5))          # the weights of the g17 fixture
    return m.to(dev()).eval()


@pytest.mark.parametrize("size", [(64, 64), (64, 80)], ids=["64x64", "64x80"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_predict_equals_merge_of_the_models_own_logits(sd_model, mode, size):
    m = sd_model
    m.set_compute_dtype(torch.float32 if mode == "f32" else torch.bfloat16, fp32_products="exact")
    x = H.synth_tensor(5, "g17.img", (2, 3) + size).to(dev())
    with torch.no_grad():
        lg, _, ft = m(x)
        before = [t.clone() for t in lg + ft]
        preds = m.predict(x)
        base = m.predict(x, novel_cls=0)
        lg2, _, ft2 = m(x)
    assert preds.shape == (2,) + size and preds.dtype == torch.int64 and preds.is_cuda
    # the prediction plan is a plan of its own: model(x) is bit for bit what it was
    assert all(torch.equal(a, b) for a, b in zip(before, lg2 + ft2))
    dec = decided_by_model([t.cpu() for t in lg], [t.cpu() for t in ft])
    undecided = 1.0 - dec.double().mean().item()
    want = torch_merge(lg, [0, 16])
    bad = int((preds.cpu()[dec] != want[dec]).sum())
    print("%s %r: undecided %.3f %%, overridden %.2f %%, mismatches %d" % (mode, size, 100 * undecided,
                                                                          100 * (want == 16).double().mean(), bad))
    assert undecided <= IC.MAX_UNDECIDED and bad == 0
    assert (want == 16).any() and (want != 16).any()
    assert int((base.cpu()[dec] != IC.first_max(lg[0].double().cpu())[dec]).sum()) == 0
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.predict(x)
    finally:
        m.eval()


def test_single_head_predict_is_the_argmax():
    import network
    m = network.deeplabv3plus_embedding_resnet50(num_classes=16, output_stride=16, pretrained_backbone=False)
    m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=5))
    m.to(dev()).eval()
    x = H.synth_tensor(5, "g17.img", (2, 3, 64, 80)).to(dev())
    with torch.no_grad():
        lg, _, ft = m(x)
        preds = m.predict(x)
    dec = decided_by_model([lg.cpu()], [ft.cpu()])
    assert 1.0 - dec.double().mean().item() <= IC.MAX_UNDECIDED
    assert int((preds.cpu()[dec] != IC.first_max(lg.double().cpu())[dec]).sum()) == 0


def test_three_incremental_heads():
    from network import modeling as M
    m = M._segm_resnet("deeplabv3plus_embedding_self_distillation", "resnet101", None, 16, False, cls_novel=3)
    keys = set(m.state_dict().keys())
    for i, k in ((1, 17), (2, 18), (3, 19)):
        assert m.state_dict()["classifier_%d.classifier.3.weight" % i].shape[0] == k
    assert not any(k.startswith("classifier_4") for k in keys)
    m.load_state_dict(H.synth_state_dict(H.shapes_of(m), seed=5))
    with torch.no_grad():
        # with these weights only head 1 claims pixels; 0.5 on each head's own novel channel makes all three fire (the fp64
        # oracle on this input: 8 %, 2 % and 0.3 % of the pixels end as 16, 17 and 18)
        for i in (1, 2, 3):
            getattr(m, "classifier_%d" % i).classifier[3].bias[15 + i] += 0.5
    m.to(dev()).eval()
    x = H.synth_tensor(5, "g17.img", (2, 3, 64, 64)).to(dev())
    with torch.no_grad():
        lg, _, ft = m(x)
        preds = m.predict(x)
        two = m.predict(x, novel_cls=2)
    dec = decided_by_model([t.cpu() for t in lg], [t.cpu() for t in ft])
    assert 1.0 - dec.double().mean().item() <= IC.MAX_UNDECIDED
    want = torch_merge(lg, [0, 16, 17, 18])
    assert int((preds.cpu()[dec] != want[dec]).sum()) == 0
    assert int((two.cpu()[dec] != torch_merge(lg[:3], [0, 16, 17])[dec]).sum()) == 0
    assert int(want.max()) == 18 and int(preds.max()) == 18      # ids up to 18
    with pytest.raises(ValueError):
        m.predict(x, novel_cls=4)


# ---------------------------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    cwd = tmp_path_factory.mktemp("selfdist")
    cmd = [sys.executable, os.path.join(H.PKG, "test_self_distillation.py"), "--synthetic", "--height", "64", "--width", "64",
           "--num_images", "2", "--novel_cls", "1", "--test_only", "--save_val_results"]
    r = subprocess.run(cmd, cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return cwd, r.stdout


def test_driver_mean_iou(driver_run):
    _, out = driver_run
    printed = float(re.search(r"Mean IoU: ([0-9.]+|nan)", out).group(1))
    sys.path.insert(0, H.PKG)
    import test_self_distillation as drv
    from datasets import Cityscapes
    o = drv.build_parser().parse_args(["--synthetic", "--height", "64", "--width", "64", "--num_images", "2", "--novel_cls", "1"])
    torch.manual_seed(1)
    m = drv.build_model(o).to(dev()).eval()
    m.set_compute_dtype(torch.bfloat16)
    lut = Cityscapes.eval_relabel_lut([13], [16]).astype(np.int64)
    conf = np.zeros((17, 17))
    for i in range(2):
        img, lab = drv.synthetic_batch(i, 1, 64, 64, 17, dev())
        with torch.no_grad():
            p = m.predict(img, novel_cls=1).cpu().numpy().reshape(-1)
        t = lut[lab.cpu().numpy().reshape(-1)]
        ok = (t >= 0) & (t < 17)
        conf += np.bincount(17 * t[ok] + p[ok], minlength=17 * 17).reshape(17, 17)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.diag(conf) / (conf.sum(1) + conf.sum(0) - np.diag(conf))
    assert abs(printed - float(np.nanmean(iou))) < 1e-6, (printed, float(np.nanmean(iou)))


def test_driver_writes_the_pngs(driver_run):
    from PIL import Image
    cwd, _ = driver_run
    names = sorted(os.listdir(os.path.join(str(cwd), "results")))
    assert names == ["0_pred.png", "0_target.png", "1_pred.png", "1_target.png"]
    for n in names:
        im = Image.open(os.path.join(str(cwd), "results", n))
        assert im.size == (64, 64) and im.mode == "RGB"
