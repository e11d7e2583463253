"""GPU: the reconstruction-consistency score (dml_rec_cosine, dml_rec_confidence; utils.rec_cosine_score,
utils.rec_confidence) against the float64 definition of tests/rec_cases.py within its GPU_BAR, the pyramid concats the
engine hands out against the oracle decoder, models.evaluate_multiscale_rec, and the reader's rec_dataset."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import rec_cases as RC
import test_ppm_model as PM

pytestmark = pytest.mark.gpu

F64 = np.float64


def _device_feats(arrays, c):
    """the case's arrays on the device in its dtype, scale s inside a buffer of pitch ld[s] whose padding holds NaN"""
    dt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    out = []
    for s, a in enumerate(arrays):
        ld = c["C"] if c["ld"] is None else c["ld"][s]
        buf = torch.full(a.shape[:3] + (ld,), float("nan"), dtype=dt, device="cuda")
        buf[..., :c["C"]] = torch.tensor(a).to(dt).cuda()
        out.append(buf[..., :c["C"]])
    return out


def _run(name):
    import utils
    c = RC.CASES[name]
    f1, f2 = RC.inputs(name)
    d1, d2 = _device_feats(f1, c), _device_feats(f2, c)
    cos = utils.rec_cosine_score(d1, d2, c["out"])
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (c["B"],) + tuple(c["out"])
    return cos, d1, d2


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_cosine_matches_the_float64_definition(name):
    cos, d1, d2 = _run(name)
    got = cos.cpu().numpy()
    ref, zero = RC.reference(name)
    err = np.abs(got.astype(F64) - ref).max()
    print("MEASURE %s err=%.3e (bar %.1e) zero pixels=%d" % (name, err, RC.GPU_BAR, zero.sum()))
    assert np.isfinite(got).all()
    assert err <= RC.GPU_BAR
    assert (got[zero] == 0.0).all()                      # an all-zero vector gives exactly 0, never NaN
    if RC.CASES[name]["mode"] == "same":
        assert np.abs(got - 1.0).max() <= RC.GPU_BAR
    # bitwise reproducible
    import utils
    again = utils.rec_cosine_score(d1, d2, RC.CASES[name]["out"])
    assert torch.equal(again, cos)


def test_cosine_unaligned_pointers_take_the_scalar_path():
    """the same values from a view that starts one element into its buffer: no 16-byte load is possible"""
    import utils
    c = RC.CASES["eight_scales_b2"]
    f1, f2 = RC.inputs("eight_scales_b2")

    def shifted(arrays):
        out = []
        for a in arrays:
            flat = torch.empty(a.size + 1, device="cuda")
            flat[1:] = torch.tensor(a).cuda().reshape(-1)
            out.append(flat[1:].view(a.shape))
        return out

    got = utils.rec_cosine_score(shifted(f1), shifted(f2), c["out"]).cpu().numpy()
    ref, _ = RC.reference("eight_scales_b2")
    assert np.abs(got.astype(F64) - ref).max() <= RC.GPU_BAR


def test_cosine_wrapper_refuses_what_the_kernel_cannot_take():
    import utils
    a = torch.zeros(1, 2, 2, 8, device="cuda")
    with pytest.raises(ValueError):
        utils.rec_cosine_score([a], [a, a], (2, 2))
    with pytest.raises(ValueError):
        utils.rec_cosine_score([a], [torch.zeros(1, 2, 3, 8, device="cuda")], (2, 2))
    with pytest.raises(ValueError):
        utils.rec_cosine_score([a] * 9, [a] * 9, (2, 2))
    with pytest.raises(TypeError):
        utils.rec_cosine_score([a.half()], [a.half()], (2, 2))
    # a layout that is not dense-with-a-pitch is copied, not misread
    x = torch.randn(1, 8, 3, 4, device="cuda")                       # NCHW storage, viewed as [B, h, w, C]
    got = utils.rec_cosine_score([x.permute(0, 2, 3, 1)], [x.permute(0, 2, 3, 1)], (3, 4))
    assert (got - 1.0).abs().max().item() <= RC.GPU_BAR


@pytest.mark.parametrize("name", sorted(RC.CONF_CASES))
def test_confidence_matches_the_float64_definition(name):
    import utils
    c = RC.CONF_CASES[name]
    scores, cos = RC.conf_inputs(name)
    ref = RC.conf_reference(name)
    got = utils.rec_confidence(torch.tensor(scores).cuda(), torch.tensor(cos).cuda(), threshold=c["threshold"],
                               prob=c["prob"], first_class=c["first_class"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"],) + RC.CONF_HW
    got = got.cpu().numpy().astype(F64)
    keep = ~ref["near"]
    err = np.abs(got - ref["conf"])[keep].max()
    print("MEASURE %s err=%.3e (bar %.1e) left out %d pixels" % (name, err, RC.GPU_BAR, ref["near"].sum()))
    assert ref["near"].mean() <= RC.GATE_MAX_FRACTION
    assert err <= RC.GPU_BAR
    # a pixel near the threshold took one of the two branches
    near = ref["near"]
    assert (np.minimum(np.abs(got - ref["msp"]), np.abs(got - ref["rec"]))[near] <= RC.GPU_BAR).all()


def test_confidence_refuses_more_than_32_classes():
    import utils
    from dmlnet import _lib
    cos = torch.zeros(1, 2, 2, device="cuda")
    with pytest.raises(_lib.DmlError):
        utils.rec_confidence(torch.zeros(1, 40, 8, 8, device="cuda"), cos)
    with pytest.raises(_lib.DmlError):
        utils.rec_confidence(torch.zeros(1, 34, 8, 8, device="cuda"), cos, first_class=1)
    utils.rec_confidence(torch.zeros(1, 33, 8, 8, device="cuda"), cos, first_class=1)
    with pytest.raises(ValueError):
        utils.rec_confidence(torch.zeros(1, 13, 8, 8, device="cuda"), cos, prob="msp")


def test_no_large_temporary():
    """C = 4096 at output (45, 80): one accumulator of the composed route is 4096 x 45 x 80 x 4 = 59 MB; the kernel's only
    allocation is the returned map"""
    import utils
    g = torch.Generator(device="cuda").manual_seed(5)
    scales = ((10, 17), (12, 21), (15, 25), (17, 30), (19, 34))
    f1 = [torch.randn(1, h, w, 4096, device="cuda", generator=g) for h, w in scales]
    f2 = [t + 0.5 * torch.randn(t.shape, device="cuda", generator=g) for t in f1]
    utils.rec_cosine_score(f1[:1], f2[:1], (4, 4))                    # the library and its code object are loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cos = utils.rec_cosine_score(f1, f2, (45, 80))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("MEASURE peak rise %d bytes for a %d-byte map" % (rise, cos.numel() * 4))
    assert rise - cos.numel() * 4 < 1 << 20
    ref, _ = RC.cosine_ref([t.cpu().numpy() for t in f1], [t.cpu().numpy() for t in f2], (45, 80))
    assert np.abs(cos.cpu().numpy().astype(F64) - ref).max() <= RC.GPU_BAR


# ----------------------------------------------------------------------------------------------- engine and model
@pytest.fixture(scope="module")
def ppm():
    """the tiny pyramid-pooling model of tests/test_ppm_model.py in exact-fp32 mode, its oracle, and the two images"""
    from oracle import ppm_ref as O
    m = PM._product()
    o = O.SegmentationModuleOODRef()
    o.load_state_dict(PM._weights(o), strict=False)
    o.eval()
    imgs = PM._imgs()[:2]                                             # 64 x 96 and 88 x 120
    return m, o, imgs


def test_engine_concats_match_the_oracle_decoder(ppm):
    m, o, imgs = ppm
    seg = (64, 96)
    seen = []
    hook = o.decoder.conv_last[0].register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        with torch.no_grad():
            for img in imgs:
                o(img, seg)
    finally:
        hook.remove()
    dev = [t.cuda() for t in imgs]
    base_scores, base_feats = m._engine.infer_multiscale(dev, seg, m._dtype)
    scores, feats, cats = m._engine.infer_multiscale(dev, seg, m._dtype, keep_cat=True)
    assert len(cats) == len(seen) == 2
    for cat, want in zip(cats, seen):
        assert cat.dtype == torch.float32 and tuple(cat.shape) == (want.shape[0], want.shape[2], want.shape[3], 4096)
        PM.relclose(cat.permute(0, 3, 1, 2), want, PM.TOL, "pyramid concat %s" % (tuple(want.shape),))
    # the default call is untouched: same bits with and without the copies
    assert torch.equal(scores, base_scores) and torch.equal(feats, base_feats)
    # the copies are the caller's: another frame through the same plans leaves them alone
    held = [c.clone() for c in cats]
    none_s, none_f, cats2 = m._engine.infer_multiscale([t.flip(-1) for t in dev], seg, m._dtype, keep_cat=True, want_scores=False)
    torch.cuda.synchronize()
    assert none_s is None and none_f is None
    assert all(torch.equal(a, b) for a, b in zip(cats, held))
    assert not torch.equal(cats2[0], cats[0])
    # and the plans still give the first frame's scores afterwards
    again_scores, _ = m._engine.infer_multiscale(dev, seg, m._dtype)
    assert torch.equal(again_scores, base_scores)


def test_evaluate_multiscale_rec(ppm):
    import models
    m, o, imgs = ppm
    seg = (64, 96)
    dev = [t.cuda() for t in imgs]
    rec = [t + 0.3 * H.synth_tensor(16, "rec.noise%d" % i, t.shape).cuda() for i, t in enumerate(dev)]
    scores, cos = models.evaluate_multiscale_rec(m, dev, rec, seg)
    assert tuple(cos.shape) == (1, 16, 24) and cos.dtype == torch.float32
    base_scores, _ = models.evaluate_multiscale(m, dev, seg)
    assert torch.equal(scores, base_scores)
    _, _, c1 = m._engine.infer_multiscale(dev, seg, m._dtype, keep_cat=True, want_scores=False)
    _, _, c2 = m._engine.infer_multiscale(rec, seg, m._dtype, keep_cat=True, want_scores=False)
    ref, zero = RC.cosine_ref([t.cpu().numpy() for t in c1], [t.cpu().numpy() for t in c2], (16, 24))
    err = np.abs(cos.cpu().numpy().astype(F64) - ref).max()
    print("MEASURE evaluate_multiscale_rec err=%.3e, cos in [%.4f, %.4f]" % (err, ref.min(), ref.max()))
    assert not zero.any() and err <= RC.GPU_BAR
    assert ref.min() < 1.0 - 10 * RC.GPU_BAR                          # the perturbation shows
    with pytest.raises(ValueError):
        models.evaluate_multiscale_rec(m, dev, rec[:1], seg)
    with pytest.raises(ValueError):
        models.evaluate_multiscale_rec(m, dev, [rec[1], rec[0]], seg)


def test_driver_evaluates_synthetic_frames(ppm, monkeypatch):
    """eval_ood_rec.evaluate on two small synthetic frames: the reconstruction differs from the frame on the anomaly blocks
    only, so the cosine map ranks those pixels below the rest"""
    import eval_ood_rec as R
    import eval_ood_traditional as T
    m, _, _ = ppm
    monkeypatch.setattr(T, "IMG_SIZES", (48, 64))
    monkeypatch.setattr(T, "IMG_MAX_SIZE", 160)
    frames = list(R.synthetic_frames(2, 72, 128, 13, torch.device("cuda")))
    assert [tuple(t.shape) for t in frames[0][0]] == [(1, 3, 48, 88), (1, 3, 64, 120)]
    for imgs, recs, lab in frames:
        assert (lab == 13).any() and all(a.shape == b.shape and not torch.equal(a, b) for a, b in zip(imgs, recs))
    r = R.evaluate(m, frames, 14, "rec", (13,))
    print("MEASURE driver rec: auroc %.4f aupr %.4f fpr %.4f" % (r["auroc"], r["aupr"], r["fpr"]))
    assert np.isfinite([r["auroc"], r["aupr"], r["fpr"]]).all() and r["auroc"] > 0.5          # better than chance
    # prob="logit" with the reference's threshold: the gate stays shut on the negative distances, conf is the resized map
    scores, cos = __import__("models").evaluate_multiscale_rec(m, frames[0][0], frames[0][1], (72, 128))
    assert scores.max().item() <= 0.0
    conf = R.confidence(scores, cos, "rec")
    want = torch.nn.functional.interpolate(cos[:, None], size=(72, 128), mode="bilinear", align_corners=False)[0, 0]
    assert (conf - want).abs().max().item() <= RC.GPU_BAR
    # --ood msp is the maximum score itself, with and without the background class
    msp = R.evaluate(m, frames, 14, "msp", (13,), exclude_back=True)
    assert np.isfinite(msp["auroc"])
    assert torch.equal(R.confidence(scores, None, "msp"), scores.amax(1)[0])
    assert torch.equal(R.confidence(scores, None, "msp", exclude_back=True), scores[:, 1:].amax(1)[0])


# ----------------------------------------------------------------------------------------------------- the reader
def test_reader_takes_the_image_from_rec_dataset(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import utils
    from datasets.streethazards import StreetHazardsReader, resized_shapes
    rs = np.random.RandomState(21)
    root, rec_root = tmp_path / "data", tmp_path / "rec"
    for d in (root / "images" / "test" / "t5", root / "annotations" / "test" / "t5", rec_root / "t5"):
        os.makedirs(str(d))
    recs, want = [], []
    for i, (h, w) in enumerate(((72, 128), (64, 96))):
        img = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        segm = rs.randint(0, 15, (h, w)).astype(np.uint8)
        rh, rw = (h // 2, w // 2) if i == 1 else (h, w)               # the second reconstruction comes at half size
        rimg = rs.randint(0, 256, (rh, rw, 3), dtype=np.uint8)
        fi, fs = "images/test/t5/%d.png" % i, "annotations/test/t5/%d.png" % i
        Image.fromarray(img).save(str(root / fi))
        Image.fromarray(segm, mode="L").save(str(root / fs))
        Image.fromarray(rimg).save(str(rec_root / "t5" / ("%d.png" % i)))
        recs.append({"fpath_img": fi, "fpath_segm": fs, "height": h, "width": w})
        want.append((np.asarray(Image.fromarray(rimg).resize((w, h), Image.NEAREST)), segm, img))
    odgt = str(tmp_path / "test.odgt")
    with open(odgt, "w") as f:
        f.write(json.dumps(recs) + "\n")
    sizes, max_size = (48, 64), 160
    plain = StreetHazardsReader(str(root), odgt, img_sizes=sizes, img_max_size=max_size, workers=2)
    reader = StreetHazardsReader(str(root), odgt, img_sizes=sizes, img_max_size=max_size, workers=2, rec_dataset=str(rec_root))
    n = 0
    for (imgs, lab), (pimgs, plab), (rimg, segm, img) in zip(reader, plain, want):
        shapes = resized_shapes(rimg.shape[0], rimg.shape[1], sizes, max_size, 8)
        ref = utils.pil_resize_normalize(torch.tensor(rimg).cuda(), shapes)
        pref = utils.pil_resize_normalize(torch.from_numpy(img).cuda(), shapes)
        assert len(imgs) == len(ref) == 2
        for a, b, c, d in zip(imgs, ref, pimgs, pref):
            assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, c)
        assert torch.equal(lab, plab) and np.array_equal(lab.cpu().numpy(), segm.astype(np.int64) - 1)
        n += 1
    assert n == 2
