"""GPU: the open-set prediction and its threshold sweep -- dml_open_set_sweep (csrc/open_sweep.hip) through the C ABI, through
metrics.OpenSetSweepMetrics, utils.open_set_predict and the open-set driver's --open_set_thresholds.

Every comparison is exact integer equality with the numpy definition of tests/open_sweep_cases.py: there are no tolerances.  The
cube and open_pred sit between guard elements that must come back untouched.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import open_sweep_cases as OC

pytestmark = pytest.mark.gpu

GUARD = 64                       # int64 elements before and after each output
CUBE_GUARD, PRED_GUARD, PRED_FILL = -7, -9, -11


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    assert (_lib.OPEN_SWEEP_SPAN, _lib.OPEN_SWEEP_MAX_BLOCKS) == (OC.SPAN, OC.MAX_BLOCKS)
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a, offset=0):
    """a host array on the device behind `offset` elements: (buffer, pointer to the first element of the copy)"""
    t = torch.from_numpy(np.array(a))
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device="cuda")
    buf[offset:] = t.cuda()
    return buf, buf.data_ptr() + offset * t.element_size()


def run(lib, conf, pred, label, t, out, nc, u, want_cube=True, write_idx=None, cube0=None, calls=1, offset=0):
    """dml_open_set_sweep on host arrays -> (cube [nc, nc, T + 1] or None, open_pred [n] or None) as numpy.  `offset` moves every
    device pointer off its 16-byte boundary: conf by one float, the int64 arrays by one element."""
    n, T = conf.size, len(t)
    keep = [dev(conf, offset), dev(pred, offset), dev(label, offset)]
    n_cells = nc * nc * (T + 1)
    cbuf = torch.full((n_cells + 2 * GUARD + offset,), CUBE_GUARD, dtype=torch.int64, device="cuda")
    cbuf[GUARD + offset:GUARD + offset + n_cells] = 0 if cube0 is None else torch.from_numpy(np.array(cube0).ravel()).cuda()
    pbuf = torch.full((n + 2 * GUARD + offset,), PRED_GUARD, dtype=torch.int64, device="cuda")
    pbuf[GUARD + offset:GUARD + offset + n] = PRED_FILL
    tt = (C.c_float * T)(*[float(v) for v in t])
    oo = (C.c_int64 * max(1, len(out)))(*out)
    for _ in range(calls):
        rc = lib.dml_open_set_sweep(keep[0][1], keep[1][1], keep[2][1], n, tt, T, oo if out else None, len(out), nc, u,
                                    cbuf.data_ptr() + 8 * (GUARD + offset) if want_cube else None,
                                    pbuf.data_ptr() + 8 * (GUARD + offset) if write_idx is not None else None,
                                    0 if write_idx is None else write_idx, st())
        assert rc == 0, "dml_open_set_sweep returned %d" % rc
    torch.cuda.synchronize()
    cube, op = cbuf.cpu().numpy()[offset:], pbuf.cpu().numpy()[offset:]
    assert (cube[:GUARD] == CUBE_GUARD).all() and (cube[GUARD + n_cells:] == CUBE_GUARD).all(), "a guard element of cube was written"
    assert (op[:GUARD] == PRED_GUARD).all() and (op[GUARD + n:] == PRED_GUARD).all(), "a guard element of open_pred was written"
    cube, op = cube[GUARD:GUARD + n_cells].reshape(nc, nc, T + 1), op[GUARD:GUARD + n]
    if not want_cube:
        assert (cube == (0 if cube0 is None else cube0)).all(), "cube was written though it was not passed"
    if write_idx is None:
        assert (op == PRED_FILL).all(), "open_pred was written though it was not passed"
    for (buf, _), a in zip(keep, (conf, pred, label)):                  # the inputs are read only
        assert np.array_equal(buf.cpu().numpy()[offset:].view(np.uint8), np.array(a).view(np.uint8))
    return (cube if want_cube else None), (op if write_idx is not None else None)


def run_case(lib, name, **kw):
    c = OC.CASES[name]
    conf, pred, label, t = OC.inputs(name)
    return run(lib, conf, pred, label, t, c["out"], c["nc"], c["u"], **kw)


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_cube_equals_the_definition(lib, name):
    c = OC.CASES[name]
    conf, pred, _, t = OC.inputs(name)
    w = len(t) // 2
    cube, op = run_case(lib, name, write_idx=w)                          # both outputs from one call
    assert np.array_equal(cube, OC.reference(name))
    assert np.array_equal(op, OC.open_pred_ref(conf, pred, t[w], c["u"]))
    only, none = run_case(lib, name)                                     # open_pred NULL leaves no trace
    assert none is None and np.array_equal(only, cube)


def test_every_write_idx_and_the_prediction_alone(lib):
    for name in ("T3", "pred_oob"):                                      # an out-of-range prediction is skipped in the cube, written here
        c = OC.CASES[name]
        conf, pred, label, t = OC.inputs(name)
        for w in range(3):
            cube, op = run_case(lib, name, write_idx=w)
            assert np.array_equal(op, OC.open_pred_ref(conf, pred, t[w], c["u"])) and np.array_equal(cube, OC.reference(name))
            none, alone = run_case(lib, name, want_cube=False, write_idx=w)          # cube NULL: the header allows it
            assert none is None and np.array_equal(alone, op)
    assert ((pred < 0) | (pred >= c["nc"])).sum() > 100


def test_accumulation_and_the_64_bit_flush(lib):
    name = "T9_k14_last"
    ref = OC.reference(name)
    twice, _ = run_case(lib, name, calls=2)
    assert np.array_equal(twice, 2 * ref)
    big = np.zeros_like(ref)
    l, q, j = np.unravel_index(np.argmax(ref), ref.shape)
    big[l, q, j] = 2 ** 33
    big[0, 0, 0] = 2 ** 40 + 5
    got, _ = run_case(lib, name, cube0=big)
    assert ref[l, q, j] > 0 and np.array_equal(got, ref + big)
    # a second frame of another size into the same cube
    c = OC.CASES[name]
    conf, pred, label, t = OC.inputs("n300007")
    other = OC.cube_ref(conf, pred, label, OC.thresholds_for(9), c["out"], c["nc"], c["u"])
    got2, _ = run(lib, conf, pred, label, OC.thresholds_for(9), c["out"], c["nc"], c["u"], cube0=ref)
    assert np.array_equal(got2, ref + other)


def test_one_cell_takes_every_pixel(lib):
    """all pixels alike: a single LDS counter takes a workgroup's whole share"""
    c = OC.CASES["const"]
    n = 3 * OC.SPAN * OC.MAX_BLOCKS + 11                                 # three passes per workgroup
    conf = np.full(n, 0.55, np.float32)
    pred, label = np.full(n, 3, np.int64), np.full(n, 5, np.int64)
    cube, _ = run(lib, conf, pred, label, OC.thresholds_for(9), c["out"], c["nc"], c["u"])
    want = np.zeros_like(cube)
    want[5, 3, 5] = n                                                    # 0.55 passes 0.1 ... 0.5
    assert np.array_equal(cube, want)


@pytest.mark.parametrize("name", ["n65", "n2049", "T12_k33_middle", "pred_oob"])
def test_pointers_at_the_promised_alignment(lib, name):
    """4 bytes for conf, 8 for the int64 arrays: every pointer one element past a 16-byte boundary"""
    c = OC.CASES[name]
    conf, pred, _, t = OC.inputs(name)
    cube, op = run_case(lib, name, write_idx=0, offset=1)
    assert np.array_equal(cube, OC.reference(name)) and np.array_equal(op, OC.open_pred_ref(conf, pred, t[0], c["u"]))


def test_misaligned_pointers_are_refused(lib):
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    t = (C.c_float * 1)(0.5)
    p = z.data_ptr()
    for k in range(5):
        ptrs = [p, p, p, p, p]
        ptrs[k] += 2 if k == 0 else 4
        assert lib.dml_open_set_sweep(ptrs[0], ptrs[1], ptrs[2], 4, t, 1, None, 0, 2, 1, ptrs[3], ptrs[4], 0, st()) == -2
    torch.cuda.synchronize()
    assert (z == 0).all()


def _updates():
    """three frames of different sizes for one meter: (label, pred, conf) numpy triples and the meter's settings"""
    c = OC.CASES["T9_k14_last"]
    frames = [OC.inputs(n) for n in ("T9_k14_last", "n300007", "n65")]
    return c, OC.thresholds_for(9), [(f[2], f[1], f[0]) for f in frames]


def test_metrics_class(lib):
    import metrics
    c, t, frames = _updates()
    nc, u = c["nc"], c["u"]
    m = metrics.OpenSetSweepMetrics(nc, t, u, c["out"])
    s = metrics.StreamSegMetrics(nc)
    cube = np.zeros((nc, nc, len(t) + 1), np.int64)
    for k, (label, pred, conf) in enumerate(frames):
        lt, lp, cf = (torch.from_numpy(np.array(a)).cuda() for a in (label, pred, conf))
        if k == 1:
            # an odd view: one element into a larger buffer, [1, n] against [n]
            lt, lp, cf = (torch.cat([x[:1], x])[1:] for x in (lt, lp, cf))
            assert lt.data_ptr() % 16 == 8 and cf.data_ptr() % 16 == 4
            lt = lt[None]
        m.update(lt, lp, cf)
        s.update(torch.from_numpy(OC.remap(label, c["out"], u)).cuda(), lp.reshape(-1))
        cube += OC.cube_ref(conf, pred, label, t, c["out"], nc, u)
    assert m.cube.dtype == torch.int64 and m.cube.is_cuda and np.array_equal(m.cube.cpu().numpy(), cube)
    res = m.get_results()
    closed = s.get_results()["Mean IoU"]
    for i in range(len(t)):
        want_m = OC.matrix_from_cube(cube, i, u)
        assert np.array_equal(m.confusion(i), want_m)
        want = OC.results_ref(want_m, u)
        for k, v in want.items():
            assert abs(res[i][k] - v) <= 1e-12, (i, k, res[i][k], v)
        assert abs(res[i]["Closed Mean IoU"] - closed) <= 1e-12
    assert len(set(r["Mean IoU"] for r in res)) > 1                      # the thresholds tell the frames apart
    m.reset()
    assert m.cube is not None and int(m.cube.abs().sum()) == 0 and m.confusion(0).sum() == 0
    with pytest.raises(ValueError):
        m.update(lt, lp[:5], cf)
    with pytest.raises(TypeError):
        m.update(lt, lp, cf.double())
    with pytest.raises(TypeError):
        m.update(lt.int(), lp, cf)
    assert int(m.cube.abs().sum()) == 0


def test_open_set_predict():
    import utils
    g = H.rng_for(43, "open_set_predict")
    conf = g.random((2, 37, 53), dtype=np.float32)
    conf[0, 0, :7] = [np.nan, np.inf, -np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                      np.nextafter(np.float32(0.5), np.float32(1)), 0.0]
    preds = g.integers(0, 13, (2, 37, 53)).astype(np.int64)
    cf, pr = torch.from_numpy(conf).cuda(), torch.from_numpy(preds).cuda()
    for t, u in ((0.5, 13), (0.8, 19), (0.0, 0)):
        out = utils.open_set_predict(cf, pr, t, u)
        assert out.shape == pr.shape and out.dtype == torch.int64 and out.is_cuda
        assert torch.equal(out, torch.where(cf >= t, pr, torch.full_like(pr, u)))
    assert (utils.open_set_predict(cf, pr, 0.5, 13)[0, 0, :7].cpu().tolist()
            == [13, int(preds[0, 0, 1]), 13, int(preds[0, 0, 3]), 13, int(preds[0, 0, 5]), 13])
    # a view that is not contiguous, and one that starts 4 / 8 bytes into its buffer
    out = utils.open_set_predict(cf.transpose(1, 2), pr.transpose(1, 2), 0.5, 13)
    assert torch.equal(out, torch.where(cf >= 0.5, pr, torch.full_like(pr, 13)).transpose(1, 2))
    out = utils.open_set_predict(cf.flatten()[1:], pr.flatten()[1:], 0.5, 13)
    assert torch.equal(out, torch.where(cf >= 0.5, pr, torch.full_like(pr, 13)).flatten()[1:])
    assert torch.equal(pr.cpu(), torch.from_numpy(preds))                # the input is not touched
    with pytest.raises(TypeError):
        utils.open_set_predict(cf.double(), pr, 0.5, 13)
    with pytest.raises(ValueError):
        utils.open_set_predict(cf, pr[:1], 0.5, 13)


def _tiny_frames(seg_size=(96, 128), n=2):
    g = torch.Generator().manual_seed(11)
    out = []
    for _ in range(n):
        imgs = [torch.randn(1, 3, h, w, generator=g).cuda() for h, w in ((96, 128), (120, 160))]
        lab = torch.randint(0, 14, (seg_size[0] // 8, seg_size[1] // 8), generator=g)
        lab = lab.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()
        lab[:3] = 255
        out.append((imgs, lab.cuda()))
    return out


def test_driver_evaluate_returns_the_sweep():
    import eval_ood_traditional as T
    import metrics
    import models
    import utils
    torch.manual_seed(304)
    enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048, weights="")
    dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, weights="", use_softmax=True)
    seg = models.SegmentationModuleOOD(enc, dec, None).cuda().eval()
    seg.set_compute_dtype(torch.float32, fp32_products="exact")
    frames = _tiny_frames()
    base = T.evaluate(seg, frames, 14, "dissum", (13,))
    assert "open_set" not in base
    got = T.evaluate(seg, frames, 14, "dissum", (13,), open_set_thresholds=(0.25, 0.5))
    assert set(got) == set(base) | {"open_set"}
    for k in ("auroc", "aupr", "fpr"):
        assert got[k] == base[k] or (np.isnan(got[k]) and np.isnan(base[k])), k
    assert np.array_equal(got["known_iou"], base["known_iou"])
    for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
        np.testing.assert_array_equal(got["seg"][k], base["seg"][k])
    np.testing.assert_array_equal(np.array(list(got["seg"]["Class IoU"].values())),
                                  np.array(list(base["seg"]["Class IoU"].values())))
    # the class fed by hand with the driver's own pred / conf / label
    m = metrics.OpenSetSweepMetrics(14, (0.25, 0.5), 13, (13,))
    for imgs, lab in frames:
        scores, ft1 = models.evaluate_multiscale(seg, imgs, tuple(lab.shape))
        m.update(lab, utils.argmax_msp(scores)[0], T.confidence(scores, "dissum", False, feats=ft1))
    want = m.get_results()
    assert len(got["open_set"]) == 2 and [r["Threshold"] for r in want] == [0.25, 0.5]
    for a, b in zip(got["open_set"], want):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    assert m.confusion(1).sum() == 2 * (96 - 3) * 128                    # the ignored rows are skipped
    assert got["open_set"][0]["Closed Mean IoU"] == pytest.approx(base["seg"]["Mean IoU"], abs=1e-12)


def test_open_set_evaluation_driver_with_thresholds():
    """eval_ood_traditional.py --synthetic --ood dissum --open_set_thresholds 0.1 0.5 0.9 end to end at a small frame size, in a
    child process"""
    drv = os.path.join(H.PKG, "eval_ood_traditional.py")
    r = subprocess.run([sys.executable, drv, "--synthetic", "--ood", "dissum", "--open_set_thresholds", "0.1", "0.5", "0.9",
                        "--num_images", "1", "--height", "360", "--width", "640", "--dtype", "bf16"], capture_output=True, text=True,
                       cwd=H.PKG, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean auroc = " in r.stdout and "Mean IoU:" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("threshold ")]
    assert len(lines) == 3 and [float(ln.split()[1].rstrip(":")) for ln in lines] == [0.1, 0.5, 0.9], r.stdout[-2000:]
    assert "Best open-set Mean IoU:" in r.stdout.split(lines[-1])[1]
