"""CPU: the float64 focal-loss definition of tests/focal_cases.py IS the reference's utils/loss.py:7-23, its inputs spread
over the saturated and unsaturated pixels, and its bars separate the likely mistakes from the right answer -- the conditions
that keep tests/test_gpu_focal_loss.py from hiding a failure.

The reference's five statements, evaluated with torch:
    ce_loss = F.cross_entropy(inputs, targets, reduction='none', ignore_index=self.ignore_index)
    pt = torch.exp(-ce_loss)
    focal_loss = self.alpha * (1 - pt) ** self.gamma * ce_loss
    return focal_loss.mean()        (size_average)
    return focal_loss.sum()         (otherwise)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_cases as FC

F64 = np.float64


def torch_statements(logits, labels, alpha, gamma, size_average, ignore_index, dtype):
    x = torch.from_numpy(np.array(logits)).to(dtype).requires_grad_(True)
    y = torch.from_numpy(np.array(labels))
    ce_loss = F.cross_entropy(x, y, reduction="none", ignore_index=ignore_index)
    pt = torch.exp(-ce_loss)
    focal_loss = alpha * (1 - pt) ** gamma * ce_loss
    loss = focal_loss.mean() if size_average else focal_loss.sum()
    loss.backward()
    return loss.detach().double().item(), x.grad.double().numpy()


SPREAD = [(K, ign) for K in FC.SPREAD_CLASSES for ign in FC.IGNORES]


@pytest.mark.parametrize("K,ignore_index", SPREAD)
def test_inputs_cover_saturated_and_unsaturated_pixels(K, ignore_index):
    lg, lab = FC.inputs(K, FC.SPREAD_SHAPE, ignore_index)
    u = FC.focal_ref(lg, lab, 1.0, 2.0, True, ignore_index)["u"]
    mid, low, high = ((u > 1e-3) & (u < 0.999)).mean(), (u < 1e-3).mean(), (u > 0.999).mean()
    print("MEASURE K=%d ignore=%d valid=%d  1e-3<u<0.999: %.3f  u<1e-3: %.3f  u>0.999: %.3f"
          % (K, ignore_index, u.size, mid, low, high))
    assert mid >= 0.30 and low >= 0.10 and high >= 0.05
    assert 0.10 < (lab == ignore_index).mean() < 0.20


@pytest.mark.parametrize("gamma", (0.5, 2.0))
@pytest.mark.parametrize("K,ignore_index", SPREAD)
def test_bars_separate_the_mutants(K, ignore_index, gamma):
    """gamma ignored, alpha dropped, and the valid count as divisor: each is at least 100 loss bars away where it changes the
    loss, and more than 50 bars away on at least half of the nonzero gradient elements"""
    lg, lab = FC.inputs(K, FC.SPREAD_SHAPE, ignore_index)
    ref = FC.focal_ref(lg, lab, 0.25, gamma, True, ignore_index)
    mutants = {"gamma ignored": FC.focal_ref(lg, lab, 0.25, 0.0, True, ignore_index),
               "alpha dropped": FC.focal_ref(lg, lab, 1.0, gamma, True, ignore_index),
               "divided by the valid count": FC.focal_ref(lg, lab, 0.25, gamma, True, ignore_index, divide_by_valid=True)}
    nz = ref["grad"] != 0
    for what, mut in mutants.items():
        off = abs(mut["loss"] - ref["loss"]) / ref["loss_bar"]
        ratio = np.abs(mut["grad"] - ref["grad"])[nz] / ref["grad_bar"][nz]
        print("MEASURE K=%d gamma=%g %s: loss off by %.0f bars, gradient median %.0f bars" % (K, gamma, what, off, np.median(ratio)))
        assert mut["loss"] != ref["loss"] and off >= 100
        assert (ratio > 50).mean() >= 0.5


CELLS = [(K, shape) for K in FC.CLASSES for shape in sorted(FC.SHAPES)]


@pytest.mark.parametrize("K,shape", CELLS)
def test_definition_is_the_references_statements_in_float64(K, shape):
    for s in FC.settings(K, shape):
        lg, lab = FC.inputs(K, shape, s["ignore_index"])
        ref = FC.focal_ref(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"])
        loss, grad = torch_statements(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], torch.float64)
        assert abs(loss - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"])), (s, loss, ref["loss"])
        fin = np.isfinite(grad)
        assert np.abs(grad - ref["grad"])[fin].max(initial=0.0) <= 1e-12, s
        if not (0 < s["gamma"] < 1):
            assert fin.all(), s


@pytest.mark.parametrize("K,shape", CELLS)
def test_float32_torch_lies_inside_the_bars(K, shape):
    """... wherever it is finite; for 0 < gamma < 1 its gradient has NaN elements (inf * 0 where pt rounds to 1), counted here"""
    worst_l = worst_g = 0.0
    nan_total = 0
    for s in FC.settings(K, shape):
        lg, lab = FC.inputs(K, shape, s["ignore_index"])
        ref = FC.focal_ref(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"])
        loss, grad = torch_statements(lg, lab, s["alpha"], s["gamma"], s["size_average"], s["ignore_index"], torch.float32)
        fin = np.isfinite(grad)
        nan_total += (~fin).sum()
        if not (0 < s["gamma"] < 1):
            assert fin.all(), s
        err = np.abs(grad - ref["grad"])
        assert (err[fin] <= ref["grad_bar"][fin]).all(), (s, (err[fin] / np.maximum(ref["grad_bar"][fin], 1e-300)).max())
        pos = fin & (ref["grad_bar"] > 0)
        worst_g = max(worst_g, (err[pos] / ref["grad_bar"][pos]).max(initial=0.0))
        assert abs(loss - ref["loss"]) <= ref["loss_bar"], (s, loss, ref["loss"], ref["loss_bar"])
        if ref["loss_bar"] > 0:
            worst_l = max(worst_l, abs(loss - ref["loss"]) / ref["loss_bar"])
    print("MEASURE K=%d %s float32 torch: worst loss err/bar=%.3f, worst gradient err/bar=%.3f, %d NaN gradient elements"
          % (K, shape, worst_l, worst_g, nan_total))
    if K >= 13 and shape != "px":
        assert nan_total > 0, "the reference's NaN gradients for 0 < gamma < 1 are expected on these inputs"


def test_limits_and_edge_frame():
    """u = 0: fl = 0, m = alpha for gamma = 0 and 0 for gamma > 0; u^0 = 1; the hand-built pixels have the ce they claim"""
    assert FC.fl_of(0.0, 0.25, 0.0) == 0.0 and FC.m_of(0.0, 0.25, 0.0) == 0.25
    for gamma in (0.5, 1.0, 2.0, 5.0):
        assert FC.fl_of(0.0, 0.25, gamma) == 0.0 and FC.m_of(0.0, 0.25, gamma) == 0.0
    lg, lab = FC.edge_frame()
    ce = FC.focal_ref(lg, lab, 1.0, 2.0, True, 255)["ce"]
    for row in range(2):
        assert ce[0, row, 0] == 0.0
        assert abs(ce[0, row, 1] - 1e-7) < 1e-12 and abs(ce[0, row, 2] - 50.0) < 1e-12 and abs(ce[0, row, 3] - 90.0) < 1e-12
    for gamma in FC.GAMMAS:
        ref = FC.focal_ref(lg, lab, 0.25, gamma, False, 255)
        assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"]) and np.isfinite(ref["grad_bar"]).all()
    # an all-ignored batch: loss 0, gradient 0, bars 0
    ref = FC.focal_ref(lg, np.full_like(lab, 255), 0.25, 2.0, True, 255)
    assert ref["loss"] == 0.0 and ref["loss_bar"] == 0.0 and not ref["grad"].any() and not ref["grad_bar"].any()
