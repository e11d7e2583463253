"""CPU: the float64 distillation-term definition of tests/distill_cases.py IS the reference's utils/loss.py:106-117 with the fill of
main_distillation.py:428-430, its inputs meet the conditions the GPU tests rely on, and its bars separate the likely mistakes
from the right answer -- the conditions that keep tests/test_gpu_distill_loss.py from hiding a failure.

The reference's statements (n, w, h of a square crop; `16` is the student's extra class; 0.01 its coefficient):
    appendix_lay = torch.zeros(n, w, h, 1).cuda()
    features_1 = torch.cat((features_1, appendix_lay), dim=3)
    for i in range(n):
        features_origin = features_1[i][target[i] != 16]
        features_new = features_2[i][target[i] != 16]
        features_diff = features_new - features_origin
        DIS_loss += torch.sum(features_diff ** 2) / (features_diff.shape[0])
    loss = CE_loss / n + 0.01 * DIS_loss / n
and in the driver
    preds = outputs.detach().max(dim=1)[1]
    labels[labels == 255] = preds[labels == 255]
"""
import numpy as np
import pytest
import torch

import distill_cases as DC

F64 = np.float64
CELLS = [(shape, ch) for shape in DC.SHAPES for ch in DC.CHANNELS]


def torch_statements(t, s, labels, novel_id, dtype, t_logits=None):
    """-> (DIS_loss / n, its autograd gradient on features_2, the labels after the driver's fill)"""
    f1 = torch.from_numpy(np.array(t)).to(dtype)
    f2 = torch.from_numpy(np.array(s)).to(dtype).requires_grad_(True)
    target = torch.from_numpy(np.array(labels))
    if t_logits is not None:
        preds = torch.from_numpy(np.array(t_logits)).max(dim=1)[1]
        target[target == 255] = preds[target == 255]
    n, h, w, cs = f2.shape
    if cs > f1.shape[3]:
        appendix_lay = torch.zeros(n, h, w, cs - f1.shape[3], dtype=dtype)
        f1 = torch.cat((f1, appendix_lay), dim=3)
    DIS_loss = torch.zeros(1, dtype=dtype)
    for i in range(n):
        features_origin = f1[i][target[i] != novel_id]
        features_new = f2[i][target[i] != novel_id]
        features_diff = features_new - features_origin
        DIS_loss = DIS_loss + torch.sum(features_diff ** 2) / (features_diff.shape[0])
    loss = DIS_loss / n
    loss.backward()
    return loss.detach().double().item(), f2.grad.double().numpy(), target.numpy()


@pytest.mark.parametrize("with_fill", (False, True))
@pytest.mark.parametrize("shape,ch", CELLS)
def test_definition_is_the_references_statements_in_float64(shape, ch, with_fill):
    t, s, lab, lg = DC.inputs(shape, ch)
    lgs = lg if with_fill else None
    ref = DC.distill_ref(t, s, lab, DC.novel_of(ch[0]), DC.IGNORE, t_logits=lgs)
    dis, grad, filled = torch_statements(t, s, lab, DC.novel_of(ch[0]), torch.float64, t_logits=lgs)
    assert np.array_equal(filled, ref["labels"])
    if with_fill:
        assert not (filled == DC.IGNORE).any()
    if (ref["cnt"] == 0).any():
        assert np.isnan(dis)                       # the reference's 0 / 0; the definition: contribution 0, gradient 0
        assert np.isfinite(ref["dis"]) and not ref["grad"][ref["cnt"] == 0].any()
        return
    assert abs(dis - ref["dis"]) <= 1e-12 * max(1.0, abs(ref["dis"]))
    assert np.abs(grad - ref["grad"]).max() <= 1e-12 * max(1.0, np.abs(ref["grad"]).max())


@pytest.mark.parametrize("shape,ch", CELLS)
def test_float32_torch_lies_inside_the_bars(shape, ch):
    """the reference's own float32 evaluation: its sums run in another order, but within the same chain-depth model"""
    t, s, lab, lg = DC.inputs(shape, ch)
    ref = DC.distill_ref(t, s, lab, DC.novel_of(ch[0]), DC.IGNORE, t_logits=lg)
    dis, grad, _ = torch_statements(t, s, lab, DC.novel_of(ch[0]), torch.float32, t_logits=lg)
    if (ref["cnt"] == 0).any():
        assert np.isnan(dis)                       # the reference divides by zero on an image without masked-in pixels
        return
    err = np.abs(grad - ref["grad"])
    pos = ref["grad_bar"] > 0
    print("MEASURE %s %s float32 torch: dis err/bar=%.3f, worst gradient err/bar=%.3f"
          % (shape, ch, abs(dis - ref["dis"]) / ref["dis_bar"], (err[pos] / ref["grad_bar"][pos]).max(initial=0.0)))
    # torch rounds d, d / cnt and that / n: three eps32, inside the gradient's four.  Its dis takes S_i / cnt_i, their sum and
    # the division by n in float32 where the kernels fold in double: three more eps32 on dis
    assert (err <= ref["grad_bar"]).all() and (grad[~pos] == 0).all()
    assert abs(dis - ref["dis"]) <= ref["dis_bar"] + 3 * DC.EPS32 * abs(ref["dis"])


@pytest.mark.parametrize("ch", DC.CHANNELS)
def test_inputs_meet_their_conditions(ch):
    t, s, lab, lg = DC.inputs(DC.SPREAD_SHAPE, ch)
    novel, ign = (lab == DC.novel_of(ch[0])).mean(), (lab == DC.IGNORE).mean()
    top = lg.max(axis=1, keepdims=True)
    tied = ((lg == top).sum(axis=1) > 1) & (lab == DC.IGNORE)
    first = lg.argmax(axis=1)
    last = lg.shape[1] - 1 - lg[:, ::-1].argmax(axis=1)
    print("MEASURE %s novel %.3f ignored %.3f, ignored pixels with a tied maximum %d" % (ch, novel, ign, tied.sum()))
    assert 0.15 <= novel <= 0.30 and 0.10 <= ign <= 0.20
    if ch[0] > 1:
        assert tied.sum() >= 10 and (first != last)[lab == DC.IGNORE].sum() >= 10    # a last-maximum rule would be seen
    assert (s[..., ch[0]:] != 0).all() and (s[..., :ch[0]] != t).any()
    # the smallest cases keep a masked-in pixel wherever the GPU test needs a finite reference value
    for shape in DC.SHAPES[1:]:
        assert (DC.distill_ref(*DC.inputs(shape, ch)[:3], DC.novel_of(ch[0]))["cnt"] > 0).all()


@pytest.mark.parametrize("with_fill", (False, True))
@pytest.mark.parametrize("ch", DC.CHANNELS)
def test_bars_separate_the_mutants(ch, with_fill):
    """each likely mistake is at least 100 bars away: in dis where it changes dis, and on at least half of the gradient elements
    it changes"""
    t, s, lab, lg = DC.inputs(DC.SPREAD_SHAPE, ch)
    lgs = lg if with_fill else None
    novel = DC.novel_of(ch[0])
    ref = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=lgs)
    for what in DC.MUTANTS:
        if what == "padded channel unpenalised" and ch[0] == ch[1]:
            continue                                                # no padded channel
        if what == "ignored pixels masked out" and with_fill:
            continue                                                # no ignored pixel is left after the fill
        mut = DC.distill_ref(t, s, lab, novel, DC.IGNORE, t_logits=lgs, mutant=what)
        off = abs(mut["dis"] - ref["dis"]) / ref["dis_bar"]
        changed = mut["grad"] != ref["grad"]
        ratio = np.abs(mut["grad"] - ref["grad"])[changed] / np.maximum(ref["grad_bar"][changed], DC.STEP32)
        print("MEASURE %s fill=%s %s: dis off by %.0f bars, %d gradient elements changed, median %.0f bars"
              % (ch, with_fill, what, off, changed.sum(), np.median(ratio)))
        if what != "factor 2 dropped":
            assert off >= 100
        assert changed.sum() > 0 and (ratio >= 100).mean() >= 0.5


def test_an_image_without_masked_in_pixels():
    """cnt_i = 0: contribution 0, gradient 0, bars 0 -- and nothing NaN anywhere else"""
    t, s, lab, _ = DC.inputs((2, 5, 7), (16, 17))
    lab = np.array(lab)
    lab[0] = 16
    ref = DC.distill_ref(t, s, lab, 16)
    one = DC.distill_ref(t[1:], s[1:], lab[1:], 16, n=2)
    assert ref["cnt"][0] == 0 and ref["S"][0] == 0 and not ref["grad"][0].any() and not ref["grad_bar"][0].any()
    assert ref["dis"] == one["dis"] and np.array_equal(ref["grad"][1], one["grad"][0])
    assert np.isfinite(ref["dis"]) and np.isfinite(ref["grad"]).all()
