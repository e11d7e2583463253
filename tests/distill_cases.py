"""The feature-distillation term of the reference's utils/loss.py:104-117 (with the fill of main_distillation.py:428-430) as a
float64 definition on float32 inputs, the bars the HIP kernels (csrc/distill_loss.hip) are held to, and the case table.
tests/test_distill_refs.py proves the definition against the reference's statements without a GPU;
tests/test_gpu_distill_loss.py holds the kernels to it.

Definition.  t [B,H,W,Ct] teacher features, s [B,H,W,Cs] student features, pad(t) = t with Cs - Ct zero channels appended,
labels [B,H,W]; with teacher logits [B,Ct,H,W] an ignored label is first replaced by the first maximal class of its pixel.
A pixel is masked in when its (filled) label != novel_id.  Per image i, over its masked-in pixels and all Cs channels,
    d = s - pad(t)      S_i = sum d^2      cnt_i = #masked-in pixels
    dis = (1 / n) sum_{i: cnt_i > 0} S_i / cnt_i            d dis / d s = gout 2 / (n cnt_i) d   (0 on a masked-out pixel)
An image with cnt_i = 0 contributes 0 and has a zero gradient (the reference: 0 / 0 = NaN).

Bars (eps32 = 2^-24), from the roundings a float32 evaluation makes, not from any output of the kernels:
    d:         one rounding of the subtraction, eps32 |d| (none in a pad channel)
    d^2:       2 eps32 d^2 from d and one more for the product: 3 eps32 d^2
    S_i:       the terms pass through a chain of float32 additions before the double fold -- four per group a lane takes
               (chain_depth below: the launch shapes documented in include/dmlnet_hip.h and DESIGN.md 7j), six in the wave's
               butterfly and three across the waves; each addition rounds at most eps32 of a partial sum that is at most S_i.
               bar_S_i = (4 + depth) eps32 S_i, one eps32 spare for the second-order terms
    dis:       sum_i bar_S_i / cnt_i / n, plus eps32 |dis| for its float32 store
    gradient:  w = float32(gout 2 / (n cnt_i)), d and the product round once each: 4 eps32 |g| with one spare, plus float32's
               step below 2^-126 (2^-149) where the bar is not 0
An element whose bar is 0 (masked-out pixels, s = t exactly) must be exactly 0.
"""
import functools

import numpy as np

import helpers as H

F64 = np.float64
EPS32 = 2.0 ** -24
STEP32 = 2.0 ** -149
DISTILL_BLOCKS = 2048                            # workgroups of the forward at most (block_partials: 2 floats each)


def chain_depth(B, Hh, Ww, Cs):
    """float32 additions a term of S_i passes through at most, the larger of the two launch shapes of dml_distill_fwd: without
    teacher logits a workgroup strides over the image's groups, with them over its tiles of 256 pixels (64 Cs groups)"""
    groups = (Hh * Ww * Cs + 3) // 4
    bpi = max(1, min((groups + 255) // 256, DISTILL_BLOCKS // B))
    flat = (groups + 256 * bpi - 1) // (256 * bpi)
    tiles = (Hh * Ww + 255) // 256
    bpi = max(1, min(tiles, DISTILL_BLOCKS // B))
    tiled = ((tiles + bpi - 1) // bpi) * ((64 * Cs + 255) // 256)
    return 4 * max(flat, tiled) + 6 + 3


def make_inputs(name, B, Hh, Ww, Ct, Cs, novel_id, ignore_index, seed=17):
    """teacher features 3 e_k + noise (the embedding's prototypes), student = pad(teacher) + 0.5 noise with pad channels of
    N(0, 1), both wider on novel and ignored pixels; labels: about 22 % novel_id, 15 % ignore_index, the rest uniform in [0, Ct); teacher logits quantised to steps of
    1/2 so that the maximum is tied on many pixels."""
    g = H.rng_for(seed, "distill." + name)
    k = g.integers(0, Ct, size=(B, Hh, Ww))
    t = g.standard_normal((B, Hh, Ww, Ct)) + 3.0 * (np.arange(Ct)[None, None, None, :] == k[..., None])
    t = t.astype(np.float32)
    s = np.zeros((B, Hh, Ww, Cs))
    s[..., :Ct] = t
    r = g.random((B, Hh, Ww))
    lab = g.integers(0, Ct, size=(B, Hh, Ww)).astype(np.int64)
    lab[r < 0.22] = novel_id
    lab[(r >= 0.22) & (r < 0.37)] = ignore_index
    # the student strays further from the teacher where the teacher was never taught: x 2 on the novel pixels, x 1.5 on the
    # ignored ones -- a mask that takes one pixel class for another then moves the mean, not only its sampling noise
    far = np.where(lab == novel_id, 2.0, np.where(lab == ignore_index, 1.5, 1.0))[..., None]
    s += far * np.where(np.arange(Cs) < Ct, 0.5, 1.0) * g.standard_normal((B, Hh, Ww, Cs))
    lg = (np.round(2.0 * g.standard_normal((B, Ct, Hh, Ww))) / 2.0).astype(np.float32)
    return t, np.ascontiguousarray(s.astype(np.float32)), lab, lg


def fill(labels, t_logits, ignore_index):
    """labels with the ignored ones replaced by the first maximal class of the teacher's logits"""
    if t_logits is None:
        return labels
    return np.where(labels == ignore_index, t_logits.argmax(axis=1).astype(np.int64), labels)     # numpy: the first maximum


def distill_ref(t, s, labels, novel_id, ignore_index=255, t_logits=None, gout=1.0, n=None, mutant=None):
    """The definition and its bars -> dict(dis, dis_bar, S, S_bar, cnt, grad, grad_bar, labels, sums).  `mutant` names a likely
    mistake, for tests/test_distill_refs.py only."""
    B, Hh, Ww, Cs = s.shape
    Ct = t.shape[3]
    n = float(B if n is None else n)
    lab = fill(labels, t_logits, ignore_index)
    mask = lab != novel_id
    if mutant == "novel pixels not masked out":
        mask = np.ones_like(mask)
    if mutant == "ignored pixels masked out":
        mask = mask & (labels != ignore_index)
    pad = np.zeros((B, Hh, Ww, Cs), dtype=F64)
    pad[..., :Ct] = t.astype(F64)
    d = (s.astype(F64) - pad) * mask[..., None]
    if mutant == "padded channel unpenalised":
        d[..., Ct:] = 0.0
    S = (d * d).sum(axis=(1, 2, 3))
    cnt = mask.sum(axis=(1, 2)).astype(F64)
    div = np.full(B, float(Hh * Ww)) if mutant == "divisor H W" else cnt
    ok = cnt > 0
    safe = np.where(ok, div, 1.0)
    nn = 1.0 if mutant == "1/n dropped" else n
    two = 1.0 if mutant == "factor 2 dropped" else 2.0
    dis = (np.where(ok, S / safe, 0.0)).sum() / nn
    w = np.where(ok, gout * two / (nn * safe), 0.0)
    grad = w[:, None, None, None] * d
    depth = chain_depth(B, Hh, Ww, Cs)
    S_bar = (4 + depth) * EPS32 * S
    dis_bar = np.where(ok, S_bar / safe, 0.0).sum() / nn + EPS32 * abs(dis)
    grad_bar = 4 * EPS32 * np.abs(grad)
    grad_bar = np.where(grad_bar > 0, grad_bar + STEP32, 0.0)
    sums = np.zeros(2 * B + 2, dtype=F64)
    sums[0:2 * B:2], sums[1:2 * B:2] = S, cnt
    sums[2 * B], sums[2 * B + 1] = np.where(ok, S / safe, 0.0).sum(), B
    total_bar = np.where(ok, S_bar / safe, 0.0).sum()
    return dict(dis=dis, dis_bar=dis_bar, S=S, S_bar=S_bar, cnt=cnt, grad=grad, grad_bar=grad_bar, labels=lab, mask=mask,
                sums=sums, total_bar=total_bar)


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 1), (2, 5, 7), (3, 33, 65), (2, 64, 64))      # one pixel; odd; H W Cs % 4 != 0 for odd Cs, several workgroups
CHANNELS = ((16, 17), (16, 16), (1, 2), (31, 32), (3, 8))      # the driver's; no pad; the narrowest; the widest; several pad channels
IGNORE = 255
SPREAD_SHAPE = (2, 24, 33)                                      # 1584 pixels: fractions of enough pixels to mean something
MUTANTS = ("divisor H W", "novel pixels not masked out", "padded channel unpenalised", "ignored pixels masked out",
           "factor 2 dropped", "1/n dropped")


def novel_of(Ct):
    """the student's extra class: the driver's 16 for 16 teacher classes"""
    return Ct


@functools.lru_cache(maxsize=None)
def inputs(shape, channels):
    B, Hh, Ww = shape
    Ct, Cs = channels
    out = make_inputs("%dx%dx%d.%d-%d" % (B, Hh, Ww, Ct, Cs), B, Hh, Ww, Ct, Cs, novel_of(Ct), IGNORE)
    for a in out:
        a.setflags(write=False)
    return out
