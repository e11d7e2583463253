"""The focal loss of the reference's utils/loss.py:7-23 as a float64 definition on float32 inputs, the bars the HIP kernels
(csrc/focal_loss.hip) are held to, and the case table.  tests/test_focal_refs.py proves the definition against the
reference's statements without a GPU; tests/test_gpu_focal_loss.py holds the kernels to it.

Definition, per valid pixel (label != ignore_index):
    ce = logsumexp_k L_k - L_y    pt = exp(-ce)    u = 1 - pt    fl = alpha u^gamma ce
    m  = alpha (u^gamma + gamma pt ce u^(gamma-1))                d fl / d L_k = m (softmax_k - [k = y])
fl = 0 and a zero gradient on an ignored pixel.  Where u = 0: fl = 0, m = alpha for gamma = 0 and 0 for gamma > 0 (the
analytic limit: ce ~ u, so pt ce u^(gamma-1) -> u^gamma); u^0 = 1 for every u.  loss = sum fl / (B H W) -- the ignored pixels
counted -- with size_average, sum fl without.

Bars (eps32 = 2^-24):
    E_ce   = eps32 (2 ce + K + 4)              one rounding of max - L_y, the K-term denominator and logf
    bar_fl = max |fl(ce +- E_ce) - fl(ce)| + 32 eps32 fl         (fl and m are functions of ce alone; the lower point is
    bar_m  likewise                                               clamped at 0)
    loss:      2 (sum bar_fl + 64 eps32 sum fl) / divisor
    gradient:  2 |w| (bar_m |softmax_k - [k=y]| + m (K + 6) eps32 (softmax_k + [k=y])),   w = gout / divisor
An element whose bar is 0 (ignored pixels, K = 1) must be exactly 0.
The gradient bar has a floor where float32 underflows: below 2^-126 the format's step is 2^-149 whatever the value is, so a
relative bar alone asks for more than any float32 can hold there (the correctly rounded definition itself would miss it, and
so does the float32 torch evaluation, which returns 0 for a gradient of 4e-46).  Two half-steps are counted: the one of
exp(L_k - max), carried by |w| m / den <= |w| alpha (1 + gamma) (pt ce / u <= 1), and the one of the result.  The floor is
added only where the bar is not 0, and is below the relative bar of every element above 1e-37.
"""
import functools

import numpy as np

import helpers as H

F64 = np.float64
EPS32 = 2.0 ** -24
STEP32 = 2.0 ** -149                             # float32's step below 2^-126


def make_inputs(name, B, K, Hh, Ww, sigma, ignore_index, ignore_frac=0.15, seed=11):
    """logits = negative squared distances of f = 3 e_t + sigma noise to the prototypes 3 e_k; t is the label on about 80 % of
    the pixels and a random class otherwise; about `ignore_frac` of the labels are then ignore_index.  The random draws do not
    depend on ignore_index: two cases that differ in it alone have the same logits and the same valid pixels."""
    g = H.rng_for(seed, "focal." + name)
    y = g.integers(0, K, size=(B, Hh, Ww))
    t = np.where(g.random((B, Hh, Ww)) < 0.8, y, g.integers(0, K, size=(B, Hh, Ww)))
    f = sigma * g.standard_normal((B, K, Hh, Ww))
    f += 3.0 * (np.arange(K)[None, :, None, None] == t[:, None])
    protos = 3.0 * np.eye(K)                                                   # [k, channel]
    d2 = ((f[:, None] - protos[None, :, :, None, None]) ** 2).sum(axis=2)      # [B, k, H, W]
    lab = y.astype(np.int64)
    lab[g.random((B, Hh, Ww)) < ignore_frac] = ignore_index
    return np.ascontiguousarray((-d2).astype(np.float32)), lab


def fl_of(ce, alpha, gamma):
    """fl as a function of ce (float64), limits included"""
    ce = np.asarray(ce, dtype=F64)
    u = -np.expm1(-ce)
    if gamma == 0:
        return alpha * ce * np.ones_like(u)
    return np.where(u > 0, alpha * np.power(u, gamma) * ce, 0.0)


def m_of(ce, alpha, gamma):
    """m = d fl / d ce as a function of ce (float64), limits included"""
    ce = np.asarray(ce, dtype=F64)
    if gamma == 0:
        return alpha * np.ones_like(ce)
    u = -np.expm1(-ce)
    safe = np.where(u > 0, u, 1.0)
    pt = np.exp(-ce)
    val = alpha * (np.power(safe, gamma) + gamma * pt * ce * np.power(safe, gamma - 1.0))
    return np.where(u > 0, val, 0.0)


def pixel_terms(logits, labels, ignore_index):
    """-> valid [B,H,W], ce [B,H,W] (0 where ignored), softmax [B,K,H,W], onehot [B,K,H,W], all float64.  The log-sum-exp
    keeps its largest term out of the sum, so a ce far below 2^-53 survives."""
    L = logits.astype(F64)
    B, K, Hh, Ww = L.shape
    valid = labels != ignore_index
    ysafe = np.where(valid, labels, 0)
    am = L.argmax(axis=1)
    mx = np.take_along_axis(L, am[:, None], axis=1)[:, 0]
    e = np.exp(L - mx[:, None])
    np.put_along_axis(e, am[:, None], 0.0, axis=1)
    rest = e.sum(axis=1)
    np.put_along_axis(e, am[:, None], 1.0, axis=1)
    softmax = e / (1.0 + rest)[:, None]
    ly = np.take_along_axis(L, ysafe[:, None], axis=1)[:, 0]
    ce = np.where(valid, (mx - ly) + np.log1p(rest), 0.0)
    onehot = (np.arange(K)[None, :, None, None] == ysafe[:, None]).astype(F64)
    return valid, ce, softmax, onehot


def focal_ref(logits, labels, alpha, gamma, size_average, ignore_index, gout=1.0, divide_by_valid=False):
    """The definition and its bars.  -> dict(loss, loss_bar, grad [B,K,H,W], grad_bar, sums (4,), u [valid pixels], fl, m).
    divide_by_valid is a mutant for tests/test_focal_refs.py only."""
    B, K, Hh, Ww = logits.shape
    valid, ce, softmax, onehot = pixel_terms(logits, labels, ignore_index)
    vf = valid.astype(F64)
    fl = fl_of(ce, alpha, gamma) * vf
    m = m_of(ce, alpha, gamma) * vf
    e_ce = EPS32 * (2.0 * ce + K + 4)
    lo = np.maximum(ce - e_ce, 0.0)
    bar_fl = (np.maximum(np.abs(fl_of(ce + e_ce, alpha, gamma) - fl_of(ce, alpha, gamma)),
                         np.abs(fl_of(lo, alpha, gamma) - fl_of(ce, alpha, gamma))) + 32 * EPS32 * np.abs(fl)) * vf
    bar_m = (np.maximum(np.abs(m_of(ce + e_ce, alpha, gamma) - m_of(ce, alpha, gamma)),
                        np.abs(m_of(lo, alpha, gamma) - m_of(ce, alpha, gamma))) + 32 * EPS32 * np.abs(m)) * vf
    pixels = float(B * Hh * Ww)
    divisor = (vf.sum() if divide_by_valid else pixels) if size_average else 1.0
    w = gout / divisor
    loss = fl.sum() / divisor
    loss_bar = 2.0 * (bar_fl.sum() + 64 * EPS32 * np.abs(fl).sum()) / divisor
    diff = (softmax - onehot) * vf[:, None]
    grad = w * m[:, None] * diff
    grad_bar = 2.0 * abs(w) * (bar_m[:, None] * np.abs(diff) + np.abs(m)[:, None] * (K + 6) * EPS32 * (softmax + onehot) * vf[:, None])
    grad_bar = np.where(grad_bar > 0, grad_bar + 0.5 * STEP32 * (1.0 + abs(w) * abs(alpha) * (1.0 + gamma)), 0.0)
    correct = ((logits.astype(F64).argmax(axis=1) == labels) & valid).sum()
    return dict(loss=loss, loss_bar=loss_bar, grad=grad, grad_bar=grad_bar, fl=fl, m=m, ce=ce, valid=valid,
                u=-np.expm1(-ce[valid]), sums=np.array([fl.sum(), vf.sum(), pixels, float(correct)], dtype=F64),
                sum_bar=2.0 * (bar_fl.sum() + 64 * EPS32 * np.abs(fl).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = (1, 2, 13, 16, 17, 19, 33)            # both sides of the backward's register / re-read split at 16
GAMMAS = (0.0, 0.5, 1.0, 2.0, 5.0)
ALPHAS = (1.0, 0.25)
SHAPES = {"odd": (2, 9, 11),                    # H W % 4 != 0: one float per lane
          "vec": (2, 8, 12),                    # 16-byte loads and stores
          "px": (1, 1, 1)}
IGNORES = (255, -1)
GOUTS = (None, 1.0, -2.5)
# sigma per class count: at 0.3, or for K = 2 at 1.0, almost every pixel is saturated one way or the other and a mutant that
# ignores gamma hides inside the loss bar.  Fewer rivals saturate more pixels: at K = 13 and sigma = 1.0 half of the pixels
# have u < 1e-3, where a wrong divisor (a relative change of the gradient of #ignored / #valid = 0.18) is worth fewer than 50
# of the gradient's bars (relative bar about 2 gamma E_ce / ce), so 13 classes get a little more noise.
SIGMA = {1: 1.0, 2: 2.5, 13: 1.2, 16: 1.0, 17: 1.0, 19: 1.0, 33: 1.0}
# the class counts whose inputs tests/test_focal_refs.py holds to the spread and mutant conditions.  K = 1 has u = 0 on every
# pixel.  K = 2 has one rival class: L_y - L_rival = +-18 + 6 sigma (n_y - n_rival) has a standard deviation of 8.5 sigma and
# 1e-3 < u < 0.999 is the window |L_y - L_rival| < 6.9, which holds at most 19 % of the pixels whatever sigma is (17 % at 2.5);
# K = 2 is therefore held to the float64 and float32 reference checks only.
SPREAD_CLASSES = (13, 16, 17, 19, 33)
SPREAD_SHAPE = (2, 24, 33)                      # 1584 pixels: the fractions below are of enough pixels to mean something


@functools.lru_cache(maxsize=None)
def inputs(K, shape, ignore_index):
    B, Hh, Ww = SHAPES[shape] if isinstance(shape, str) else shape
    frac = 0.0 if B * Hh * Ww == 1 else 0.15
    lg, lab = make_inputs("k%d.%dx%dx%d" % (K, B, Hh, Ww), B, K, Hh, Ww, SIGMA[K], ignore_index, ignore_frac=frac)
    lg.setflags(write=False)
    lab.setflags(write=False)
    return lg, lab


def settings(K, shape):
    """every gamma x alpha x reduction of a (K, shape) cell; ignore_index and gout cycle through their six pairs so that
    each pair meets every gamma, alpha and reduction somewhere in the table"""
    out, i = [], CLASSES.index(K) + 3 * sorted(SHAPES).index(shape)
    for gamma in GAMMAS:
        for alpha in ALPHAS:
            for size_average in (True, False):
                out.append(dict(gamma=gamma, alpha=alpha, size_average=size_average, ignore_index=IGNORES[i % 2],
                                gout=GOUTS[(i // 2) % 3]))
                i += 1
    return out


def edge_frame(K=16):
    """hand-built pixels [1, K, 2, 4]: ce = 0 exactly, about 1e-7, 50 and 90, each once with the own class first and once
    last.  Logit 0 for the own class and one rival at r, the others at -1e4 (their exp is 0 in float32 and in float64):
    ce = log1p(exp(r)) for r < 0 and r + log1p(exp(-r)) for r > 0."""
    lg = np.full((1, K, 2, 4), -1e4, dtype=np.float32)
    lab = np.zeros((1, 2, 4), dtype=np.int64)
    rivals = (-1e4, float(np.log(1e-7)), 50.0, 90.0)
    for row, own in enumerate((0, K - 1)):
        for col, r in enumerate(rivals):
            lab[0, row, col] = own
            lg[0, own, row, col] = 0.0
            lg[0, (own + 3) % K, row, col] = r
    return lg, lab
