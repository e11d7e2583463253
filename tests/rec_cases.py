"""The float64 definition of the reconstruction-consistency score (`eval_ood_rec.py --ood rec`: dml_rec_cosine and
dml_rec_confidence) in numpy, the seeded inputs and the case lists that tests/test_rec_refs.py (CPU) and
tests/test_gpu_rec_score.py (GPU) share.

For one frame of label size (H, W), F_k,s [B, h_s, w_s, C] the pyramid concat of the s-th of n resized copies of the frame
(k = 1) and of its reconstruction (k = 2), R the bilinear resize of F.interpolate(mode='bilinear', align_corners=False):
    A_k  = (1/n) sum_s R(F_k,s -> (Hq, Wq)),  (Hq, Wq) = (int(H / 4), int(W / 4))
    u_k  = A_k / max(|A_k|, 1e-12)                                                   (F.normalize over the channels)
    cos  = sum_c (u_1 / max(|u_1|, 1e-8)) (u_2 / max(|u_2|, 1e-8))                   (F.cosine_similarity, eps = 1e-8)
    rec  = R(cos -> (H, W))
    msp  = max_c tmp (prob "logit") or max_c softmax(tmp) (prob "softmax"), tmp = scores[:, first_class:]
    conf = msp if msp > threshold else rec
The resize is a pair of dense matrices here and every sum an einsum: nothing is shared with the device code's walk.
"""
import functools

import numpy as np
import torch

F64 = np.float64

# |cos - cos64| and |conf - conf64| on every pixel.  The rule: 10 x the largest deviation, over CASES and CONF_CASES, of the
# reference's own statements run by torch in float32 from this float64 definition; the factor covers another summation
# order on the device.  tests/test_rec_refs.py recomputes the deviation and holds this constant to the rule.
GPU_BAR = 2.0e-5
GATE_MAX_FRACTION = 0.01      # pixels whose float64 msp lies within GPU_BAR of the threshold may take either branch
MAX_SCALES, MAX_CLASSES = 8, 32


# ------------------------------------------------------------------------------------------------ the definition
def resize_matrix(n_out, n_in):
    """M [n_out, n_in]: row d holds the two weights of area_pixel_compute_source_index(align_corners=False)"""
    scale = F64(n_in) / F64(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=F64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    M = np.zeros((n_out, n_in), dtype=F64)
    np.add.at(M, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(M, (np.arange(n_out), i1), l1)
    return M


def resize_nhwc(F, out_hw):
    """[B, h, w, C] -> [B, Hq, Wq, C]"""
    My, Mx = resize_matrix(out_hw[0], F.shape[1]), resize_matrix(out_hw[1], F.shape[2])
    return np.einsum("yi,xj,bijc->byxc", My, Mx, F.astype(F64), optimize=True)


def mean_resized(feats, out_hw):
    return sum(resize_nhwc(f, out_hw) for f in feats) / F64(len(feats))


def cosine_ref(feats1, feats2, out_hw):
    """-> (cos [B, Hq, Wq] float64, zero [B, Hq, Wq] bool: the pixels where a mean vector is exactly zero)"""
    A1, A2 = mean_resized(feats1, out_hw), mean_resized(feats2, out_hw)
    n1, n2 = np.sqrt((A1 * A1).sum(-1)), np.sqrt((A2 * A2).sum(-1))
    u1, u2 = A1 / np.maximum(n1, 1e-12)[..., None], A2 / np.maximum(n2, 1e-12)[..., None]
    m1, m2 = np.sqrt((u1 * u1).sum(-1)), np.sqrt((u2 * u2).sum(-1))
    cos = ((u1 / np.maximum(m1, 1e-8)[..., None]) * (u2 / np.maximum(m2, 1e-8)[..., None])).sum(-1)
    return cos, (n1 == 0) | (n2 == 0)


def confidence_ref(scores, cos, threshold, prob, first_class):
    """scores [B, K, H, W], cos [B, Hq, Wq] -> dict(conf, msp, rec, gate) in float64; gate: msp > threshold"""
    B, K, H, W = scores.shape
    My, Mx = resize_matrix(H, cos.shape[1]), resize_matrix(W, cos.shape[2])
    rec = np.einsum("yi,xj,bij->byx", My, Mx, cos.astype(F64), optimize=True)
    tmp = scores[:, first_class:].astype(F64)
    if prob == "softmax":
        e = np.exp(tmp - tmp.max(axis=1, keepdims=True))
        tmp = e / e.sum(axis=1, keepdims=True)
    msp = tmp.max(axis=1)
    gate = msp > threshold
    return {"conf": np.where(gate, msp, rec), "msp": msp, "rec": rec, "gate": gate}


# ------------------------------------------------------------------- the reference's statements, run by torch (CPU)
def torch_cosine(feats1, feats2, out_hw, dtype):
    """eval_ood_rec.py:96-125,143-146 of the reference on the two lists of concats, in `dtype`"""
    Fn = torch.nn.functional
    n = len(feats1)

    def accumulate(feats):
        B, _, _, C = feats[0].shape
        ft = torch.zeros(B, C, out_hw[0], out_hw[1], dtype=dtype)
        for f in feats:
            ft_temp = torch.tensor(f).to(dtype).permute(0, 3, 1, 2)
            ft_temp = Fn.interpolate(ft_temp, size=ft.shape[2:], mode="bilinear", align_corners=False)
            ft = ft + ft_temp / n
        return ft

    ft1, ft2 = Fn.normalize(accumulate(feats1), dim=1), Fn.normalize(accumulate(feats2), dim=1)
    return Fn.cosine_similarity(ft1, ft2, dim=1).numpy()


def torch_confidence(scores, cos, threshold, prob, first_class, dtype):
    """eval_ood_rec.py:127-129,141,147-150 of the reference (with the softmax in front of the maximum for prob "softmax")"""
    Fn = torch.nn.functional
    scores, cos = torch.tensor(scores).to(dtype), torch.tensor(cos).to(dtype)
    tmp_scores = scores[:, first_class:]
    if prob == "softmax":
        tmp_scores = Fn.softmax(tmp_scores, dim=1)
    msp, _ = torch.max(tmp_scores, dim=1)
    ft_dist = Fn.interpolate(cos.unsqueeze(1), size=scores.shape[2:], mode="bilinear", align_corners=False)[:, 0]
    t = threshold
    conf = msp * (msp > t).to(dtype) + ft_dist * (msp <= t).to(dtype)
    return conf.numpy(), msp.numpy()


# ------------------------------------------------------------------------------------------------------ the cases
def bf16_round(a):
    """float32 array rounded to bfloat16 and back (what a bf16 plan's concat holds)"""
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


FIVE = ((5, 7), (6, 9), (7, 11), (9, 13), (10, 16))          # -> (9, 12): the last is larger than the output both ways
EIGHT = ((1, 1), (2, 3), (3, 2), (4, 5), (5, 7), (7, 6), (9, 11), (12, 14))

# name -> scales (h, w) per scale, out (Hq, Wq), C, B, dtype, ld (None: C; else one pitch per scale), mode:
#   "noisy": F2 = F1 + 0.7 noise (signed inputs, cos around 0.8); "same": F2 = F1; "zero": noisy with a block of source pixels,
#   the top-left (h + 1) // 2 + 1 rows and (w + 1) // 2 + 1 columns of every scale of F2, set to zero
CASES = {
    "identity_c8": dict(scales=((9, 12),), out=(9, 12), C=8, B=1, dtype="f32", ld=None, mode="noisy", seed=1),
    "five_c4096_f32": dict(scales=FIVE, out=(9, 12), C=4096, B=1, dtype="f32", ld=(4096, 4096, 4104, 4096, 4096), mode="noisy", seed=2),
    "five_c4096_bf16": dict(scales=FIVE, out=(9, 12), C=4096, B=1, dtype="bf16", ld=(4096, 4096, 4104, 4096, 4096), mode="noisy", seed=3),
    "c13_scalar": dict(scales=((4, 5), (6, 7)), out=(5, 6), C=13, B=1, dtype="f32", ld=None, mode="noisy", seed=4),
    "c13_tail": dict(scales=((4, 5), (6, 7)), out=(5, 6), C=13, B=1, dtype="f32", ld=(16, 16), mode="noisy", seed=5),
    "c13_bf16_tail": dict(scales=((4, 5), (6, 7)), out=(5, 6), C=13, B=2, dtype="bf16", ld=(16, 20), mode="noisy", seed=6),
    "c4100_f32": dict(scales=((3, 4), (5, 5)), out=(4, 6), C=4100, B=1, dtype="f32", ld=None, mode="noisy", seed=7),
    "c4100_bf16": dict(scales=((3, 4), (5, 5)), out=(4, 6), C=4100, B=1, dtype="bf16", ld=None, mode="noisy", seed=8),
    "c4099_scalar": dict(scales=((3, 4), (5, 5)), out=(4, 6), C=4099, B=1, dtype="f32", ld=None, mode="noisy", seed=9),
    "eight_scales_b2": dict(scales=EIGHT, out=(6, 19), C=64, B=2, dtype="f32", ld=None, mode="noisy", seed=10),
    "one_by_one_out": dict(scales=((3, 4), (1, 1)), out=(1, 1), C=32, B=2, dtype="f32", ld=None, mode="noisy", seed=11),
    "wide_two_strips": dict(scales=((2, 40), (3, 9)), out=(2, 35), C=20, B=1, dtype="bf16", ld=None, mode="noisy", seed=12),
    "zero_block": dict(scales=FIVE, out=(9, 12), C=64, B=1, dtype="f32", ld=None, mode="zero", seed=13),
    "zero_block_bf16": dict(scales=FIVE, out=(9, 12), C=36, B=1, dtype="bf16", ld=None, mode="zero", seed=14),
    "same_c4096": dict(scales=FIVE, out=(9, 12), C=4096, B=1, dtype="f32", ld=None, mode="same", seed=15),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (feats1, feats2): lists of float32 arrays [B, h, w, C] (bf16 cases: already rounded to bf16 values)"""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c["seed"])
    f1, f2 = [], []
    for (h, w) in c["scales"]:
        a = rng.standard_normal((c["B"], h, w, c["C"])).astype(np.float32)
        b = a if c["mode"] == "same" else (a + 0.7 * rng.standard_normal(a.shape)).astype(np.float32)
        if c["mode"] == "zero":
            b = b.copy()
            b[:, :(h + 1) // 2 + 1, :(w + 1) // 2 + 1] = 0.0
        if c["dtype"] == "bf16":
            a, b = bf16_round(a), bf16_round(b)
        a.setflags(write=False)
        b.setflags(write=False)
        f1.append(a)
        f2.append(b)
    return f1, f2


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (cos64, zero) of the case, computed once"""
    f1, f2 = inputs(name)
    cos, zero = cosine_ref(f1, f2, CASES[name]["out"])
    cos.setflags(write=False)
    zero.setflags(write=False)
    return cos, zero


# name -> K, first_class, prob, threshold, amp (the scores are amp x standard normal), B; (H, W) = (37, 50) over cos (9, 12)
CONF_HW, CONF_COS_HW = (37, 50), (9, 12)
CONF_CASES = {
    "k13_logit": dict(K=13, first_class=0, prob="logit", threshold=1.6, amp=1.0, B=1, seed=1),
    "k13_logit_back": dict(K=13, first_class=1, prob="logit", threshold=1.6, amp=1.0, B=2, seed=2),
    "k13_logit_closed": dict(K=13, first_class=0, prob="logit", threshold=0.999, amp=-1.0, B=1, seed=3),   # scores <= 0: gate shut
    "k13_softmax": dict(K=13, first_class=0, prob="softmax", threshold=0.5, amp=2.0, B=1, seed=4),
    "k13_softmax_back": dict(K=13, first_class=1, prob="softmax", threshold=0.5, amp=2.0, B=2, seed=5),
    "k13_softmax_999": dict(K=13, first_class=0, prob="softmax", threshold=0.999, amp=9.0, B=1, seed=6),
    "k1_logit": dict(K=1, first_class=0, prob="logit", threshold=0.0, amp=1.0, B=1, seed=7),
    "k2_back_softmax": dict(K=2, first_class=1, prob="softmax", threshold=0.999, amp=1.0, B=1, seed=8),     # softmax of one class: 1
    "k32_softmax": dict(K=32, first_class=0, prob="softmax", threshold=0.4, amp=2.5, B=1, seed=9),
    "k33_back_logit": dict(K=33, first_class=1, prob="logit", threshold=2.0, amp=1.0, B=1, seed=10),
}


@functools.lru_cache(maxsize=None)
def conf_inputs(name):
    """-> (scores [B, K, 37, 50], cos [B, 9, 12]) float32"""
    c = CONF_CASES[name]
    rng = np.random.default_rng(2000 + c["seed"])
    s = rng.standard_normal((c["B"], c["K"]) + CONF_HW)
    s = -np.abs(s) if c["amp"] < 0 else c["amp"] * s
    scores = s.astype(np.float32)
    cos = rng.uniform(-1.0, 1.0, (c["B"],) + CONF_COS_HW).astype(np.float32)
    scores.setflags(write=False)
    cos.setflags(write=False)
    return scores, cos


@functools.lru_cache(maxsize=None)
def conf_reference(name):
    """-> dict(conf, msp, rec, gate, near): near marks the pixels left out, |msp - threshold| <= GPU_BAR"""
    c = CONF_CASES[name]
    scores, cos = conf_inputs(name)
    r = confidence_ref(scores, cos, c["threshold"], c["prob"], c["first_class"])
    r["near"] = np.abs(r["msp"] - c["threshold"]) <= GPU_BAR
    for v in r.values():
        v.setflags(write=False)
    return r
