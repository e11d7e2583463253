"""Shared by tests/test_incremental_refs.py (CPU) and tests/test_gpu_incremental_predict.py (GPU): the fp64 reference of the
merged prediction of the incremental multi-head model (test_self_distillation.py:292-297 of the reference), the per-pixel
margin that says where a float32 implementation must agree with it, and the seeded cases both files run.

The rule.  Per head i: upsample its low-resolution embedding e_i [B,h,w,C_i] to (H,W) (bilinear, align_corners=False),
logits d_k = -sum_c (f_c - P[k][c])^2 with P = 3 I_K cut to the C_i carried channels, a_i = first maximal k.  Then
pred = a_0 and, for i = 1 .. n-1 in order, pred = novel_id_i where a_i == novel_id_i.

The margin.  A float32 evaluation of d_k (any summation order, with or without fused multiply-adds, on an fp32 bilinear
sample) is off by a small multiple of eps32 * A_k, A_k = sum_c (F_c + P[k][c])^2 with F = the same upsample of |e|: A_k
bounds the sum of the absolute values of every term of d_k written out in the samples of e.  A pixel is DECIDED when in every
head the gap between the two largest logits exceeds 64 * eps32 * max_k A_k (the convention of tests/tools/mint_golden_large.py:
FACT = 64, eps32 = 2^-23); only decided pixels are compared, and a case may exclude at most 1 % of its pixels.
"""
import numpy as np
import torch

from oracle import dmlnet_ref as O

FACT = 64.0
EPS32 = 2.0 ** -23
MAX_UNDECIDED = 0.01

# (h, w, H, W, B): the smallest shapes at which the kernel can go wrong
SHAPES = [
    (1, 1, 4, 4, 1),        # every tap clamped
    (1, 1, 1, 1, 1),
    (3, 5, 12, 20, 2),
    (5, 7, 18, 27, 2),      # non-integer ratio, odd W, single-pixel tail
    (2, 2, 5, 5, 3),        # H W % 4 != 0, batch offsets
    (16, 16, 64, 64, 2),
    (4, 3, 3, 2, 2),        # downscale
]
# (K per head, C per head, novel_id per head)
HEAD_SETS = [
    ((16,), (16,), (0,)),
    ((16, 17), (16, 24), (0, 16)),
    ((16, 17, 18), (16, 24, 24), (0, 16, 17)),
    ((16, 17, 18, 19), (16, 24, 24, 24), (0, 16, 17, 18)),
    ((5, 6), (8, 8), (0, 5)),
]


def centers(K, C, dtype=torch.float64):
    """3 I_K cut to the C carried channels (row C of a K = C + 1 head is zero)"""
    return 3.0 * torch.eye(K, C, dtype=dtype)


def make_heads(seed, shape, head_set, ld_extra=0):
    """Seeded embeddings: list of dicts e [B,h,w,ld] float32 (channels K..C-1 zero as the engine's padded final conv leaves
    them, columns C..ld-1 NaN: never to be read), C, K, ld, novel_id."""
    h, w, H, W, B = shape
    Ks, Cs, ids = head_set
    rng = np.random.default_rng([seed, h, w, H, W, B, len(Ks), Ks[0]])
    heads = []
    for K, C, nid in zip(Ks, Cs, ids):
        ld = C + ld_extra
        e = np.full((B, h, w, ld), np.nan, dtype=np.float32)
        e[..., :C] = 0.0
        n_live = min(K, C)
        e[..., :n_live] = rng.normal(0.0, 1.5, size=(B, h, w, n_live)).astype(np.float32)
        heads.append(dict(e=torch.from_numpy(e), C=C, K=K, ld=ld, novel_id=nid))
    return heads


def head_logits64(e, C, K, H, W):
    """(logits [B,K,H,W], A [B,H,W]) in float64 from e [B,h,w,>=C]"""
    x = e[..., :C].double().permute(0, 3, 1, 2).contiguous()
    up = O.bilinear(x, (H, W))
    logits, _, _ = O.distance_head(up, centers(K, C))
    upa = O.bilinear(x.abs(), (H, W))
    live = upa[:, :min(K, C)]
    A = (upa ** 2).sum(1) + 6.0 * live.max(1).values + 9.0          # max_k sum_c (F_c + P[k][c])^2
    return logits, A


def first_max(logits):
    """first maximal index along dim 1 (numpy's argmax returns the first occurrence)"""
    return torch.from_numpy(np.argmax(logits.numpy(), axis=1)).long()


def merge(argmaxes, novel_ids):
    pred = argmaxes[0].clone()
    for a, nid in zip(argmaxes[1:], novel_ids[1:]):
        pred[a == nid] = nid
    return pred


def merge_literal(outputs, novel_cls):
    """test_self_distillation.py:292-297 of the reference, as written there (head widths 16, 17, ...)"""
    preds_base = outputs[0].detach().max(dim=1)[1]
    for i in range(novel_cls):
        labels_base = outputs[i + 1].detach().max(dim=1)[1]
        preds_base[labels_base == (16 + i)] = 16 + i
    return preds_base


def decided_from_logits(logits, A):
    if logits.shape[1] < 2:
        return torch.ones_like(A, dtype=torch.bool)
    top = logits.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > FACT * EPS32 * A


def reference(heads, H, W):
    """fp64 reference: dict pred [B,H,W] int64, argmax (list per head), decided [B,H,W] bool, logits (list, fp64)"""
    ams, dec, lgs = [], None, []
    for hd in heads:
        lg, A = head_logits64(hd["e"], hd["C"], hd["K"], H, W)
        ams.append(first_max(lg))
        d = decided_from_logits(lg, A)
        dec = d if dec is None else dec & d
        lgs.append(lg)
    return dict(pred=merge(ams, [hd["novel_id"] for hd in heads]), argmax=ams, decided=dec, logits=lgs)


def case(seed, shape, head_set, ld_extra=0):
    """(heads, reference) of one seeded case; asserts the 1 % cap on the reference alone"""
    heads = make_heads(seed, shape, head_set, ld_extra)
    ref = reference(heads, shape[2], shape[3])
    undecided = 1.0 - ref["decided"].double().mean().item()
    assert undecided <= MAX_UNDECIDED, "case %r %r seed %d: %.2f %% of the pixels undecided" % (shape, head_set, seed,
                                                                                             100 * undecided)
    return heads, ref


SEED = 17
CASES = [(SEED, s, hs) for s in SHAPES for hs in HEAD_SETS]


def case_id(c):
    seed, (h, w, H, W, B), (Ks, Cs, ids) = c
    return "%dx%d-%dx%d-b%d-k%s" % (h, w, H, W, B, "_".join(str(k) for k in Ks))
