"""Case table shared by tests/test_novel_refs.py (CPU) and tests/test_gpu_novel_classes.py (GPU): the float64 definition
of the one-pass open-world post-processing with N few-shot prototypes (dml_open_world_post), its seeded inputs and the
decision margins.  A plain module in the style of tests/open_set_cases.py (no fixtures, no hooks); nothing here looks at
a kernel's output.

The rule: preds = first maximal logit; d_j = -sum_c (f_c - p_jc)^2; j* = the index whose d is strictly above every other
d_j (a tie for the top: none); preds = new_labels[j*] iff d_j* > thresh and (not vs_known or d_j* > max_k logit_k).
"""
import numpy as np

import open_set_cases as CS

MAXN = 8                                      # csrc/scores.hip: prototypes per launch
RANDOM_NS = (1, 2, 3, 8)
RANDOM_SHAPE = (2, 96, 160)
ODD_SHAPES = ((3, 5, 7), (1, 1, 1))           # H W not a multiple of 4: the one-pixel-per-lane path
ODD_CS = (1, 13, 32)
ODD_KS = (1, 13, 19, 32)
ODD_NS = (0, 1, 3)
EXACT_THRESHOLDS = (np.float32(-1.5), CS.up(-1.5), CS.down(-1.5), np.float32(0.0), np.float32(-5.0))


def post_ref(lg, feats, protos, new_labels, thresh, vs_known):
    """float64 of the definition on float32 inputs lg [B,K,H,W], feats [B,H,W,C], protos [N,C].  Returns a dict:
    preds (int64 [B,H,W]), hit (relabelled), jstar (index of the top distance; -1 for N = 0), tie, and `sure`: the pixels
    whose decision an fp32 evaluation cannot change -- every margin above its bound:
      |d* - thresh| and (vs_known) |d* - max logit| above relabel_err(d*, C) = (C + 2) eps32 |d*|,
      d* - second-best d above (C + 2) eps32 (|d*| + |d_2nd|)   (two such evaluations are compared)."""
    B, K, Hh, Ww = lg.shape
    preds = np.argmax(lg, axis=1).astype(np.int64)                       # first maximal index; exact in any precision
    N = 0 if protos is None else len(protos)
    if N == 0:
        z = np.zeros((B, Hh, Ww), bool)
        return dict(preds=preds, hit=z, jstar=np.full((B, Hh, Ww), -1), tie=z, sure=~z)
    C = feats.shape[-1]
    f = feats.astype(np.float64)
    d = np.stack([-((f - protos[j].astype(np.float64)) ** 2).sum(axis=-1) for j in range(N)], axis=-1)   # [B,H,W,N]
    jstar = np.argmax(d, axis=-1)
    dstar = d.max(axis=-1)
    best = lg.astype(np.float64).max(axis=1)
    if N > 1:
        d2 = np.sort(d, axis=-1)[..., -2]
        tie = d2 == dstar
        sure = (dstar - d2) > (C + 2) * CS.EPS32 * (np.abs(dstar) + np.abs(d2))
    else:
        tie = np.zeros(dstar.shape, bool)
        sure = np.ones(dstar.shape, bool)
    hit = ~tie & (dstar > np.float64(thresh))
    sure &= np.abs(dstar - np.float64(thresh)) > CS.relabel_err(dstar, C)
    if vs_known:
        hit &= dstar > best
        sure &= np.abs(dstar - best) > CS.relabel_err(dstar, C)
    out = preds.copy()
    out[hit] = np.asarray(new_labels, np.int64)[jstar[hit]]
    return dict(preds=out, hit=hit, jstar=jstar, tie=tie, sure=sure)


def random_batch(N, C=16, K=16, shape=RANDOM_SHAPE):
    """features scattered around a prototype picked per pixel (one noise scale per pixel, 0.05 .. 0.6), logits
    -|N(0,1)| 2 - 0.3.  Returns feats [B,H,W,C], logits [B,K,H,W], protos [N,C] (None for N = 0), new_labels."""
    rs = np.random.RandomState(505 + N)
    B, Hh, Ww = shape
    protos = rs.standard_normal((N, C))
    if N:
        j = rs.randint(0, N, (B, Hh, Ww))
        centre = protos[j]
    else:
        centre = np.zeros((B, Hh, Ww, C))
    feats = (centre + rs.standard_normal((B, Hh, Ww, C)) * rs.uniform(0.05, 0.6, (B, Hh, Ww, 1))).astype(np.float32)
    lg = (-np.abs(rs.standard_normal((B, K, Hh, Ww))) * 2.0 - 0.3).astype(np.float32)
    return feats, lg, (protos.astype(np.float32) if N else None), [K + j for j in range(N)]


def exact_row(C, K, new_labels=(16, 17, 18)):
    """One row of pixels against three prototypes p0 = 0, p1 = e_0, p2 = 4 e_1: every difference is a multiple of 0.5,
    so every d_j is exact in fp32 and no pixel is left out.  Needs C >= 3.  Returns feats [2,1,n,C], logits [2,K,1,n],
    protos [3,C], and `what`: pixel index by name.  Image 1 is image 0 reversed, so a batch-stride slip cannot pass.
      tie        d0 = d1 = -0.25 above the threshold and every logit: an exact two-way tie for the top, never relabelled
      on_thresh  d0 = -1.5: relabelled only for a threshold below -1.5
      on_logit   d0 = -0.25 = the max logit: relabelled only with vs_known = False
      above      the same with the max logit one ulp below: relabelled
      p1, p2     on the prototype itself (d = 0), logits far below
      zero       d1 = 0 and a max logit of 0: d > logit is false
      far        ten units from everything"""
    assert C >= 3
    protos = np.zeros((3, C), np.float32)
    protos[1, 0] = 1.0
    protos[2, 1] = 4.0

    def vec(**kw):
        v = np.zeros(C, np.float32)
        for k, x in kw.items():
            v[{"a": 0, "b": 1, "z": C - 1}[k]] = x
        return v

    px = [("tie", vec(a=0.5), -10.0),
          ("on_thresh", vec(a=-1.0, z=0.5, b=-0.5), -10.0),
          ("on_logit", vec(a=-0.5), np.float32(-0.25)),
          ("above", vec(a=-0.5), CS.down(-0.25)),
          ("p1", protos[1].copy(), -10.0),
          ("p2", protos[2].copy(), -10.0),
          ("zero", protos[1].copy(), 0.0),
          ("far", vec(a=10.0, z=-10.0), -10.0)]
    n = len(px)
    feats = np.stack([f for _, f, _ in px])[None, None]
    lg = np.full((1, K, 1, n), -50.0, np.float32)
    for i, (_, _, m) in enumerate(px):
        lg[0, (K - 1 - i) % K, 0, i] = m                                 # the maximum sits at a different k per pixel
    feats = np.concatenate([feats, feats[:, :, ::-1]]).astype(np.float32)
    lg = np.concatenate([lg, lg[:, :, :, ::-1]])
    return feats, lg, protos, list(new_labels), {name: i for i, (name, _, _) in enumerate(px)}
