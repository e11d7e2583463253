"""Case table shared by tests/test_loss_refs.py (CPU) and tests/test_gpu_loss_edges.py (GPU): the float64 definitions of the DML loss
(dml_loss_fwd / dml_loss_finalize / dml_loss_bwd, csrc/dml_loss.hip) and of the fused backward of loss + distance head + x4 upsample
(dml_head_bwd_fused, csrc/head.hip), the seeded inputs, the case tables, the launch arithmetic of the entry points restated as pure
functions, the error bars and the comparison both test files use.  A plain module (numpy only): nothing here imports the library or
looks at a kernel's output other than as the `got` argument of head_cases.check_close.

Definitions (float64, on the float32 inputs and the float32 scalars the kernels get):
  loss_ref      per pixel lse = max + log sum_k exp(l_k - max), nll = lse - l_y, p_k = exp(l_k - lse).  sums = (sum of nll over the
                valid pixels, their number, VAR = sum over valid of (-l_y) / (H W), number of valid pixels whose FIRST maximal plane
                is the label, n);  loss = (sums[0] / sums[1] + alpha sums[2]) / n;
                d loss / d l_k = gout ((p_k - [k == y]) / (n_valid n) - alpha [k == y] / (H W n)) on a valid pixel, 0 elsewhere.
                This is oracle/dmlnet_ref.dml_loss (tests/test_loss_refs.py compares them through float64 autograd).
  head_bwd_ref  logits = -|f - m_k|^2, p = softmax, g_k = w_ce (p_k - [k == y]) - w_var [k == y] on valid pixels and 0 elsewhere,
                df = -2 sum_k g_k (f - m_k), de = U^T df with U the separable x4 bilinear matrix of align_corners=False (weights 1/8,
                3/8, 5/8, 7/8 and the clamped 1 at the borders: exact);  w_ce = gout / (n_valid n), w_var = gout alpha / (H W n).

eps32 = 2^-24 is float32's unit roundoff.  Bars, each a count of float32 roundings (never measured on a kernel); c and a are the
count times 2 for the order of the sums:
  g_k           p_k w_ce: the denominator's K - 1 = 15 additions, the division w_ce / den, the two roundings of w_ce (the product
                n_valid n, the quotient) and the product with exp: 19; the label term adds w_var (three roundings), the sum
                w_ce + w_var and the subtraction: 22.  C_G = 44, against ghat_k = w_ce p_k + [k == y] (w_ce + w_var) >= |g_k|;
  softmax       the exponent's argument x_k = l_k - max is rounded once (eps32 |x_k|); the 2^(x log2 e) form of __expf rounds the
                product again and carries log2 e to 0.22 eps32: together XC = 2.25 eps32 |x_k| for the fused kernel, 1 for
                dml_loss_bwd's expf; exp itself two ulp = 4 eps32 and the rounding of the result: a = 5, A_EXP = 10.  In the fused
                kernel the logits are recomputed from the features in float32 (include/dmlnet_hip.h: "the logits recomputed from
                feats"), so the argument also carries logit k's own bar, head_cases's (C + 3) eps32 d_k for the general path or
                2 eps32 |d_k (2 f_k - d_k)| <= 2 eps32 (|f|^2 + d_k) for the closed form of a diagonal matrix; either path is
                allowed, the bar takes the larger.  The computed maximum is one number subtracted from every class: its own error
                is a common shift, which the softmax ignores.  With e_k the arguments' errors, |e_k| <= E_k,
                log(p~_k / p_k) = e_k - log sum_j p_j exp(e_j) = (1 - q_k) e_k - sum_{j != k} q_j e_j for a softmax q between p
                and p~ (mean value theorem), q_j <= p_j exp(2 max E): p_k moves by at most
                p_k expm1(exp(2 max E) ((1 - p_k) E_k + sum_{j != k} p_j E_j)).  A dominant class (1 - p_k ~ 0) cannot move by
                its own E_k, and far classes have large E_k and no weight: the term is per class, not the maximum over the
                classes;
  df, de        gs = sum_k g_k: 15 additions on top of the 22 of g_k; gs f_c one more: 38, against G |f_c| with G = sum_k ghat_k
                (gs itself cancels to -w_var: like head_cases's backward bar this one is against the magnitudes that entered, not
                against |gs|);  gm_c = sum_k g_k m_kc: 16 products, 15 additions: 38 against sum_k ghat_k |m_kc|;  the difference:
                39;  the transposed bilinear: the product with the column weight, at most 7 additions into a row cell (in the
                thread and across the LDS exchange), the product with the row weight, at most 7 additions over the rows: 16.
                C_HEAD = 2 (39 + 16) = 110, against M_c = 2 (G |f_c| + sum_k ghat_k |m_kc|) summed with the weights wy wx;
                half a bfloat16 spacing more for a bfloat16 de (bn_cases.stored_bar).  The unfused chain does the same operations
                (with d loss / d logits and d loss / d features rounded to float32 in between, which the counts already hold);
  loss          nll of a pixel: den as above ((K - 1) + 5 + sum_k p_k |x_k|), logf two ulp of log den, the difference max - l_y and
                the sum once each; a lane adds T = (pixels per item) x (trips) of them, a wave folds in 6 steps, the workgroup in
                3, the rest is double: (T + 9) eps32 sum nll.  VAR the same with |l_y|.  Times 2; one more rounding for the float
                the loss is stored as.
Counts (sums[1], sums[3]) and sums[4] are integers: compared exactly.

Exact inputs of the fused kernel ("exact"): features are multiples of 1/4 in [-2, 2] except one channel per pixel, the dominant
class's, at +-64 (+ a multiple of 1/4): that class leads by more than 200 in logit, so every other softmax weight is exactly 0 in
float32 (exp(-200) is below the smallest subnormal) and below 1e-80 in float64 (the reference sets them to 0: the difference is below
1e-80 of a gradient of order 2^-12).  Prototypes 3 I ("eye"), a dyadic diagonal with a negative and a zero entry and -0.0 beside the
diagonal ("diag"), a dyadic general matrix ("gend").  n_valid = 1024, n = 2, gout = 0.5 or NULL; alpha = H W 2^-12 (or 0), so that
w_ce = 2^-12 (2^-11) and w_var = 2^-14 (2^-13) are powers of two -- alpha alone a power of two would leave w_var = gout alpha /
(H W n) with the odd factors of H W (49 at 7 x 14) in its denominator, and nothing downstream would be exact.  Every g is then a
multiple of 2^-14, every product and partial sum a multiple of 2^-21 below 2^3: exact in float32 in any order
(tests/test_loss_refs.py asserts the grid and the magnitudes case by case).
"""
import numpy as np

import head_cases as HC
import pool_cases as PC
from bn_cases import EPS32, F32, F64, store, stored_bar

C = K = 16                                     # what dml_head_bwd_fused supports
C_G, C_HEAD, A_EXP = 44, 110, 10
XC_FUSED, XC_LOSS = 2.25, 1.0
TINY = 2.0 ** -120                             # float32 flushes what float64 still holds
HB_TJ, HB_TI = 7, 14                           # head.hip's tile of the low-resolution map
MAX_BLOCKS = 2048                              # common.h: grid cap of dml_loss_fwd
BWD_BLOCKS = 256 * 32                          # dml_loss_bwd's own cap
MUTANTS = ("no_wvar", "swap_lr", "clamp_x1", "last_max")   # the `mut` arguments below: wrong on purpose, for tests/test_loss_refs.py


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------
def grid_for(items, block, cap):
    return int(min(max((items + block - 1) // block, 1), cap))


def loss_launch(entry, B, H, W):
    """(pixels per item, workgroups, trips of the grid-stride loop) of dml_loss_fwd ("fwd") / dml_loss_bwd ("bwd")"""
    px = 4 if (H * W) % 4 == 0 else 1
    items = B * H * W // px
    grid = grid_for(items, 256, MAX_BLOCKS if entry == "fwd" else BWD_BLOCKS)
    return px, grid, -(-items // (grid * 256))


def fused_tiles(h, w):
    """(tiles down, tiles across) of one image"""
    return -(-h // HB_TJ), -(-w // HB_TI)


def is_diagonal(P):
    """head.hip's test: every off-diagonal scalar == 0 (-0.0 included; a NaN is not)"""
    P = np.asarray(P, F32)
    off = P[~np.eye(P.shape[0], dtype=bool)]
    return bool((off == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# float64 definitions
# ---------------------------------------------------------------------------------------------------------------------
def _softmax(lg):
    """lg[N, K] -> (p, x = lg - max, log den)"""
    with np.errstate(invalid="ignore", over="ignore"):
        mx = lg.max(1, keepdims=True)
        x = lg - mx
        e = np.exp(x)
        den = e.sum(1, keepdims=True)
        return e / den, x, np.log(den[:, 0])


def first_max(lg, last=False):
    """lg[N, K] -> the first (last: the mutant's) maximal plane; a NaN never wins"""
    lg = np.where(np.isnan(lg), -np.inf, lg)
    if last:
        return lg.shape[1] - 1 - np.argmax(lg[:, ::-1], 1)
    return np.argmax(lg, 1)


def loss_ref(logits, labels, ignore, alpha, n_images, gout, n_valid=None, bars=True, mut=None, chunk=1 << 18):
    """logits[B, K, H, W] float32, labels[B, H, W] -> dict: sums[5], sbar[5] (0 for the integers), loss, lbar, grad[B, K, H, W] float64,
    gbar float32.  n_images: the float the kernel gets (> 0).  gout: None is 1.  n_valid: the count the gradient divides by (default:
    the labels' own).  Evaluated in chunks of pixels: the above-the-cap cases stay within a few hundred MB."""
    B, Kk, H, W = logits.shape
    HW = H * W
    lg3, lab2 = logits.reshape(B, Kk, HW), labels.reshape(B, HW)
    alpha, go, n = float(F32(alpha)), 1.0 if gout is None else float(F32(gout)), float(F32(n_images))
    s = np.zeros(5)
    mag = np.zeros(3)                                                          # per-pixel part of bar0, sum nll, sum |own|
    for b in range(B):
        for at in range(0, HW, chunk):
            lg = lg3[b, :, at:at + chunk].T.astype(F64)
            lab = lab2[b, at:at + chunk]
            valid = lab != ignore
            y = np.where(valid, lab, 0)
            p, x, logden = _softmax(lg)
            with np.errstate(invalid="ignore"):
                own = np.take_along_axis(lg, y[:, None], 1)[:, 0]
                nll = (lg.max(1) - own) + logden
                s[0] += nll[valid].sum()
                s[1] += valid.sum()
                s[2] += -own[valid].sum() / HW
                s[3] += (first_max(lg, mut == "last_max")[valid] == lab[valid]).sum()
                if bars:
                    px = np.where(np.isfinite(x), p * np.abs(x), 0.0).sum(1)
                    mag[0] += ((Kk + 4) + px + 4 * logden + (lg.max(1) - own) + nll)[valid].sum()
                    mag[1] += np.abs(nll[valid]).sum()
                    mag[2] += np.abs(own[valid]).sum()
    s[4] = n
    nv = s[1] if n_valid is None else np.float64(n_valid)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = (s[0] / s[1] + alpha * s[2]) / n
        w_ce, w_var = go / (nv * n), (0.0 if mut == "no_wvar" else go * alpha / (HW * n))
    out = {"sums": s, "loss": loss, "sbar": None, "lbar": None, "gbar": None}
    if bars:
        T = loss_launch("fwd", B, H, W)[0] * loss_launch("fwd", B, H, W)[2]
        sbar = np.zeros(5)
        sbar[0] = 2 * EPS32 * (mag[0] + (T + 9) * mag[1])
        sbar[2] = 2 * EPS32 * (T + 9) * mag[2] / HW
        out["sbar"] = sbar
        with np.errstate(invalid="ignore", divide="ignore"):
            out["lbar"] = (sbar[0] / s[1] + alpha * sbar[2]) / n + 2 * EPS32 * (abs(s[0] / s[1]) + abs(alpha * s[2])) / n
    grad = np.zeros((B, Kk, HW))
    gbar = np.zeros((B, Kk, HW), F32) if bars else None
    for b in range(B):
        for at in range(0, HW, chunk):
            lg = lg3[b, :, at:at + chunk].T.astype(F64)
            lab = lab2[b, at:at + chunk]
            valid = (lab != ignore)[:, None]
            oh = (np.arange(Kk)[None, :] == lab[:, None]) & valid
            p, x, _ = _softmax(lg)
            with np.errstate(invalid="ignore"):
                grad[b, :, at:at + chunk] = np.where(valid, w_ce * (p - oh) - w_var * oh, 0.0).T
                if bars:
                    gbar[b, :, at:at + chunk] = _gbar(p, x, oh, valid, w_ce, w_var, 0.0, XC_LOSS)[0].T
    out["grad"] = grad.reshape(B, Kk, H, W)
    if bars:
        out["gbar"] = gbar.reshape(B, Kk, H, W)
    return out


def _gbar(p, x, oh, valid, w_ce, w_var, lbar, xc):
    """(bar of g[N, K], ghat[N, K], dp[N, K]) from the softmax p, the exponents' arguments x, the one-hot labels and the bar lbar[N, K] of
    the logits themselves (0: they are inputs)"""
    with np.errstate(invalid="ignore", over="ignore"):
        E = lbar + EPS32 * (A_EXP + xc * np.where(np.isfinite(x), np.abs(x), 0.0))
        pE = np.where(p > 0, p * E, 0.0)
        second = np.exp(2 * np.minimum(np.max(np.where(np.isnan(E), 0.0, E), 1, keepdims=True), 25.0))
        L = second * ((p.sum(1, keepdims=True) - p) * E + (pE.sum(1, keepdims=True) - pE))
        dp = np.where(p > 0, p * np.expm1(np.minimum(L, 50.0)), 0.0)
        ghat = np.where(valid, w_ce * p + oh * (w_ce + w_var), 0.0)
        bar = np.where(valid, w_ce * dp + C_G * EPS32 * ghat + TINY * w_ce, 0.0)
    return bar, ghat, dp


def lerp4(out, inn, mut=None):
    """PC.lerp_matrix with the mutants of tests/test_loss_refs.py: the two column weights swapped; x1 clamped one column early"""
    i0, i1, l0, l1, _ = PC.src_index(out, inn)
    if mut == "clamp_x1":
        i1 = i0 + (i0 < inn - 2)
    if mut == "swap_lr":
        l0, l1 = l1, l0
    M = np.zeros((out, inn))
    np.add.at(M, (np.arange(out), i0), l0)
    np.add.at(M, (np.arange(out), i1), l1)
    return M


def head_bwd_ref(feats, labels, protos, n_valid, n_images, ignore, alpha, gout, out="f32", bars=True, mut=None, parts=False):
    """feats[B, H, W, 16] float32, labels[B, H, W], protos[16, 16] -> (de[B, h, w, 16] float64, its bar or None).  parts: also the dict
    of the intermediates (logits NCHW, glogits NCHW and its bar, df NHWC)."""
    f, P = np.asarray(feats, F64), np.asarray(protos, F64)
    B, H, W, Cc = f.shape
    h, w = H // 4, W // 4
    alpha, go, n = float(F32(alpha)), 1.0 if gout is None else float(F32(gout)), float(F32(n_images))
    w_ce = go / (float(n_valid) * n) if n_valid else np.inf
    w_var = 0.0 if mut == "no_wvar" else go * alpha / (H * W * n)
    fl, lab = f.reshape(-1, Cc), np.asarray(labels).reshape(-1)
    valid = (lab != ignore)[:, None]
    oh = (np.arange(P.shape[0])[None, :] == lab[:, None]) & valid
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((fl[:, None, :] - P[None]) ** 2).sum(-1)
        p, x, _ = _softmax(-d)
        p = np.where(x < -200.0, 0.0, p)                                         # below 1e-80; float32 has exactly 0 there
        g = np.where(valid, w_ce * (p - oh) - w_var * oh, 0.0)
        df = -2.0 * (g.sum(1, keepdims=True) * fl - g @ P)
        My, Mx = lerp4(H, h), lerp4(W, w, mut if mut in ("swap_lr", "clamp_x1") else None)
        de = PC._sep(My, Mx, df.reshape(B, H, W, Cc), True)
        bar = gb = None
        if bars:
            f2 = (fl * fl).sum(1, keepdims=True)
            lbar = EPS32 * np.maximum((Cc + 3) * d, 2 * (f2 + d))
            gb, ghat, dp = _gbar(p, x, oh, valid, w_ce, w_var, lbar, XC_FUSED)
            M = 2 * (ghat.sum(1, keepdims=True) * np.abs(fl) + ghat @ np.abs(P))
            S = np.where(valid, 2 * w_ce * (dp.sum(1, keepdims=True) * np.abs(fl) + dp @ np.abs(P)), 0.0)
            pix = C_HEAD * EPS32 * M + S + TINY * np.where(valid, w_ce, 0.0)
            bar = stored_bar(PC._sep(lerp4(H, h), lerp4(W, w), pix.reshape(B, H, W, Cc), True), de, out)
    if parts:
        nchw = lambda a: np.ascontiguousarray(a.reshape(B, H, W, -1).transpose(0, 3, 1, 2))
        return de, bar, {"logits": nchw(-d), "glogits": nchw(g), "gbar": None if gb is None else nchw(gb), "df": df.reshape(B, H, W, Cc)}
    return de, bar


# ---------------------------------------------------------------------------------------------------------------------
# the fused kernel's cases
# ---------------------------------------------------------------------------------------------------------------------
# name -> (B, h, w); H = 4 h, W = 4 w
GEOMS = {
    "every_clamp_1x1": (1, 1, 1),              # x1 == x0 and y1 == y0 everywhere
    "one_row_1x14": (2, 1, 14),
    "one_column_7x1": (1, 7, 1),
    "one_tile_7x14": (1, 7, 14),               # both halos outside the image
    "second_tile_one_column_7x15": (1, 7, 15),  # fed almost only by the left halo
    "second_tile_one_row_8x14": (1, 8, 14),
    "ragged_tile_6x13": (2, 6, 13),
    "tiles_3x3_15x29": (1, 15, 29),            # an interior tile with halos on all sides
    "exact_multiples_14x28_b3": (3, 14, 28),   # the block-to-image index
}
EXACT_PKINDS = ("eye", "diag", "gend")
REAL_PKINDS = ("eye", "diag", "general", "almost")
LABEL_KINDS = ("ten_percent", "image0_ignored", "all_ignored")
EXACT_NVALID, EXACT_N = 1024.0, 2.0
# (gout, alpha on?, n_images passed -- 0: read from sums[4]) of the runs of one case
SCALARS = [(0.5, True, True), (None, True, False), (0.5, False, True)]
REAL_ALPHA, REAL_GOUT = 0.01, 1.7


def _seed(*parts):
    return (7700 + sum(p * int(n) for p, n in zip((1, 3, 17, 5, 29, 101, 211, 13), parts))) % (2 ** 31 - 1)


def protos(pkind):
    """float32 P[16, 16]"""
    rs = np.random.RandomState(_seed(*[ord(ch) for ch in pkind[:4]]))
    eye = 3.0 * np.eye(K, C)
    if pkind == "eye":
        return eye.astype(F32)
    if pkind == "diag":
        P = np.full((K, C), -0.0, F32)
        P[np.arange(K), np.arange(C)] = np.array([3, -2, 0, 2.5, 3, -3, 2, 4, 3, 0, -2.5, 3, 2, -4, 3, 3.5], F32)
        return P
    if pkind == "gend":
        P = eye.copy()
        for _ in range(12):
            k, c = rs.randint(0, K), rs.randint(0, C)
            if k != c:
                P[k, c] = rs.choice([-0.25, 0.25])
        return P.astype(F32)
    if pkind == "general":
        return (eye + 0.05 * rs.standard_normal((K, C))).astype(F32)
    assert pkind == "almost"
    P = eye.astype(F32)
    P[5, 9] = F32(2.0 ** -20)
    return P


def labels_for(lkind, B, H, W, ignore, rs, dom=None):
    """int64 labels[B, H, W]: 10 % ignored; the same with image 0 all ignored; all ignored.  dom[B, H, W] (exact inputs): half the
    valid pixels carry the dominant class, the others another one"""
    lab = rs.randint(0, K, (B, H, W)).astype(np.int64)
    if dom is not None:
        lab = np.where(rs.rand(B, H, W) < 0.5, dom, (dom + 1 + rs.randint(0, K - 1, (B, H, W))) % K).astype(np.int64)
    lab[rs.rand(B, H, W) < 0.1] = ignore
    if lkind == "image0_ignored":
        lab[0] = ignore
    if lkind == "all_ignored":
        lab[:] = ignore
    return lab


def fused_input(kind, pkind, gname, lkind="ten_percent", ignore=255):
    """(feats[B, H, W, 16] float32, labels, P).  kind: "exact", "real" (1.5 N), "big" (30 N: exponents' arguments below -1000)"""
    B, h, w = GEOMS[gname]
    H, W = 4 * h, 4 * w
    P = protos(pkind)
    rs = np.random.RandomState(_seed(B, h, w, ("exact", "real", "big").index(kind), REAL_PKINDS.index(pkind) if pkind in REAL_PKINDS else 9))
    if kind == "exact":
        f = rs.randint(-8, 9, (B, H, W, C)).astype(F64) / 4
        strong = np.flatnonzero(np.abs(np.diag(P)) >= 2)
        dom = strong[rs.randint(0, len(strong), (B, H, W))]
        big = np.sign(np.diag(P))[dom] * 64.0 + rs.randint(-8, 9, (B, H, W)) / 4
        np.put_along_axis(f, dom[..., None], big[..., None], -1)
        return f.astype(F32), labels_for(lkind, B, H, W, ignore, rs, dom), P
    f = ((1.5 if kind == "real" else 30.0) * rs.standard_normal((B, H, W, C))).astype(F32)
    return f, labels_for(lkind, B, H, W, ignore, rs), P


def exact_scalars(H, W, gout, alpha_on):
    """(n_valid, n, alpha) of an exact case: w_ce and w_var powers of two"""
    return EXACT_NVALID, EXACT_N, (float(F32(H * W * 2.0 ** -12)) if alpha_on else 0.0)


def fused_scalars(kind, lkind, lab, ignore, H_, W_, gout=0.5, alpha_on=True):
    """(n_valid, n, alpha, gout) a case runs with: powers of two for the exact kind; the labels' own count, n = B for the others; no
    valid pixel: n_valid = 0 (w_ce is inf)"""
    if kind == "exact":
        nv, n, alpha = exact_scalars(H_, W_, gout, alpha_on)
    else:
        nv, n, alpha = float((lab != ignore).sum()), float(lab.shape[0]), (REAL_ALPHA if alpha_on else 0.0)
        gout = None if gout is None else REAL_GOUT
    if lkind == "all_ignored":
        nv = 0.0
    return nv, n, alpha, gout


def fused_cases():
    """(kind, pkind, geometry, label kind, ignore_index): every geometry with every prototype kind; the label kinds and the
    second ignore_index on the three geometries with B >= 2; the 30 N features on the 3 x 3 tiles"""
    out = []
    for gname in GEOMS:
        out += [("exact", pk, gname, "ten_percent", 255) for pk in EXACT_PKINDS]
        out += [("real", pk, gname, "ten_percent", 255) for pk in REAL_PKINDS]
    for gname in ("one_row_1x14", "ragged_tile_6x13", "exact_multiples_14x28_b3"):
        for kind, pk in (("exact", "diag"), ("real", "general")):
            out += [(kind, pk, gname, "image0_ignored", -1), (kind, pk, gname, "all_ignored", 255), (kind, pk, gname, "ten_percent", -1)]
    out += [("big", pk, "tiles_3x3_15x29", "ten_percent", 255) for pk in ("eye", "general")]
    return out


NONFINITE_X = (4 * 16 + 2, 4 * 17 + 1)          # third pixel of a group: columns 16 and 17, not 15; second pixel: 16 and 17, not 18


def fused_nonfinite(pkind, value, X=NONFINITE_X[0], gname="tiles_3x3_15x29"):
    """(feats with `value` in one channel of one pixel, labels with that pixel ignored -- the reference of every other element --, P,
    must[B, h, w]: the low-resolution pixels that pixel interpolates into with a non-zero weight).  The pixel lies in the interior
    tile, in a pixel group whose two neighbour groups belong to the same tile: the kernel folds a pixel into three column partials
    (left, own, right), one of them with weight zero, and all three columns are written by this tile"""
    f, lab, P = fused_input("real", pkind, gname)
    B, H, W, _ = f.shape
    h, w = H // 4, W // 4
    Y = 4 * 7 + 1
    assert HB_TI + 1 < X // 4 < 2 * HB_TI - 1
    f, lab = f.copy(), lab.copy()
    f[0, Y, X, 3] = value
    ref_lab = lab.copy()
    ref_lab[0, Y, X] = 255
    lab[0, Y, X] = 3
    must = np.zeros((B, h, w), bool)
    My, Mx = lerp4(H, h), lerp4(W, w)
    must[0] = np.outer(My[Y] > 0, Mx[X] > 0)
    assert 1 <= must.sum() <= 4
    return f, lab, ref_lab, P, must


# ---------------------------------------------------------------------------------------------------------------------
# the loss kernels' cases
# ---------------------------------------------------------------------------------------------------------------------
# name, B, K, H, W, ignore_index, which pixels are ignored, regimes
LOSS_CASES = [
    # what tests/test_gpu_ops.py's LOSS_CASES has
    ("hw1_65x97", 2, 16, 65, 97, 255, "5%", ("spread", "close")),
    ("hw3_31x33_k32", 2, 32, 31, 33, 255, "5%", ("spread", "close")),
    ("hw0_50x34_k13", 3, 13, 50, 34, -1, "5%", ("spread", "close")),
    ("hw3_7x9_image1_ignored", 2, 21, 7, 9, 255, "image1", ("spread", "close")),
    ("hw1_513_grid_stride", 4, 16, 513, 513, 255, "5%", ("spread",)),
    # K = 1: the loss is alpha VAR / n, the cross-entropy gradient 0
    ("k1_hw3", 2, 1, 5, 7, 255, "5%", ("spread",)),
    ("k1_hw0", 2, 1, 6, 10, 255, "5%", ("spread",)),
    ("k19", 2, 19, 6, 10, 255, "5%", ("spread", "close")),
    ("k40", 1, 40, 5, 7, -1, "5%", ("spread", "close")),
    # H W % 4 in {1, 3, 2, 0, 2, 0}
    ("hw1_3x3", 2, 16, 3, 3, 255, "5%", ("close",)),
    ("hw3_3x5", 2, 16, 3, 5, 255, "5%", ("close",)),
    ("hw2_3x6", 2, 16, 3, 6, 255, "5%", ("close",)),
    ("hw0_4x5", 2, 16, 4, 5, 255, "5%", ("close",)),
    ("hw2_5x6", 2, 16, 5, 6, 255, "5%", ("close",)),
    ("hw0_6x10", 2, 16, 6, 10, 255, "5%", ("close",)),
    # exact ties at the maximum: two planes and all K, the label on the first and on the second (sums[3] counts the first only)
    ("ties_hw0", 2, 5, 4, 6, 255, "5%", ("ties",)),
    ("ties_hw3", 2, 5, 5, 7, 255, "5%", ("ties",)),
    # one non-finite logit per image
    ("nan_logit_hw0", 2, 16, 6, 10, 255, "5%", ("nan",)),
    ("nan_logit_hw3", 2, 16, 5, 7, 255, "5%", ("nan",)),
    ("neg_inf_plane0_hw0", 2, 16, 6, 10, 255, "5%", ("neg_inf_plane0",)),
    ("neg_inf_plane0_hw3", 2, 16, 5, 7, 255, "5%", ("neg_inf_plane0",)),
    ("neg_inf_plane_last_hw0", 2, 16, 6, 10, 255, "5%", ("neg_inf_plane_last",)),
    ("neg_inf_plane_last_hw3", 2, 16, 5, 7, 255, "5%", ("neg_inf_plane_last",)),
]
# above the caps, K = 2.  The smallest with a second trip: 2048 * 256 + 1 = 3 * 174763 four-pixel items (forward), 8192 * 256 + 1 =
# 3 * 699051 items (backward: four-pixel and one-pixel).  The vector backward needs 8 388 612 pixels: 67 MB each of logits, gradient
# and int64 labels, 201 MB on the device -- with K = 2 nothing smaller makes a second trip.
BIG_CASES = [
    ("big_fwd_vector", 1, 2, 12, 174763, 255, "5%", ("spread",)),
    ("big_bwd_vector", 1, 2, 12, 699051, 255, "5%", ("spread",)),
    ("big_bwd_scalar", 1, 2, 3, 699051, 255, "5%", ("spread",)),
]
BIG_REACH = {"big_fwd_vector": ("fwd", 4), "big_bwd_vector": ("bwd", 4), "big_bwd_scalar": ("bwd", 1), "hw1_513_grid_stride": ("fwd", 1)}


def loss_input(case, regime):
    """(logits[B, K, H, W] float32, labels[B, H, W] int64).  spread: minus squared distances of order 10 .. 300; close: of order 1e4 with
    a runner-up within 1 of the top; ties: small integers with two-way and K-way ties at the maximum; nan / neg_inf_*: spread with one
    such logit per image at a valid pixel whose label is another plane"""
    name, B, Kk, H, W, ign, which = case[:7]
    rs = np.random.RandomState(_seed(B, Kk, H, W % 9973, len(regime), ord(regime[0]), len(name)))
    n = B * H * W
    lab = rs.randint(0, Kk, (B, H, W)).astype(np.int64)
    if which == "image1":
        lab[1] = ign
    else:
        lab[rs.rand(B, H, W) < 0.05] = ign
    if regime == "close":
        lg = -(1e4 + 300.0 * rs.rand(n, Kk))
        k2 = rs.randint(0, Kk, n)
        lg[np.arange(n), k2] = lg.max(1) - 0.99 * rs.rand(n)
    elif regime == "ties":
        lg = -rs.randint(10, 50, (n, Kk)).astype(F64)
        kind = np.arange(n) % 4                                                # two-way / K-way tie, label on the first / second
        a = rs.randint(0, Kk - 1, n)
        b = a + 1 + rs.randint(0, Kk, n) % (Kk - 1 - a)
        two = kind < 2
        lg[two, a[two]] = -5.0
        lg[two, b[two]] = -5.0
        lg[~two] = -7.0
        labf = np.where(two, np.where(kind == 0, a, b), np.where(kind == 2, 0, 1))
        lab = np.where(lab == ign, ign, labf.reshape(B, H, W)).astype(np.int64)
    else:
        lg = -(10.0 + 290.0 * rs.rand(n, Kk))
    lg = np.ascontiguousarray(lg.astype(F32).reshape(B, H, W, Kk).transpose(0, 3, 1, 2))
    if regime in ("nan", "neg_inf_plane0", "neg_inf_plane_last"):
        plane = {"nan": 3, "neg_inf_plane0": 0, "neg_inf_plane_last": Kk - 1}[regime]
        for b in range(B):
            y, x = (b + 1) % H, (2 * b + 3) % W
            lab[b, y, x] = (plane + 5) % Kk
            lg[b, plane, y, x] = np.nan if regime == "nan" else -np.inf
    return lg, lab


def nonfinite_pixels(lg):
    """[B, H, W]: pixels with a NaN logit"""
    return np.isnan(lg).any(1)


def cases_reach():
    """asserts that every above-the-cap case makes a second trip of its kernel's grid-stride loop (the new ones exactly two), with the
    pixels per item its name says, inside the memory the issue allows; returns {name: trips}"""
    out = {}
    for case in LOSS_CASES + BIG_CASES:
        name, B, Kk, H, W = case[:5]
        if name not in BIG_REACH:
            assert loss_launch("fwd", B, H, W)[2] == 1 and loss_launch("bwd", B, H, W)[2] == 1, name
            continue
        entry, px = BIG_REACH[name]
        got_px, grid, trips = loss_launch(entry, B, H, W)
        assert got_px == px and trips >= 2 and grid == (MAX_BLOCKS if entry == "fwd" else BWD_BLOCKS), (name, got_px, grid, trips)
        assert trips == 2 or name == "hw1_513_grid_stride", name
        assert B * H * W // px == grid * 256 + 1 or name == "hw1_513_grid_stride", name     # the smallest
        out[name] = trips
    return out


def compare(what, got, ref, bar, exact=False):
    """head_cases.check_close in slices of 2^21 elements (the above-the-cap gradients): (error, bar) of the largest share"""
    best = (0.0, 0.0)
    got, ref, bar = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1), None if bar is None else np.asarray(bar).reshape(-1)
    assert got.shape == ref.shape, "%s: %d elements, expected %d" % (what, got.size, ref.size)
    for at in range(0, ref.size, 1 << 21):
        sl = slice(at, at + (1 << 21))
        e, b = HC.check_close(what, got[sl], ref[sl], None if bar is None else bar[sl], exact)
        if b > 0 and (best[1] == 0 or e / b > best[0] / best[1]):
            best = (e, b)
    return best
