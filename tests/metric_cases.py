"""The Inter and Center terms of the reference's utils/loss.py:43-79 as a float64 definition on float32 inputs, the bars the HIP
kernels (csrc/metric_terms.hip) are held to, and the case table.  tests/test_metric_refs.py proves the definition against the
reference's statements without a GPU; tests/test_gpu_metric_terms.py holds the kernels to it.

Definition.  L [B,K,H,W] logits, F [B,H,W,C] features taken flat over H W, y [B,H,W] labels, N = H W (every pixel of an image,
the ignored ones too), a pixel valid when y != ignore_index.  For image i and class c with n_ic >= 1 pixels
    mu_ic    = (1 / n_ic) sum_{p: y_p = c} F[i,p,:]
    Inter_i  = (1 / N) sum_{valid p} sum_{k != y_p} L[i,k,p]
    Center_i = (1 / N) sum_{valid p} |F[i,p,:] - mu_{i,y_p}|^2
    term     = (beta sum_i Inter_i + gamma sum_i Center_i) / n
    d term / d L[i,k,p] = gout beta / (n N) on a valid pixel for k != y_p, else 0
    d term / d F[i,p,:] = gout 2 gamma / (n N) (F[i,p,:] - mu_{i,y_p}) on a valid pixel, else 0
beta and gamma are the float32 values the C ABI takes.

Bars (eps = 2^-24), from the roundings a float32 evaluation makes in the launch shapes documented in include/dmlnet_hip.h, never
from an output of the kernels.  A float32 addition errs by at most eps times the magnitude of its result, which is at most the
sum A of the magnitudes of the terms; a chain of m additions onto 0 makes m - 1 roundings (0 + x is exact).
    mu:      a lane of the class-sum launch adds at most D1 = ceil(N / (workgroups 4 waves 64/CP pixels)) terms, and never more
             than the class has (n); everything after the lane is double.  |sum error| <= (min(D1, n) - 1) eps A, A = sum |F| over
             the class; the mean is stored as float32: eps |mu|.  dmu = eps (min(D1, n) A / n + |mu|), one eps A / n spare.
             dmu = 0 where the sum is exact: a class of one pixel, or a channel that is constant over the class with every
             multiple j v, j <= n, a float32 (then every partial sum is exact, and so are the double fold and the division).
    Center:  the kernel takes d' = fl(F - mu') with mu' = mu + e, |e| <= dmu, squares and adds.  sum (d - e)^2 = sum d^2 - 2 e sum d
             + n e^2, and sum d = 0 over a class, so the stored mean enters at second order: n dmu^2 per class and channel.  The
             cross term comes back through the roundings only: d' and the square carry 3 eps relative, so 6 eps dmu sum |d|.
             The squares themselves: 3 eps each, then the chain -- 4 additions per group of four floats a lane takes, D3 groups
             per lane, 6 in the wave's butterfly, 3 across the waves -- each at most eps of the whole sum S' = S + n dmu^2 summed.
             bar(N Center_i) = sum_{k,c} (n dmu^2 + 6 eps dmu sum |d|) + (4 + 4 D3 + 9) eps S', one eps spare.
    Inter:   K additions per pixel, 4 per group of four pixels a lane takes (D4 groups), 9 to the workgroup's partial:
             bar(N Inter_i) = (K + 4 D4 + 9 + 1) eps A_i, A_i = sum over valid pixels and k != y of |L|.
    term:    the double combination of the per-image bars, plus eps |term| for its float32 store.
    d / d L: the weight is rounded to float32 once: eps |w| (plus float32's smallest step).  Added into a buffer x the sum rounds once
             more: eps |x + w|.
    d / d F: w' fl(F - mu'): |w| dmu + 4 eps |g| (the weight, the subtraction, the product, one spare), plus the smallest step.
An element whose bar is 0 -- an ignored pixel, the own-class logit of a pixel, a one-pixel class, an exactly constant class -- must
be exactly 0.
"""
import functools

import numpy as np

import helpers as HP

F64 = np.float64
EPS32 = 2.0 ** -24
STEP32 = 2.0 ** -149
METRIC_BLOCKS = 2048


def _grid(items, per, B):
    return max(1, min((items + per - 1) // per, METRIC_BLOCKS // B))


def chain_depths(B, Hh, Ww, K, C, with_feats=True, with_logits=True):
    """(D1, D3, D4): terms per lane of the class-sum launch, groups of four floats and groups of four pixels per lane of the terms
    launch (its workgroups per image are the larger of the two loops' needs)"""
    N = Hh * Ww
    cp = 1
    while cp < C:
        cp *= 2
    ppw = 64 // cp
    bpi1 = _grid(N, 4 * ppw, B)
    d1 = -(-N // (bpi1 * 4 * ppw))
    groups, quads = (N * C + 3) // 4, (N + 3) // 4
    bpi = max(_grid(groups, 256, B) if with_feats else 1, _grid(quads, 256, B) if with_logits else 1)
    return d1, -(-groups // (256 * bpi)), -(-quads // (256 * bpi))


def _exact_constant(v, n):
    """every multiple j v, j <= n, is a float32: a chain of additions of v is exact"""
    j = np.arange(1, n + 1, dtype=F64)
    return bool((np.float32(j * v).astype(F64) == j * v).all())


def metric_ref(L, F, y, ignore_index, beta, gamma, gout=1.0, n=None, chain="kernel", mutant=None, with_feats=True,
               with_logits=True):
    """The definition and its bars.  chain="kernel": the documented launch shapes; "any": the bound of ANY order of float32
    summation (m terms: m - 1 roundings), for evaluations that sum in another order.  `mutant` names a likely mistake, for
    tests/test_metric_refs.py only.  with_feats / with_logits False: that input is not given, its term is 0."""
    B, K, Hh, Ww = L.shape
    C = F.shape[3]
    N = Hh * Ww
    n = float(B if n is None else n)
    beta, gamma = float(np.float32(beta)), float(np.float32(gamma))
    Ld = L.astype(F64).reshape(B, K, N)
    Fd = F.astype(F64).reshape(B, N, C)
    yy = y.reshape(B, N)
    valid = yy != ignore_index
    d1, d3, d4 = chain_depths(B, Hh, Ww, K, C, with_feats, with_logits)
    means = np.zeros((B, K, C), dtype=F64)
    dmu = np.zeros((B, K, C), dtype=F64)
    counts = np.zeros((B, K), dtype=np.int64)
    inter, inter_bar = np.zeros(B), np.zeros(B)
    center, center_bar = np.zeros(B), np.zeros(B)
    dev = np.zeros((B, N, C), dtype=F64)
    dmu_px = np.zeros((B, N, C), dtype=F64)
    own = np.zeros((B, K, N), dtype=bool)
    div = np.full(B, float(N))
    if mutant == "divisor = valid pixels":
        div = np.maximum(valid.sum(axis=1), 1).astype(F64)
    for i in range(B):
        classes = list(range(K))
        lab = yy[i].copy()
        ok = valid[i].copy()
        if mutant == "ignored pixels counted":
            lab = np.where(ok, lab, K)                      # a class of their own, as the reference's loop without its `continue`
            ok = np.ones_like(ok)
            classes.append(K)
        own[i] = (np.arange(K)[:, None] == lab[None, :]) & ok[None, :]
        if mutant == "own class in Inter":
            own[i] = False
        if with_logits:
            others = np.where(own[i] | ~ok[None, :], 0.0, Ld[i])
            inter[i] = others.sum() / div[i]
            A = np.abs(others).sum() if chain == "kernel" else np.abs(Ld[i] * ok[None, :]).sum()
            depth = (K + 4 * d4 + 9 + 1) if chain == "kernel" else ok.sum() * K + 4
            inter_bar[i] = depth * EPS32 * A / N
        if not with_feats:
            continue
        S, second = 0.0, 0.0
        for k in classes:
            sel = (lab == k) & ok
            nk = int(sel.sum())
            if k < K:
                counts[i, k] = nk
            if nk == 0:
                continue
            Fk = Fd[i][sel]
            mu = Fk.mean(axis=0)
            if mutant == "mean over the batch":
                allsel = (yy == k) & valid
                mu = Fd[allsel].mean(axis=0)
            dk = Fk - mu
            A = np.abs(Fk).sum(axis=0)
            m = min(d1, nk) if chain == "kernel" else nk
            e = EPS32 * (m * A / nk + np.abs(mu))
            for c in range(C):
                if nk == 1 or (Fk[:, c].min() == Fk[:, c].max() and _exact_constant(Fk[0, c], nk)):
                    e[c] = 0.0
            if k < K:
                means[i, k], dmu[i, k] = mu, e
            dev[i][sel] = dk
            dmu_px[i][sel] = e
            S += (dk * dk).sum() + (nk * e * e).sum()
            second += (nk * e * e + 6 * EPS32 * e * np.abs(dk).sum(axis=0)).sum()
        center[i] = (dev[i] ** 2).sum() / div[i]
        depth = (4 + 4 * d3 + 9) if chain == "kernel" else 4 + int(valid[i].sum()) * C
        center_bar[i] = (second + depth * EPS32 * S) / N
    if mutant == "Center as sum F^2 - n mu^2 in float32":
        f32 = np.float32
        for i in range(B):
            tot = f32(0)
            for k in range(K):
                sel = (yy[i] == k) & valid[i]
                if not sel.any():
                    continue
                Fk = F.reshape(B, N, C)[i][sel].astype(f32)
                mu = Fk.mean(axis=0, dtype=f32)
                tot = f32(tot + f32((Fk * Fk).sum(dtype=f32) - f32(f32(sel.sum()) * (mu * mu).sum(dtype=f32))))
            center[i] = float(tot) / N
    term = (beta * inter.sum() + gamma * center.sum()) / n
    term_bar = (abs(beta) * inter_bar.sum() + abs(gamma) * center_bar.sum()) / n + EPS32 * abs(term)
    wl = gout * beta / (n * div)
    wf = gout * 2.0 * gamma / (n * div)
    vmask = (yy != ignore_index) if mutant != "ignored pixels counted" else np.ones_like(valid)
    gl = np.where(own | ~vmask[:, None, :], 0.0, wl[:, None, None]) if with_logits else np.zeros((B, K, N))
    gl_bar = np.where(gl != 0, EPS32 * np.abs(gl) + STEP32, 0.0)
    gf = wf[:, None, None] * dev
    if mutant in ("mu path of the own pixel only", "mu path twice"):
        nk_px = np.ones((B, N))
        for i in range(B):
            for k in range(K):
                sel = (yy[i] == k) & valid[i]
                nk_px[i][sel] = sel.sum()
        gf = gf * (1.0 - (1.0 if mutant.endswith("only") else 2.0) / nk_px)[..., None]
    gf_bar = np.abs(wf)[:, None, None] * dmu_px + 4 * EPS32 * np.abs(gf)
    gf_bar = np.where(gf_bar > 0, gf_bar + STEP32, 0.0)
    sums = np.zeros(2 * B + 3, dtype=F64)
    sums[0:2 * B:2], sums[1:2 * B:2] = inter, center
    sums[2 * B], sums[2 * B + 1], sums[2 * B + 2] = inter.sum(), center.sum(), B
    return dict(term=term, term_bar=term_bar, inter=inter, inter_bar=inter_bar, center=center, center_bar=center_bar,
                means=means, means_bar=dmu, counts=counts, gl=gl.reshape(L.shape), gl_bar=gl_bar.reshape(L.shape),
                gf=gf.reshape(F.shape), gf_bar=gf_bar.reshape(F.shape), sums=sums, valid=valid.reshape(y.shape))


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
# labels: "mix" about 15 % ignored, the rest uniform; "edges": image 0 has class 1 on exactly one pixel and no class 0, image 1 is
# entirely ignored, image 2 is class 0 alone but for three ignored pixels
# features: "trained" 3 e_y + N(0, 0.3^2); "offset" 50 + N(0, 0.01^2) in every channel; "constant" (y + c % 4) / 4 on the valid pixels
CASES = {
    "1x1":            dict(B=1, H=1, W=1, K=2, C=1, ignore=255, labels="mix", feats="trained", beta=1e-4, gamma=1e-2, gout=1.0),
    "3x5 edges":      dict(B=3, H=3, W=5, K=16, C=5, ignore=-1, labels="edges", feats="trained", beta=1e-4, gamma=1e-2, gout=-2.5),
    "17x23 edges":    dict(B=3, H=17, W=23, K=17, C=17, ignore=255, labels="edges", feats="trained", beta=1e-4, gamma=1e-2, gout=0.75),
    "17x23 narrow":   dict(B=1, H=17, W=23, K=2, C=1, ignore=255, labels="mix", feats="trained", beta=0.0, gamma=1e-2, gout=-2.5),
    "17x23 offset":   dict(B=3, H=17, W=23, K=16, C=16, ignore=255, labels="mix", feats="offset", beta=1e-4, gamma=1e-2, gout=-2.5),
    "17x23 constant": dict(B=3, H=17, W=23, K=17, C=17, ignore=-1, labels="mix", feats="constant", beta=1e-4, gamma=1e-2, gout=0.75),
    "96x160":         dict(B=3, H=96, W=160, K=16, C=16, ignore=255, labels="mix", feats="trained", beta=1e-4, gamma=1e-2, gout=-2.5),
    "96x160 edges":   dict(B=3, H=96, W=160, K=16, C=5, ignore=-1, labels="edges", feats="trained", beta=1e-4, gamma=1e-2, gout=0.75),
    "96x160 wide":    dict(B=1, H=96, W=160, K=32, C=32, ignore=-1, labels="mix", feats="trained", beta=1e-4, gamma=0.0, gout=-2.5),
    "96x160 offset":  dict(B=1, H=96, W=160, K=32, C=32, ignore=255, labels="mix", feats="offset", beta=0.0, gamma=1e-2, gout=1.0),
}
MUTANTS = {                                                 # likely mistake -> the case that must show it
    "divisor = valid pixels": "96x160",
    "own class in Inter": "96x160",
    "ignored pixels counted": "96x160",
    "mean over the batch": "96x160",
    "mu path of the own pixel only": "17x23 edges",
    "mu path twice": "17x23 edges",
    "Center as sum F^2 - n mu^2 in float32": "17x23 offset",
}


def make_inputs(name, B, H, W, K, C, ignore, labels, feats, seed=23, **_):
    g = HP.rng_for(seed, "metric." + name)
    N = H * W
    y = g.integers(0, K, size=(B, N)).astype(np.int64)
    r = g.random((B, N))
    y[r < 0.15] = ignore
    if N == 1:
        y[:] = 1                                            # the one pixel is valid
    if labels == "edges":
        y[0][y[0] == 0] = 2 % K                              # class 0 absent from image 0 ...
        y[0][y[0] == 1] = 2 % K
        y[0, N // 2] = 1                                     # ... and class 1 there on exactly one pixel
        if B >= 2:
            y[1] = ignore                                    # an image without a valid pixel
        if B >= 3:
            y[2] = 0                                         # an image of a single class: the one absent from image 0
            y[2, :3] = ignore
    yv = np.where(y == ignore, 0, y)
    if feats == "trained":
        f = 0.3 * g.standard_normal((B, N, C)) + 3.0 * (np.arange(C)[None, None, :] == yv[..., None])
    elif feats == "offset":
        f = 50.0 + 0.01 * g.standard_normal((B, N, C))
    else:
        f = (yv[..., None] + np.arange(C)[None, None, :] % 4) / 4.0
        f = np.where((y == ignore)[..., None], g.standard_normal((B, N, C)), f)
    f = np.ascontiguousarray(f.astype(np.float32).reshape(B, H, W, C))
    # logits: minus the squared distances to prototypes 3 e_k of a K-channel embedding around the label's prototype
    emb = 0.3 * g.standard_normal((B, N, K)) + 3.0 * (np.arange(K)[None, None, :] == yv[..., None])
    lg = -((emb[:, :, None, :] - 3.0 * np.eye(K)[None, None]) ** 2).sum(-1)
    lg = np.ascontiguousarray(lg.transpose(0, 2, 1).astype(np.float32).reshape(B, K, H, W))
    return lg, f, y.reshape(B, H, W)



@functools.lru_cache(maxsize=None)
def inputs(name):
    out = make_inputs(name, **CASES[name])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the definition on a case with the case's weights and gout: computed once, shared, read-only"""
    c = CASES[name]
    lg, f, y = inputs(name)
    ref = metric_ref(lg, f, y, c["ignore"], c["beta"], c["gamma"], gout=c["gout"], with_feats=c["gamma"] != 0,
                     with_logits=c["beta"] != 0)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref
