"""Case table shared by tests/test_bn_refs.py (CPU) and tests/test_gpu_bn_edges.py (GPU): the float64 definitions of the
BatchNorm contract of include/dmlnet_hip.h, the input generators, the case tables and the error bars derived from the
arithmetic a kernel is allowed to do.  A plain module (no fixtures, no hooks, numpy only); nothing here looks at a
kernel's output or imports the library.

eps32 = 2^-24 is float32's unit roundoff; a bfloat16 store is off by at most half an ulp of its binade (stored_bar).

Two kinds of input:
  exact  every value dyadic and small, so that every product and every partial sum of the contract is exact in float32
         in any order, contracted or not: the kernel must then EQUAL the float64 result (test_bn_refs.py proves the
         exactness on every case);
  real   seeded Gaussians with the channels that hurt (|mean| / std = 1e4, var << eps, std = 1e3, constant), compared
         against bars that count the float32 roundings of the contract.
"""
import numpy as np

F64 = np.float64
F32 = np.float32
EPS32 = 2.0 ** -24
BN_EPS = 1e-5
EXCLUDE_CAP = 1e-4                            # share of elements whose ReLU / mask decision may lie inside its bar
STAT_ROWS = 64                                # rows of one dml_bn_stats partial (DML_STAT_ROWS)
RED_MAX_ROWS = 1024                           # the exact cases stay exact while a backward partial covers <= this many rows


def vec(dtype):
    """elements of one 16-byte vector"""
    return 8 if dtype == "bf16" else 4


def bf16_round(x):
    """round-to-nearest-even to bfloat16, returned as float32 (finite values)"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F32).reshape(np.shape(x))


def store(x, dtype):
    """the value a kernel's output buffer of `dtype` holds for the exact (float64) result x"""
    x32 = np.asarray(x, F64).astype(F32)
    return bf16_round(x32) if dtype == "bf16" else x32


# ---------------------------------------------------------------------------------------------------------------------
# the contract, float64
# ---------------------------------------------------------------------------------------------------------------------
def fwd_ref(y, res, mean, scale, shift, relu, keep=None, keep_scale=1.0):
    """z = act((y - mean) scale + shift [+ res]) [dropout: kept elements times keep_scale, the others 0]; returns
    (z, pre) with pre the value before the activation"""
    pre = (np.asarray(y, F64) - np.asarray(mean, F64)) * np.asarray(scale, F64) + np.asarray(shift, F64)
    if res is not None:
        pre = pre + np.asarray(res, F64)
    z = np.maximum(pre, 0.0) if relu else pre.copy()
    if keep is not None:
        z = np.where(keep, z * keep_scale, 0.0)
    return z, pre


def pack_mask(on, V):
    """[M, N] booleans -> [M, N / V] bytes: one byte per 16-byte vector, bit c % V"""
    M, N = on.shape
    b = on.reshape(M, N // V, V).astype(np.uint16)
    return (b << np.arange(V, dtype=np.uint16)).sum(-1).astype(np.uint8)


def unpack_mask(mask, V):
    M, NV = mask.shape
    return ((mask[:, :, None] >> np.arange(V, dtype=np.uint8)) & 1).astype(bool).reshape(M, NV * V)


def bwd_g(dz, on, gscale):
    """g = dz [z > 0] gscale"""
    g = np.asarray(dz, F64) * gscale
    return g if on is None else np.where(on, g, 0.0)


def bwd_sums(g, y, mean, invstd):
    """(sum g, sum g xhat) per channel, [2, N]"""
    xhat = (np.asarray(y, F64) - np.asarray(mean, F64)) * np.asarray(invstd, F64)
    return np.stack([g.sum(0), (g * xhat).sum(0)])


def bwd_coef(sums, gamma, mean, invstd, M):
    """coef[4][N] of dy = c0 g + c1 (y - c3) + c2; M = 0: a layer that normalised with fixed statistics"""
    gam = np.ones_like(np.asarray(invstd, F64)) if gamma is None else np.asarray(gamma, F64)
    inv = np.asarray(invstd, F64)
    A = gam * inv
    if M > 0:
        c1, c2 = -A * inv * sums[1] / M, -A * sums[0] / M
    else:
        c1, c2 = np.zeros_like(A), np.zeros_like(A)
    return np.stack([A, c1, c2, np.asarray(mean, F64)])


def bwd_apply_ref(g, y, coef):
    coef = np.asarray(coef, F64)
    return coef[0] * g + coef[1] * (np.asarray(y, F64) - coef[3]) + coef[2]


def batch_stats(y):
    """(mean, biased variance) over the rows, float64"""
    y = np.asarray(y, F64)
    return y.mean(0), y.var(0)


# ---------------------------------------------------------------------------------------------------------------------
# group partials and their merge
# ---------------------------------------------------------------------------------------------------------------------
def group_rows(M, stat_rows):
    G = (M + stat_rows - 1) // stat_rows
    rows = np.full(G, stat_rows, np.int64)
    rows[-1] = M - (G - 1) * stat_rows
    return rows


def partials(y, stat_rows):
    """[G, N, 2] float64: (sum, M2 about the group's own mean) of every group of stat_rows rows"""
    y = np.asarray(y, F64)
    M, N = y.shape
    out = np.empty((len(group_rows(M, stat_rows)), N, 2), F64)
    for g in range(out.shape[0]):
        blk = y[g * stat_rows:(g + 1) * stat_rows]
        out[g, :, 0] = blk.sum(0)
        out[g, :, 1] = ((blk - blk.mean(0)) ** 2).sum(0)
    return out


def chan_merge(part, rows):
    """Chan et al. pairwise merge in float64 of part[G, N, 2] = (sum, M2), rows[G] rows each -> (count, mean, M2).
    A different algorithm from the kernel's Q + P - S^2 / M on purpose."""
    part = np.asarray(part, F64)
    n = np.asarray(rows, F64)[:, None] * np.ones((1, part.shape[1]))
    mean = part[:, :, 0] / n
    m2 = part[:, :, 1].copy()
    while n.shape[0] > 1:
        if n.shape[0] & 1:                     # an odd one out joins the next round unchanged
            n = np.concatenate([n, np.zeros_like(n[:1])])
            mean = np.concatenate([mean, np.zeros_like(mean[:1])])
            m2 = np.concatenate([m2, np.zeros_like(m2[:1])])
        na, nb = n[0::2], n[1::2]
        nn = na + nb
        d = mean[1::2] - mean[0::2]
        mean = mean[0::2] + d * (nb / nn)
        m2 = m2[0::2] + m2[1::2] + d * d * (na * nb / nn)
        n = nn
    return n[0], mean[0], m2[0]


def finalize_ref(count, mean, m2, gamma, beta, rm, rv, momentum, eps=BN_EPS):
    """what dml_bn_finalize writes, float64, from merged moments; `momentum` is the float32 the kernel gets.  Returns a dict
    of value and, per output, the magnitudes its bar is built from."""
    mom = float(F32(momentum))
    eps = float(F32(eps))                      # ... and the float32 eps
    var_b = m2 / count
    var_u = m2 / (count - 1.0) if count > 1 else var_b
    invstd = 1.0 / np.sqrt(var_b + eps)
    gam = np.ones_like(mean) if gamma is None else np.asarray(gamma, F64)
    out = {"mean": mean, "invstd": invstd, "scale": gam * invstd,
           "shift": np.zeros_like(mean) if beta is None else np.asarray(beta, F64)}
    one_m = float(F32(1.0) - F32(momentum))    # the kernel forms 1 - momentum in float32
    if rm is not None:
        out["running_mean"] = one_m * np.asarray(rm, F64) + mom * mean
        out["running_mean_mag"] = np.abs(one_m * np.asarray(rm, F64)) + np.abs(mom * mean)
    if rv is not None:
        out["running_var"] = one_m * np.asarray(rv, F64) + mom * var_u
        out["running_var_mag"] = np.abs(one_m * np.asarray(rv, F64)) + np.abs(mom * var_u)
    out["cancel"] = 1e-13 * (1.0 + mean * mean / (var_b + eps))      # float64 cancellation of Q + P - S^2 / M, relative to var
    return out


def finalize_bars(ref):
    """elementwise bars of dml_bn_finalize's outputs against finalize_ref: the final float32 roundings only (one for mean and
    invstd, two for scale, four for a running update, whose 1 - momentum is exact in the reference) plus the float64
    cancellation term, which reaches invstd with factor 1/2 and the variance with factor 1."""
    c = ref["cancel"]
    bars = {"mean": EPS32 * np.abs(ref["mean"]) + 1e-13 * np.abs(ref["mean"]) + 1e-300,
            "invstd": (EPS32 + 0.5 * c) * np.abs(ref["invstd"]),
            "scale": (2 * EPS32 + 0.5 * c) * np.abs(ref["scale"]),
            "shift": np.zeros_like(ref["mean"])}
    if "running_mean" in ref:
        bars["running_mean"] = 4 * EPS32 * ref["running_mean_mag"] + 1e-13 * np.abs(ref["mean"])
    if "running_var" in ref:
        bars["running_var"] = (4 * EPS32 + c) * ref["running_var_mag"]
    return bars


def stats_bars(y, stat_rows=STAT_ROWS):
    """bars of dml_bn_stats' float32 partials against partials(y): a sequential float32 sum of n <= stat_rows terms is within
    (n - 1) eps32 sum |y| of the exact one; the mean s / n adds one rounding, so it is off by at most
    delta = ((n - 1) eps32 sum |y|) / n + eps32 |mean|; then sum (y - mean')^2 = M2 + n delta^2 exactly, every term
    fl(fl(y - mean')^2) carries three roundings and the sum n - 1 more.  Returns (sum_bar, m2_bar), each [G, N]."""
    y = np.asarray(y, F64)
    M, N = y.shape
    rows = group_rows(M, stat_rows)
    sb, mb = np.empty((len(rows), N)), np.empty((len(rows), N))
    for g, n in enumerate(rows):
        blk = y[g * stat_rows:(g + 1) * stat_rows]
        sb[g] = (n - 1) * EPS32 * np.abs(blk).sum(0)
        delta = sb[g] / n + EPS32 * np.abs(blk.mean(0))
        m2p = ((np.abs(blk - blk.mean(0)) + delta) ** 2).sum(0)
        mb[g] = n * delta ** 2 + (n + 2) * EPS32 * m2p * (1 + 8 * EPS32)
        if n == 1:
            sb[g], mb[g] = 0.0, 0.0           # one row: s = y and y - y = 0, exactly
    return sb, mb


def merged_bars(part, rows, sum_bar, m2_bar):
    """how far the mean and M2 merged from partials may move when every partial moves inside its bar: (mean_bar, m2_bar) per
    channel.  M2 = sum M2_g + sum n_g (mean_g - mean)^2 and d/ds_g of the second sum is 2 (mean_g - mean); second order kept."""
    part = np.asarray(part, F64)
    n = np.asarray(rows, F64)[:, None]
    cnt, mean, _ = chan_merge(part, rows)
    mean_bar = sum_bar.sum(0) / cnt
    dev = np.abs(part[:, :, 0] / n - mean) + mean_bar
    return mean_bar, m2_bar.sum(0) + (2 * dev * sum_bar + sum_bar ** 2 / n).sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# plane scale of a bound, fp16 planes
# ---------------------------------------------------------------------------------------------------------------------
def root_count(count):
    return np.sqrt(float(count)) * 1.0001


def fwd_bound(gamma, beta, N, count, mult=1.0, res_max=0.0):
    g = np.ones(N) if gamma is None else np.abs(np.asarray(gamma, F64))
    b = np.zeros(N) if beta is None else np.abs(np.asarray(beta, F64))
    with np.errstate(invalid="ignore"):
        return float((g * root_count(count) + b).max() * mult + res_max)


def bwd_bound(coef, invstd, count, gmax):
    c = np.abs(np.asarray(coef, F64))
    return float((c[0] * gmax + c[1] * root_count(count) / np.asarray(invstd, F64) + c[2]).max())


def unscale_of_bound(b):
    """work[1024] = 1 / s, s the power of two that puts b * (1 + 2^-10) into [2^14, 2^15); 1 for b = 0 or a non-finite b"""
    if b == 0 or not np.isfinite(b):
        return 1.0
    return 2.0 ** (int(np.floor(np.log2(b * 1.0009765625))) - 14)


def bound_margin(b):
    """relative distance of b (1 + 2^-10) from the nearest power of two"""
    m = np.log2(b * 1.0009765625)
    return abs(2.0 ** (m - np.round(m)) - 1.0)


def h2_planes(x, unscale):
    """dml_h2_split's arithmetic on float32 x: hi = fp16(x / unscale), lo = fp16(x / unscale - hi), round-to-nearest-even"""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = np.asarray(x, F32) * F32(1.0 / unscale)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(F32)).astype(np.float16)
    return hi, lo


# ---------------------------------------------------------------------------------------------------------------------
# exact inputs
# ---------------------------------------------------------------------------------------------------------------------
SCALES = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0])
GSCALE = 2.0


def _grid(rs, lo, hi, step, shape):
    return rs.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape).astype(F64) * step


def exact_inputs(M, N, seed=0, fine_res=False):
    """Dyadic inputs (float64 arrays whose values are float32- and bfloat16-exact): y, res, dz multiples of 1/4 in [-8, 8], mean a
    multiple of 1/4, scale in SCALES, shift a multiple of 1/8, invstd a power of two; coef: dyadic backward coefficients (c0 in SCALES, c1 a multiple of 2^-8, c2 of 1/8, c3 = mean).
    Channel 0 has shift 0 and scale 1, and y = mean, res = 0 in row 0 and every 7th row after: z is exactly 0 there.  Channel 1
    has scale -2, channel 2 scale 0.  fine_res: res a multiple of 2^-12 instead (z then needs more than fp16's 11 bits, so
    that the lo plane is not all zero)."""
    rs = np.random.RandomState(1000 + 7 * seed + 13 * N + M % 9973)
    d = {"y": _grid(rs, -8, 8, 0.25, (M, N)), "dz": _grid(rs, -8, 8, 0.25, (M, N)),
         "res": _grid(rs, -8, 8, 2.0 ** -12 if fine_res else 0.25, (M, N)),
         "mean": _grid(rs, -2, 2, 0.25, N), "scale": SCALES[rs.randint(0, len(SCALES), N)].copy(),
         "shift": _grid(rs, -1, 1, 0.125, N), "invstd": 2.0 ** rs.randint(-1, 2, N).astype(F64)}
    d["scale"][0], d["shift"][0] = 1.0, 0.0
    d["y"][0::7, 0] = d["mean"][0]
    d["res"][0::7, 0] = 0.0
    d["scale"][1] = -2.0
    d["scale"][2] = 0.0
    # (c1 a multiple of 2^-8: dy then needs more than fp16's 11 bits, so that its lo plane is not all zero)
    d["coef"] = np.stack([SCALES[rs.randint(0, len(SCALES), N)], _grid(rs, -1, 1, 2.0 ** -8, N), _grid(rs, -1, 1, 0.125, N), d["mean"]])
    d["dres0"] = _grid(rs, -8, 8, 0.25, (M, N))      # what an accumulating dres holds beforehand
    return d


def shape_table(V):
    """(N, M) with V the elements of a 16-byte vector (4: f32, 8: bf16)"""
    return [(V, 1), (V, 2), (V, 257), (V, 513),      # CB = 1; a second row block of one row
            (3 * V, 171),                             # RB = 85, one idle thread, last trip half valid
            (257 * V, 5), (512 * V, 3),               # two column chunks, the first with a one-column last chunk
            (16 * V, 33017)]                          # two trips of the row loop


def apply_shapes(dtype):
    return shape_table(4) if dtype == "f32" else [(8, 257), (24, 171), (72, 45)]


# planes-only forward (z == NULL), (N, M): eight channels per thread; 264 in a slice of pitch 304; 2056: two column chunks; 12 and 48 (the
# latter with a planes pointer 8- but not 16-byte aligned) fall back to the four-channel kernel
PLANES_SHAPES = [(8, 37), (24, 171), (264, 30), (2056, 3), (12, 37), (48, 30)]
# (the 264 channels sit at offset 40 of pitch 304, the 48 at offset 256: offset 256 + 264 channels would run into the next row)
# backward apply (N, M): 264 = two chunks of the four-channel kernel's 64 threads, 520 = two chunks of the eight-channel kernel
BWD_APPLY_SHAPES = [(264, 9), (520, 9), (48, 297), (12, 171), (528, 9), (24, 171)]

# y, res, z each in a channel slice of its own pitch: (N, M, (ldz, offz))
SLICES = {"f32": [(48, 30, (304, 256)), (256, 30, (1280, 1024))], "bf16": [(48, 30, (304, 256))]}


def slice_pitches(N, V):
    """(ldy, offy), (ldres, offres) of a slice case"""
    return (N + 3 * V, 2 * V), (N + V, 0)


# backward reduce: the forward table plus two column chunks (RED_COLS = 64 vector columns per block)
def reduce_shapes(dtype):
    return shape_table(vec(dtype)) + ([(264, 9)] if dtype == "f32" else [(528, 9)])


# ---------------------------------------------------------------------------------------------------------------------
# real-valued inputs
# ---------------------------------------------------------------------------------------------------------------------
REAL_SHAPES = [(297, 48), (2, 256)]


def real_inputs(M, N, dtype, seed=0):
    """float32 (bf16: bfloat16-rounded) y, res, dz and float32 gamma / beta.  Channel 0: |mean| / std = 1e4; channel 1: var << eps;
    channel 2: std = 1e3; channel 3: constant; gamma negative in channel 4, zero in channel 5."""
    rs = np.random.RandomState(77 + seed + M + 3 * N)
    std = rs.uniform(0.5, 2.0, N)
    mu = rs.standard_normal(N) * 3.0
    std[0], mu[0] = 1.0, 1e4
    std[1], mu[1] = 1e-5, 0.5
    std[2], mu[2] = 1e3, -40.0
    y = rs.standard_normal((M, N)) * std + mu
    y[:, 3] = 1.25
    q = (lambda a: bf16_round(a.astype(F32))) if dtype == "bf16" else (lambda a: a.astype(F32))
    gamma = rs.uniform(0.5, 1.5, N)
    gamma[4], gamma[5] = -gamma[4], 0.0
    return {"y": q(y), "res": q(rs.standard_normal((M, N)) * 1.5), "dz": q(rs.standard_normal((M, N))),
            "gamma": gamma.astype(F32), "beta": (rs.standard_normal(N) * 0.1).astype(F32)}


STATS_MS = (1, 63, 64, 65, 64 * 7 + 1)
STATS_NS = (4, 72)


def stats_inputs(M, N, dtype, seed=0):
    """float32 / bfloat16-rounded [M, N] with the four hard channels of real_inputs"""
    rs = np.random.RandomState(11 + seed + M + 5 * N)
    std, mu = rs.uniform(0.5, 2.0, N), rs.standard_normal(N) * 3.0
    std[:3], mu[:3] = (1.0, 1e-5, 1e3), (1e4, 0.5, -40.0)
    y = rs.standard_normal((M, N)) * std + mu
    y[:, 3] = 1.25
    return bf16_round(y.astype(F32)) if dtype == "bf16" else y.astype(F32)


def real_case(M, N, dtype, seed=0):
    """the float32 per-channel operands the kernels get for real_inputs: statistics of y in float64, rounded once"""
    d = real_inputs(M, N, dtype, seed)
    mean, var = batch_stats(d["y"])
    invstd = (1.0 / np.sqrt(var + BN_EPS)).astype(F32)
    d.update(mean=mean.astype(F32), invstd=invstd, scale=(d["gamma"].astype(F64) * invstd).astype(F32), shift=d["beta"])
    return d


def apply_bar(y, res, mean, scale, shift, dtype, dropout=False):
    """four float32 roundings (subtract, multiply, add, add), one more under dropout, times the magnitudes of the terms; bf16
    storage rounds the computed value once more"""
    mag = np.abs((np.asarray(y, F64) - np.asarray(mean, F64)) * np.asarray(scale, F64)) + np.abs(np.asarray(shift, F64))
    if res is not None:
        mag = mag + np.abs(np.asarray(res, F64))
    return (5 if dropout else 4) * EPS32 * mag


def stored_bar(bar32, ref, dtype):
    """bf16 storage rounds the computed value (within bar32 of ref) to nearest: half a bfloat16 ulp of its binade, 2^(e - 8) for a
    value in [2^e, 2^(e + 1)) -- between 2^-9 and 2^-8 of the value"""
    if dtype != "bf16":
        return bar32
    mag = np.abs(ref) + bar32
    with np.errstate(divide="ignore"):
        half_ulp = np.where(mag > 0, 2.0 ** (np.floor(np.log2(np.where(mag > 0, mag, 1.0))) - 8), 0.0)
    return bar32 + half_ulp


def reduce_bars(g, y, mean, invstd, n):
    """bars of the sums over all partial rows: a term g xhat carries four roundings (g, y - mean, two products), g itself one, and
    a float32 sum of the n rows of one partial, in any order, n - 1 more per term; the partial rows are added in float64."""
    xhat = (np.asarray(y, F64) - np.asarray(mean, F64)) * np.asarray(invstd, F64)
    return np.stack([(n - 1 + 1) * EPS32 * np.abs(g).sum(0), (n - 1 + 4) * EPS32 * np.abs(g * xhat).sum(0)])


def partial_rows_bound(M, nblocks):
    """most rows one backward partial can cover when nblocks equal blocks (the last one shorter) cover M rows"""
    return M if nblocks == 1 else (M - 1) // (nblocks - 1)


def bwd_apply_bar(g, y, coef, gscale):
    """c0 gscale dz: two roundings and two additions; c1 (y - c3): a subtraction, a product and two additions; c2: one addition
    at least -- four units on the sum of the magnitudes"""
    coef = np.asarray(coef, F64)
    return 4 * EPS32 * (np.abs(coef[0] * g) + np.abs(coef[1] * (np.asarray(y, F64) - coef[3])) + np.abs(coef[2]))


# ---------------------------------------------------------------------------------------------------------------------
# finalize from hand-built partials
# ---------------------------------------------------------------------------------------------------------------------
FIN_GS = (1, 63, 64, 65, 2047, 2048, 2049, 2176, 9216)
FIN_NS = (1, 3, 5, 72, 260)


def fin_combos(G):
    """(stat_rows, N, ragged last group, momentum, null) walked for one G: every N, and stat_rows, raggedness, momentum and the
    null pointer changing from one to the next"""
    nulls = ("none", "gamma", "beta", "running", "save_invstd")
    out = []
    for i, N in enumerate(FIN_NS):
        k = i + FIN_GS.index(G)
        out.append(((64, 48)[k % 2], N, (k // 2) % 2 == 0, (0.0, 0.1, 1.0)[k % 3], nulls[k % 5]))
    return out


def hand_partials(G, N, stat_rows, ragged, seed=0):
    """float32 partials [G, N, 2] of a tensor nobody needs to build: per group a float64 (sum, M2) drawn as the statistics of
    `rows` samples of N(mean_c, std_c^2) would fall, rounded once.  Channel 0 has |mean| / std = 1e4.  A ragged last group has one
    row and M2 = 0.  Returns (partials, rows, M)."""
    rs = np.random.RandomState(500 + seed + G + 31 * N + stat_rows)
    rows = np.full(G, stat_rows, np.int64)
    if ragged:
        rows[-1] = 1
    std = rs.uniform(0.3, 3.0, N)
    mu = rs.standard_normal(N) * 2.0
    mu[0] = 1e4 * std[0]
    n = rows[:, None].astype(F64)
    gmean = mu + std * rs.standard_normal((G, N)) / np.sqrt(n)
    m2 = std ** 2 * rs.chisquare(np.maximum(rows - 1, 1), (N, G)).T
    m2[rows == 1] = 0.0
    return np.stack([gmean * n, m2], -1).astype(F32), rows, int(rows.sum())


def fin_params(N, seed=0):
    rs = np.random.RandomState(900 + seed + N)
    gamma = rs.uniform(0.5, 1.5, N) * np.where(rs.rand(N) < 0.3, -1.0, 1.0)
    if N > 2:
        gamma[2] = 0.0
    return {"gamma": gamma.astype(F32), "beta": (rs.standard_normal(N) * 0.2).astype(F32),
            "rm": (rs.standard_normal(N) * 0.5).astype(F32), "rv": rs.uniform(0.5, 2.0, N).astype(F32)}


# dml_bn_bwd_finalize: exact partials
BWD_FIN_BLOCKS = (1, 64, 65, 2048, 2049, 9216)
BWD_FIN_NS = (1, 5, 260)


def bwd_hand_partials(nblocks, N, seed=0):
    """multiples of 1/4 in [-8, 8]: every sum of up to 9216 of them is exact in float32 and float64; dyadic gamma, invstd, mean and
    non-zero dyadic dgamma / dbeta to accumulate onto"""
    rs = np.random.RandomState(300 + seed + nblocks + 17 * N)
    return {"part": _grid(rs, -8, 8, 0.25, (nblocks, N, 2)).astype(F32),
            "gamma": SCALES[rs.randint(0, len(SCALES), N)].astype(F32), "invstd": (2.0 ** rs.randint(-2, 3, N)).astype(F32),
            "mean": _grid(rs, -2, 2, 0.25, N).astype(F32),
            "dgamma0": (_grid(rs, -4, 4, 0.5, N) + 0.25).astype(F32), "dbeta0": (_grid(rs, -4, 4, 0.5, N) + 0.25).astype(F32)}


# ---------------------------------------------------------------------------------------------------------------------
# synchronised pieces
# ---------------------------------------------------------------------------------------------------------------------
SYNC_RANKS, SYNC_M_EACH, SYNC_N = 3, 64 * 3 + 7, 12


def sync_inputs(seed=0):
    """three ranks whose means differ by many standard deviations: [ranks, M_each, N] float32"""
    rs = np.random.RandomState(41 + seed)
    std = rs.uniform(0.5, 2.0, SYNC_N)
    off = np.array([-30.0, 0.0, 55.0])[:, None, None] * std
    y = rs.standard_normal((SYNC_RANKS, SYNC_M_EACH, SYNC_N)) * std + off + rs.standard_normal(SYNC_N)
    return y.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# plane-scale bounds
# ---------------------------------------------------------------------------------------------------------------------
def bound_params(N, seed=0, small=False):
    """gamma / beta whose bound is far from a power of two (test_bn_refs.py checks every use)"""
    rs = np.random.RandomState(600 + seed + N)
    gamma = rs.uniform(0.2, 1.0, N) * np.where(rs.rand(N) < 0.4, -1.0, 1.0)
    beta = rs.standard_normal(N) * 0.3
    gamma[N // 2] = -1.37                      # the largest term, somewhere in the middle
    beta[N // 2] = -0.61
    if small:
        gamma, beta = gamma / 64.0, beta / 64.0
    return gamma.astype(F32), beta.astype(F32)


BOUND_COUNTS = (297, 1200)


REACH_MS = (2, 297)


def reach_case(M, N=8):
    """A tensor that drives xhat towards sqrt(count): one row of ones and M - 1 rows of zeros per channel, so that the ones are at
    xhat = sqrt(M - 1) (M = 2: 1); gamma and beta of equal sign, so that their terms add.  Returns y, dz (non-zero in that row only),
    gamma, beta."""
    y = np.zeros((M, N), F32)
    y[M // 2] = 1.0
    dz = np.zeros((M, N), F32)
    dz[M // 2] = np.linspace(-1.0, 1.0, N).astype(F32) + F32(0.07)
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    gamma = (sign * np.linspace(0.9, 1.45, N)).astype(F32)
    beta = (sign * np.linspace(0.05, 0.3, N)).astype(F32)
    return y, dz, gamma, beta


def words(value, at):
    """1024 amax words, all zero but `value` at index `at`"""
    w = np.zeros(1024, F32)
    w[at] = value
    return w


def fwd_bound_cases():
    """name -> (gamma, beta, N, count, mult, res_words); the expected scale is unscale_of_bound(fwd_bound(...))"""
    g4, b4 = bound_params(4)
    g260, b260 = bound_params(260)
    inf = g4.copy()
    inf[1] = np.inf
    return {"N4": (g4, b4, 4, 297, 1.0, None), "N260": (g260, b260, 260, 1200, 1.0, None),
            "null_gamma_beta": (None, None, 4, 297, 1.0, None), "mult2": (g260, b260, 260, 297, 2.0, None),
            "res_word0": (g4, b4, 4, 297, 1.0, words(77.5, 0)), "res_word1023": (g260, b260, 260, 297, 2.0, words(1234.5, 1023)),
            "all_zero": (np.zeros(4, F32), np.zeros(4, F32), 4, 297, 1.0, None), "inf_gamma": (inf, b4, 4, 297, 1.0, None)}


def fwd_bound_of(case):
    gamma, beta, N, count, mult, w = case
    return fwd_bound(gamma, beta, N, count, mult, 0.0 if w is None else float(w.max()))


def bwd_bound_cases():
    """name -> (coef[4, N], invstd, count, g_words)"""
    out = {}
    for name, N, count, at in (("N4", 4, 297, 0), ("N260", 260, 1200, 1023)):
        rs = np.random.RandomState(700 + N)
        coef = np.stack([rs.uniform(-2, 2, N), rs.uniform(-0.01, 0.01, N), rs.uniform(-0.1, 0.1, N), rs.standard_normal(N)]).astype(F32)
        out[name] = (coef, rs.uniform(0.3, 3.0, N).astype(F32), count, words(3.3, at))
    return out


def bwd_bound_of(case):
    coef, invstd, count, w = case
    return bwd_bound(coef, invstd, count, float(w.max()))


# the two fused finalize calls: (G, N, stat_rows, mult, residual word index or None)
FUSED_CASES = ((5, 4, 64, 1.0, None), (7, 260, 48, 2.0, 1023), (2049, 72, 64, 1.0, 0))
FUSED_RES_MAX = 19.25
BWD_FUSED_CASES = ((7, 4), (65, 260), (2049, 72))
BWD_FUSED_GMAX = 3.3


def bwd_fused_case(nb, N, f):
    """exact partials times the power of two f, max |g| = 3.3 f: (inputs, gmax, float64 bound with count = M = 64 nb - 5)"""
    h = bwd_hand_partials(nb, N)
    h = dict(h, part=(h["part"] * F32(f)).astype(F32))
    M = 64 * nb - 5
    sums = h["part"].astype(F64).sum(0).T
    return h, BWD_FUSED_GMAX * f, bwd_bound(bwd_coef(sums, h["gamma"], h["mean"], h["invstd"], M), h["invstd"], M, float(F32(BWD_FUSED_GMAX * f)))


MULTI_CASES = ((4,), (48, 256, 4))             # dml_h2_bound_bn_multi: the entries' N
