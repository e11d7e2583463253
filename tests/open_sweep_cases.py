"""Shared by tests/test_open_sweep_refs.py (CPU) and tests/test_gpu_open_sweep.py (GPU): the numpy definition of the open-set
threshold sweep (dml_open_set_sweep; include/dmlnet_hip.h), the brute-force route it must equal, and seeded inputs.

Definition (the header's text): l = label[p], l = unknown_id if l is one of out_labels; q = pred[p]; j = #{i : conf[p] >= t_i} in
float32 (NaN -> 0, +inf -> T, a tie keeps the prediction); cube[l][q][j] += 1 when both l and q are classes, else the pixel is
skipped; open_pred[p] = conf[p] >= t_w ? q : unknown_id for every pixel.
Brute force (anomaly/eval_ood_traditional.py:537-549 of the reference, once per threshold): pred_t = np.where(conf >= t, pred, u)
and a bincount of (label, pred_t) over the pixels whose label and prediction are classes.

Everything is integer: the GPU tests compare with exact equality.
"""
import functools

import numpy as np

import helpers as H

F32 = np.float32
SPAN, MAX_BLOCKS = 2048, 512          # dmlnet/_lib.py OPEN_SWEEP_SPAN / OPEN_SWEEP_MAX_BLOCKS (the tests assert they agree)


def thresholds_for(T):
    if T == 1:
        return np.array([0.5], F32)
    if T == 2:                                              # two adjacent float32 values
        return np.array([0.5, np.nextafter(F32(0.5), F32(1))], F32)
    if T == 3:
        return np.array([0.25, 0.5, 0.75], F32)
    if T == 9:                                              # the reference's sweep
        return np.array([0.1 * k for k in range(1, 10)], F32)
    return np.linspace(0.05, 0.95, T).astype(F32)


def remap(label, out_labels, u):
    lab = np.array(label, dtype=np.int64)
    lab[np.isin(label, np.asarray(out_labels, dtype=np.int64))] = u
    return lab


def cube_ref(conf, pred, label, thresholds, out_labels, nc, u):
    """the definition: int64 [nc, nc, T + 1]"""
    t = np.asarray(thresholds, F32)
    lab = remap(label, out_labels, u)
    with np.errstate(invalid="ignore"):
        j = (conf.astype(F32)[:, None] >= t[None, :]).sum(axis=1)
    ok = (lab >= 0) & (lab < nc) & (pred >= 0) & (pred < nc)
    cube = np.zeros((nc, nc, len(t) + 1), np.int64)
    np.add.at(cube, (lab[ok], pred[ok], j[ok]), 1)
    return cube


def matrix_from_cube(cube, i, u):
    """M_i[l][q] = sum_{j > i} cube[l][q][j] for q != u;  M_i[l][u] = sum_{j > i} cube[l][u][j] + sum_q sum_{j <= i} cube[l][q][j]"""
    m = cube[:, :, i + 1:].sum(axis=2)
    m[:, u] += cube[:, :, :i + 1].sum(axis=(1, 2))
    return m


def open_pred_ref(conf, pred, t, u):
    with np.errstate(invalid="ignore"):
        return np.where(conf.astype(F32) >= F32(t), pred, np.int64(u)).astype(np.int64)


def matrix_brute(conf, pred, label, t, out_labels, nc, u):
    """one threshold as the reference writes it, then np.bincount as metrics/stream_metrics.py does"""
    lab = remap(label, out_labels, u)
    ok = (lab >= 0) & (lab < nc) & (pred >= 0) & (pred < nc)           # decided on the prediction as it came in
    p_t = open_pred_ref(conf, pred, t, u)
    return np.bincount(nc * lab[ok] + p_t[ok], minlength=nc * nc).reshape(nc, nc).astype(np.int64)


def results_ref(m, u):
    """float64 scores of one matrix: the formulas of StreamSegMetrics.get_results, and the two classes of the reference's
    intersectionAndUnion(unknown_pred, seg_label_unknown, 2) written from the binary maps' areas"""
    m = m.astype(np.float64)
    tp, per_true, per_pred, total = np.diag(m), m.sum(axis=1), m.sum(axis=0), m.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp / (per_true + per_pred - tp)
        known = np.arange(m.shape[0]) != u
        inter_known = m[known][:, known].sum()
        return {"Overall Acc": tp.sum() / total, "Mean IoU": np.nanmean(iou), "Unknown IoU": iou[u],
                "Known IoU": inter_known / (m[known].sum() + m[:, known].sum() - inter_known)}


OOB_LABELS = (100, 101, 102, 103, 104, 105, 106)       # ids beyond any class count: they occur in the labels of "mixed" frames


def u_of(nc, where):
    return {"last": nc - 1, "first": 0, "middle": nc // 2}[where]


def out_for(n_out, u):
    """1: the driver's (unknown_id,); 3: unknown_id, one id that occurs, one that never does; 8: seven that occur and unknown_id"""
    return {0: (), 1: (u,), 3: (100, u, 77), 8: OOB_LABELS + (u,)}[n_out]


def _case(n, T, nc, where, n_out=1, conf="uniform", lab="mixed", pred="in"):
    return dict(n=n, T=T, nc=nc, u=u_of(nc, where), out=out_for(n_out, u_of(nc, where)), conf=conf, lab=lab, pred=pred)


CASES = {}
# pixel counts: below, at and above a wave; a workgroup's pass -1 / exact / +1 (exact is the most a single workgroup gets, +1 the
# first grid of two); the first count at which a workgroup makes a second pass; many workgroups with an odd tail
_combo = [(T, nc, w) for T in (1, 9, 12) for nc in (2, 14, 33) for w in ("last", "first", "middle")]
for k, n in enumerate((1, 2, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, SPAN * MAX_BLOCKS + 1, 300007)):
    T, nc, w = _combo[(7 * k + 3) % len(_combo)]
    CASES["n%d" % n] = _case(n, T, nc, w, n_out=(1, 3, 8)[k % 3], conf="edges" if k % 2 else "uniform")
# every T x n_classes x position of unknown_id, on three workgroups with an odd tail
for T, nc, w in _combo:
    CASES["T%d_k%d_%s" % (T, nc, w)] = _case(2 * SPAN + 37, T, nc, w, n_out=(1, 3, 8)[(T + nc) % 3], conf="edges")
CASES["const"] = _case(3 * SPAN + 5, 9, 14, "last", conf="const")                  # one cell takes every pixel
CASES["adjacent"] = _case(4099, 2, 14, "last", conf="edges")                       # thresholds one ulp apart
CASES["all_unknown"] = _case(4099, 9, 14, "last", lab="all_unknown")
CASES["no_unknown"] = _case(4099, 9, 14, "last", n_out=3, lab="no_unknown")
CASES["no_out_labels"] = _case(4099, 9, 14, "last", n_out=0)
CASES["pred_oob"] = _case(4099, 3, 14, "middle", n_out=8, conf="edges", pred="oob")
CASES["T3"] = _case(5003, 3, 14, "last", n_out=3, conf="edges")                     # every write_idx


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(conf float32 [n], pred int64 [n], label int64 [n], thresholds float32 [T]) of a case; read-only"""
    c = CASES[name]
    g = H.rng_for(41, "open_sweep." + name)
    n, nc, u = c["n"], c["nc"], c["u"]
    t = thresholds_for(c["T"])
    if c["conf"] == "uniform":
        conf = g.random(n, dtype=F32)
    elif c["conf"] == "const":
        conf = np.full(n, 0.55, F32)
    else:
        # each threshold, the float32 just below and just above it, NaN and both infinities, and uniform values in between
        pool = np.concatenate([t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf)),
                               np.array([np.nan, np.inf, -np.inf], F32), g.random(8, dtype=F32)]).astype(F32)
        conf = pool[g.integers(0, pool.size, n)]
    pred = g.integers(0, nc, n).astype(np.int64)                       # includes unknown_id
    if c["pred"] == "oob":
        bad = g.random(n) < 0.2
        pred[bad] = g.choice(np.array([-1, nc, 255, 2 ** 40, -2 ** 40], np.int64), int(bad.sum()))
    if c["lab"] == "all_unknown":
        label = np.full(n, c["out"][0], np.int64)
    elif c["lab"] == "no_unknown":
        known = np.array([k for k in range(nc) if k != u], np.int64)
        label = known[g.integers(0, known.size, n)]
    else:
        label = g.integers(0, nc, n).astype(np.int64)
        r = g.random(n)
        label[r < 0.10] = 255                                          # ignored
        label[(r >= 0.10) & (r < 0.15)] = -1
        occ = (r >= 0.15) & (r < 0.30)
        label[occ] = g.choice(np.array(OOB_LABELS, np.int64), int(occ.sum()))
    for a in (conf, pred, label, t):
        a.setflags(write=False)
    return conf, pred, label, t


@functools.lru_cache(maxsize=None)
def reference(name):
    """(cube [nc, nc, T + 1] int64, read-only) of a case"""
    c = CASES[name]
    conf, pred, label, t = inputs(name)
    cube = cube_ref(conf, pred, label, t, c["out"], c["nc"], c["u"])
    cube.setflags(write=False)
    return cube
