"""The reference's pixel-level OOD measures (anomaly/anom_utils.py there) computed on the MI355X.

Same function names; the arguments are CUDA tensors where the reference takes numpy arrays, so that the
per-image score map (2 M pixels at 1024 x 2048) is sorted and ranked where the model left it instead of being
copied to the host and argsorted there (eval_ood_traditional.py:128-148, :566-569).  Three doubles come back.
No CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from dmlnet import _lib

recall_level_default = 0.95


def _measures(conf, seg_label, out_labels, mask, recall_level):
    lib = _lib.load()
    if not (isinstance(conf, torch.Tensor) and conf.is_cuda and conf.dtype == torch.float32):
        raise TypeError("scores must be a float32 CUDA tensor (there is no CPU fallback)")
    if not (seg_label.is_cuda and seg_label.dtype == torch.int64 and seg_label.numel() == conf.numel()):
        raise TypeError("labels must be an int64 CUDA tensor with one entry per score")
    conf, seg_label = conf.contiguous(), seg_label.contiguous()
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
        if mask.numel() != conf.numel() or not mask.is_cuda:
            raise TypeError("mask must be a CUDA tensor with one entry per score")
    n = conf.numel()
    work = torch.empty(lib.dml_ood_workspace_bytes(n), dtype=torch.uint8, device=conf.device)
    res = torch.empty(5, dtype=torch.float64, device=conf.device)
    ol = (C.c_int64 * len(out_labels))(*[int(v) for v in out_labels])
    st = torch.cuda.current_stream(conf.device).cuda_stream
    _lib.check(lib.dml_ood_measures(conf.data_ptr(), seg_label.data_ptr(), mask.data_ptr() if mask is not None else None, n,
                                    ol, len(out_labels), float(recall_level), work.data_ptr(), work.numel(), res.data_ptr(),
                                    st), "dml_ood_measures")
    r = res.cpu().numpy()
    if r[3] == 0 or r[4] == 0:
        return None
    return float(r[0]), float(r[1]), float(r[2])


def get_measures(_pos, _neg, recall_level=recall_level_default):
    """(auroc, aupr, fpr) with `_pos` the scores of the positive class (anom_utils.py:68-78)"""
    pos, neg = _pos.reshape(-1), _neg.reshape(-1)
    scores = torch.cat([pos, neg]).to(torch.float32)
    labels = torch.zeros(scores.numel(), dtype=torch.int64, device=scores.device)
    labels[: pos.numel()] = 1
    res = _measures(-scores, labels, [1], None, recall_level)       # the kernel negates conf
    if res is None:
        raise ValueError("both classes need at least one sample")
    return res


def print_measures(auroc, aupr, fpr, method_name="Ours", recall_level=recall_level_default):
    print("\t\t\t\t" + method_name)
    print("FPR{:d}:\t\t\t{:.2f}".format(int(100 * recall_level), 100 * fpr))
    print("AUROC: \t\t\t{:.2f}".format(100 * auroc))
    print("AUPR:  \t\t\t{:.2f}".format(100 * aupr))


def get_and_print_results(out_score, in_score, num_to_avg=1):
    """anom_utils.py:96-105: one evaluation, returned as means"""
    auroc, aupr, fpr = get_measures(out_score, in_score)
    return float(np.mean([auroc])), float(np.mean([aupr])), float(np.mean([fpr]))


def eval_ood_measure(conf, seg_label, out_labels, mask=None, recall_level=recall_level_default):
    """eval_ood_traditional.py:128-148: scores -conf, positives = pixels labelled with one of `out_labels`
    (cfg.OOD.out_labels there); None when the image has no OOD pixel or only OOD pixels."""
    res = _measures(conf, seg_label, out_labels, mask, recall_level)
    if res is None:
        print("This image does not contain any OOD pixels or is only OOD.")
    return res


class PooledOodMeasures(object):
    """AUROC / AUPR / FPR at a recall level over all pixels of a dataset at once, where `eval_ood_measure` scores one frame and
    the drivers average: frames weigh by their anomaly area, frames without an anomaly count as negatives, and one threshold
    serves the whole set.  `update` adds a frame's pixels to a histogram of the confidence over `bins` equal bins of [lo, hi],
    positives (labels in `out_labels`) and negatives apart, in one launch on the device (dml_pooled_ood_update); the measures
    are those of the binned scores, and `tie_mass` / `auroc_bounds` say how far binning can have moved the AUROC.  The state is
    2 * bins + 5 int64 counts: it can be merged, saved and resumed.  No CPU fallback."""

    def __init__(self, out_labels, lo=0.0, hi=1.0, bins=4096, recall_level=recall_level_default, device=None):
        self.out_labels = tuple(int(v) for v in out_labels)
        self.lo, self.hi = float(np.float32(lo)), float(np.float32(hi))
        self.bins, self.recall_level = int(bins), float(recall_level)
        if not 1 <= len(self.out_labels) <= _lib.POOLED_OOD_MAX_OUT:
            raise ValueError("between 1 and %d out_labels" % _lib.POOLED_OOD_MAX_OUT)
        if not 1 <= self.bins <= _lib.POOLED_OOD_MAX_BINS:
            raise ValueError("bins must be in 1 .. %d" % _lib.POOLED_OOD_MAX_BINS)
        with np.errstate(over="ignore"):
            width = np.float32(self.hi) - np.float32(self.lo)          # the kernel's float32 subtraction
        if not (np.isfinite(self.lo) and np.isfinite(self.hi) and self.hi > self.lo and np.isfinite(width)):
            raise ValueError("the range needs finite float32 bounds with lo < hi, not [%r, %r]" % (lo, hi))
        if np.isnan(self.recall_level):
            raise ValueError("recall_level is NaN")
        self._out = (C.c_int64 * len(self.out_labels))(*self.out_labels)
        self.device = torch.device(device) if device is not None else None
        self.state = None                     # device int64 [2 * bins + 5], created on the first update

    def _config(self):
        return (self.lo, self.hi, self.bins, self.out_labels)

    def _state_on(self, device):
        if self.state is None:
            self.state = torch.zeros(2 * self.bins + _lib.POOLED_OOD_COUNTERS, dtype=torch.int64, device=device)
            self.device = self.state.device
        return self.state

    def _default_device(self):
        return self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def update(self, conf, seg_label, mask=None):
        """one frame: float32 confidences, int64 labels and an optional mask (0 = skip), CUDA tensors as eval_ood_measure takes"""
        lib = _lib.load()
        if not (isinstance(conf, torch.Tensor) and conf.is_cuda and conf.dtype == torch.float32):
            raise TypeError("scores must be a float32 CUDA tensor (there is no CPU fallback)")
        if not (isinstance(seg_label, torch.Tensor) and seg_label.is_cuda and seg_label.dtype == torch.int64
                and seg_label.numel() == conf.numel()):
            raise TypeError("labels must be an int64 CUDA tensor with one entry per score")
        conf, seg_label = conf.contiguous(), seg_label.contiguous()
        if mask is not None:
            if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.numel() == conf.numel()):
                raise TypeError("mask must be a CUDA tensor with one entry per score")
            mask = mask.to(torch.uint8).contiguous()
        if self.state is not None and self.state.device != conf.device:
            raise ValueError("the state lives on %s, the frame on %s" % (self.state.device, conf.device))
        state = self._state_on(conf.device)
        st = torch.cuda.current_stream(conf.device).cuda_stream
        _lib.check(lib.dml_pooled_ood_update(conf.data_ptr(), seg_label.data_ptr(), mask.data_ptr() if mask is not None else None,
                                             conf.numel(), self._out, len(self.out_labels), self.lo, self.hi, self.bins,
                                             state.data_ptr(), st), "dml_pooled_ood_update")

    def merge(self, other):
        """add another accumulator's counts (disjoint frames: another rank, another shard)"""
        if not isinstance(other, PooledOodMeasures) or other._config() != self._config():
            raise ValueError("only accumulators with the same range, bins and out_labels can be merged")
        if other.state is not None:
            state = self._state_on(other.state.device if self.state is None else self.state.device)
            state += other.state.to(state.device)
        return self

    def all_reduce(self, group=None):
        """sum the state over the ranks of a data-parallel evaluation; a rank that saw no frame still issues the collective"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        dist.all_reduce(self._state_on(self._default_device()), group=group)

    def reset(self):
        if self.state is not None:
            self.state.zero_()

    def state_dict(self):
        host = np.zeros(2 * self.bins + _lib.POOLED_OOD_COUNTERS, np.int64) if self.state is None else self.state.cpu().numpy()
        return {"state": torch.from_numpy(host.copy()), "lo": self.lo, "hi": self.hi, "bins": self.bins,
                "out_labels": list(self.out_labels), "recall_level": self.recall_level}

    def load_state_dict(self, sd):
        got = (float(sd["lo"]), float(sd["hi"]), int(sd["bins"]), tuple(int(v) for v in sd["out_labels"]))
        if got != self._config():
            raise ValueError("the saved state has range, bins, out_labels %r, this accumulator %r" % (got, self._config()))
        state = torch.as_tensor(sd["state"], dtype=torch.int64).reshape(-1)
        if state.numel() != 2 * self.bins + _lib.POOLED_OOD_COUNTERS:
            raise ValueError("the saved state has %d entries, not %d" % (state.numel(), 2 * self.bins + _lib.POOLED_OOD_COUNTERS))
        self.state = state.to(self._default_device()).contiguous().clone()
        self.device = self.state.device

    def _finalize(self):
        """(float64 result[8], int64 counters[5]) on the host: one launch, one copy"""
        lib = _lib.load()
        state = self._state_on(self._default_device())
        res = torch.empty(8 + _lib.POOLED_OOD_COUNTERS, dtype=torch.float64, device=state.device)
        st = torch.cuda.current_stream(state.device).cuda_stream
        _lib.check(lib.dml_pooled_ood_finalize(state.data_ptr(), self.bins, self.recall_level, res.data_ptr(), st),
                   "dml_pooled_ood_finalize")
        res[8:] = state[2 * self.bins:]                   # counts below 2^53: exact in float64; they ride in the one copy
        r = res.cpu().numpy()
        return r[:8], r[8:].astype(np.int64)

    def get_results(self):
        """dict of the pooled measures, or None when no positive or no negative pixel was seen (as eval_ood_measure)"""
        r, cnt = self._finalize()
        if r[3] == 0 or r[4] == 0:
            return None
        auroc, tie = float(r[0]), float(r[5])
        return {"auroc": auroc, "aupr": float(r[1]), "fpr": float(r[2]), "positives": int(r[3]), "negatives": int(r[4]),
                "tie_mass": tie, "auroc_bounds": (auroc - 0.5 * tie, auroc + 0.5 * tie), "cut_bin": int(r[6]),
                "threshold": self._edge(int(r[6])), "n_nan": int(cnt[0]), "n_below": int(cnt[1]), "n_above": int(cnt[2]),
                "n_masked": int(cnt[3]), "frames": int(cnt[4])}

    def counters(self):
        """dict of the five counters beside the histogram, from the host copy of the state: n_nan, n_below, n_above, n_masked, frames
        (what get_results() cannot say when it returns None: a confidence that is NaN everywhere counts no pixel)"""
        cnt = [0] * _lib.POOLED_OOD_COUNTERS if self.state is None else self.state[2 * self.bins:].cpu().tolist()
        return dict(zip(("n_nan", "n_below", "n_above", "n_masked", "frames"), cnt))

    def _edge(self, cut):
        return self.lo + (cut + 1) * (self.hi - self.lo) / self.bins

    def threshold_at_recall(self):
        """float64 upper edge of the cut-off bin: every pixel with conf below it is flagged at the recall level (what
        --open_set_thresholds takes); None without a positive or a negative pixel"""
        r, _ = self._finalize()
        if r[3] == 0 or r[4] == 0:
            return None
        return self._edge(int(r[6]))

    def curve(self):
        """(tp, fp, edges) on the host: int64 [bins] positives / negatives flagged at each bin's upper edge (bin <= b), and the
        float64 [bins + 1] bin edges"""
        state = self._state_on(self._default_device())
        cum = torch.cumsum(state[:2 * self.bins].view(2, self.bins), dim=1).cpu().numpy()
        edges = self.lo + np.arange(self.bins + 1, dtype=np.float64) * (self.hi - self.lo) / self.bins
        return cum[0], cum[1], edges
