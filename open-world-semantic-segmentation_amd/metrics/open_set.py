"""The open-set prediction scored against a list of thresholds (anomaly/eval_ood_traditional.py:155-156,227-229,537-549,
599-607,645-653 of the reference: `pred[conf < thre] = 13`, nine `intersection_meter_unknown` / `union_meter_unknown`
meters for the thresholds 0.1 ... 0.9, the best threshold by IoU -- its scoring loop is commented out there).

`update` takes the label, prediction and confidence tensors where the model left them and adds one (label, prediction,
bin) histogram -- the cube -- to a device int64 tensor in one launch for all thresholds (dml_open_set_sweep); only the
cube comes to the host, in `get_results`.  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from dmlnet import _lib


def cube_to_matrix(cube, i, unknown_id):
    """The confusion matrix of threshold i (rows = label, columns = open-set prediction) from the cube [n, n, T + 1]:
    a pixel in bin j has passed j thresholds, so it keeps its prediction for j > i and is `unknown_id` otherwise."""
    cube = np.asarray(cube)
    m = cube[:, :, i + 1:].sum(axis=2)
    m[:, unknown_id] += cube[:, :, :i + 1].sum(axis=(1, 2))
    return m


class OpenSetSweepMetrics(object):
    def __init__(self, n_classes, thresholds, unknown_id, out_labels=()):
        """n_classes counts the unknown class (K + 1); labels in `out_labels` are remapped to `unknown_id`."""
        self.n_classes, self.unknown_id = int(n_classes), int(unknown_id)
        self.thresholds = tuple(float(np.float32(t)) for t in thresholds)
        self.out_labels = tuple(int(v) for v in out_labels)
        T = len(self.thresholds)
        if not 1 <= T <= _lib.OPEN_SWEEP_MAX_T:
            raise ValueError("between 1 and %d thresholds, not %d" % (_lib.OPEN_SWEEP_MAX_T, T))
        if not all(b > a for a, b in zip(self.thresholds, self.thresholds[1:])) or np.isnan(self.thresholds[0]):
            raise ValueError("thresholds must be strictly increasing (as float32): %r" % (self.thresholds,))
        if not 2 <= self.n_classes <= _lib.OPEN_SWEEP_MAX_CLASSES:
            raise ValueError("n_classes must be in 2 .. %d" % _lib.OPEN_SWEEP_MAX_CLASSES)
        if not 0 <= self.unknown_id < self.n_classes:
            raise ValueError("unknown_id must be one of the n_classes")
        if len(self.out_labels) > _lib.OPEN_SWEEP_MAX_OUT:
            raise ValueError("at most %d out_labels" % _lib.OPEN_SWEEP_MAX_OUT)
        self._t = (ctypes.c_float * T)(*self.thresholds)
        self._out = (ctypes.c_int64 * max(1, len(self.out_labels)))(*self.out_labels)
        self.cube = None                      # device int64 [n, n, T + 1], created on the first update

    def _shape(self):
        return (self.n_classes, self.n_classes, len(self.thresholds) + 1)

    def update(self, label_trues, label_preds, conf):
        lib = _lib.load()
        for t, dt in ((label_trues, torch.int64), (label_preds, torch.int64), (conf, torch.float32)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt):
                raise TypeError("OpenSetSweepMetrics.update takes int64, int64 and float32 CUDA tensors "
                                "(there is no CPU fallback)")
        if not label_trues.numel() == label_preds.numel() == conf.numel():
            raise ValueError("label_trues, label_preds and conf differ in size")
        # a contiguous view of an int64 / float32 tensor is aligned to its element, which is all the kernel asks for
        lt, lp, cf = label_trues.contiguous(), label_preds.contiguous(), conf.contiguous()
        if self.cube is None or self.cube.device != lt.device:
            self.cube = torch.zeros(self._shape(), dtype=torch.int64, device=lt.device)
        st = torch.cuda.current_stream(lt.device).cuda_stream
        _lib.check(lib.dml_open_set_sweep(cf.data_ptr(), lp.data_ptr(), lt.data_ptr(), lt.numel(), self._t,
                                          len(self.thresholds), self._out, len(self.out_labels), self.n_classes,
                                          self.unknown_id, self.cube.data_ptr(), None, 0, st), "dml_open_set_sweep")

    def all_reduce(self, group=None):
        """Sum the cube over the ranks of a data-parallel evaluation, as StreamSegMetrics.all_reduce does its matrix: a
        rank that saw no image still issues the collective.  No-op outside a process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        if self.cube is None:
            self.cube = torch.zeros(self._shape(), dtype=torch.int64,
                                    device=torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(self.cube, group=group)

    def _host_cube(self):
        return np.zeros(self._shape(), dtype=np.int64) if self.cube is None else self.cube.cpu().numpy()

    def confusion(self, i):
        """int64 [n_classes, n_classes] matrix of threshold i"""
        if not 0 <= i < len(self.thresholds):
            raise IndexError("threshold index %r" % (i,))
        return cube_to_matrix(self._host_cube(), i, self.unknown_id)

    def get_results(self):
        """One dict per threshold, in float64 with the formulas of StreamSegMetrics.get_results on M_i: "Threshold",
        "Overall Acc", "Mean IoU" over the K + 1 classes (classes that never occur are skipped), "Unknown IoU" (class
        unknown_id) and "Known IoU" (every other class taken as one: the two halves of the reference's
        intersectionAndUnion(unknown_pred, seg_label_unknown, 2)), and "Closed Mean IoU", the mean IoU of the
        predictions as they came in (the cube summed over its bins), the same for every threshold."""
        cube = self._host_cube()
        u = self.unknown_id
        with np.errstate(divide="ignore", invalid="ignore"):
            closed = cube.sum(axis=2).astype(np.float64)
            ctp = np.diag(closed)
            closed_miou = np.nanmean(ctp / (closed.sum(axis=1) + closed.sum(axis=0) - ctp))
            out = []
            for i, t in enumerate(self.thresholds):
                m = cube_to_matrix(cube, i, u).astype(np.float64)
                tp, per_true, per_pred, total = np.diag(m), m.sum(axis=1), m.sum(axis=0), m.sum()
                iou = tp / (per_true + per_pred - tp)
                known_tp = total - per_true[u] - per_pred[u] + tp[u]        # label and prediction both known
                out.append({"Threshold": t,
                            "Overall Acc": tp.sum() / total,
                            "Mean IoU": np.nanmean(iou),
                            "Unknown IoU": iou[u],
                            "Known IoU": known_tp / ((total - per_true[u]) + (total - per_pred[u]) - known_tp),
                            "Closed Mean IoU": closed_miou})
        return out

    @staticmethod
    def to_str(results):
        """one line per threshold"""
        lines = ["threshold %.4f: Unknown IoU %.4f, Known IoU %.4f, Mean IoU %.4f, Overall Acc %.4f"
                 % (r["Threshold"], r["Unknown IoU"], r["Known IoU"], r["Mean IoU"], r["Overall Acc"]) for r in results]
        return "\n" + "\n".join(lines) + "\n"

    def reset(self):
        if self.cube is not None:
            self.cube.zero_()
