"""Open-world scores computed on the device instead of on 134 MB/img host copies
(test_embedding.py:339-350,365,385-386,428-445; anomaly/eval_ood_traditional.py:301-305,434-448,492-510,511-530,537-549)."""
from __future__ import annotations

import numpy as np
import torch

from dmlnet import _lib


def _st(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("open-world scores run on the HIP path only (no CPU fallback)")


def argmax_msp(logits: torch.Tensor):
    """preds = argmax_k logits, scores = 1 - max softmax."""
    _need_cuda(logits)
    lib = _lib.load()
    logits = logits.contiguous().float()
    B, K, H, W = logits.shape
    preds = torch.empty((B, H, W), dtype=torch.int64, device=logits.device)
    msp = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
    _lib.check(lib.dml_argmax_msp(logits.data_ptr(), preds.data_ptr(), msp.data_ptr(), B, K, H, W, _st(logits)),
               "dml_argmax_msp")
    return preds, msp


def dissum_score(logits: torch.Tensor, clip: float = 1000.0, inclusive: bool = False) -> torch.Tensor:
    """-sum_k logit_k, clipped (`> clip` for the DeepLab driver, `>= clip` with clip=400 for anomaly/),
    min-max normalised per image."""
    _need_cuda(logits)
    lib = _lib.load()
    logits = logits.contiguous().float()
    B, K, H, W = logits.shape
    score = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
    work = torch.empty(2 * B, dtype=torch.float32, device=logits.device)
    _lib.check(lib.dml_dissum_score(logits.data_ptr(), score.data_ptr(), work.data_ptr(), B, K, H, W, float(clip),
                                    1 if inclusive else 0, _st(logits)), "dml_dissum_score")
    return score


def dissum_msp_score(logits: torch.Tensor, clip: float = 400.0, threshold: float = 0.2, slope: float = 50.0,
                     prob: str = "softmax", first_class: int = 0) -> torch.Tensor:
    """The paper's "EDS + MMSP" anomaly score of logits [B, K, H, W] over the classes first_class .. K - 1 -> [B, H, W]
    (dml_dissum_msp_score): with d the clipped distance sum -sum_k logit_k and q the maximum softmax probability, each
    min-max normalised per image, conf = c d + (1 - c) q under the gate c = 1 / (1 + exp(slope (d - threshold))) --
    anomaly/eval_ood_traditional.py:302-305, :434-435 and :447-448 of the reference (the defaults are its clip 400,
    Coefficient_map(dis_sum, 0.2) and lamda = 50).  first_class=1 is --exclude_back without a copy of the logits.
    prob="logit" takes the maximum logit in place of the maximum softmax: the DeepLab driver's recipe
    (test_embedding.py:366-369) is dissum_msp_score(outputs, clip=1000.0, threshold=0.3, prob="logit").  An image whose
    d or q map is constant comes back NaN, as numpy evaluates the reference's statements."""
    _need_cuda(logits)
    if logits.dim() != 4:
        raise ValueError("logits must be [B, K, H, W]")
    if prob not in ("softmax", "logit"):
        raise ValueError("prob must be 'softmax' or 'logit', not %r" % (prob,))
    lib = _lib.load()
    logits = logits.contiguous().float()
    B, K, H, W = logits.shape
    conf = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
    work = torch.empty(4 * B + 2 * B * H * W, dtype=torch.float32, device=logits.device)
    _lib.check(lib.dml_dissum_msp_score(logits.data_ptr(), conf.data_ptr(), work.data_ptr(), B, K, H, W, int(first_class),
                                        float(clip), float(threshold), float(slope), 1 if prob == "logit" else 0,
                                        _st(logits)), "dml_dissum_msp_score")
    return conf


def knn_cosine_score(feats: torch.Tensor, neighbor_size: int = 9) -> torch.Tensor:
    """The kNN anomaly score of anomaly/eval_ood_traditional.py:511-530 on feats [B, C, H, W] (the second return value of
    models.evaluate_multiscale): per pixel the sum of the cosine similarities with the (neighbor_size - 1)^2 pixels
    down-right and the (neighbor_size - 1)^2 pixels up-left of it, 0 for a neighbour outside the image
    (dml_knn_cosine_score) -> [B, H, W]."""
    _need_cuda(feats)
    if feats.dim() != 4:
        raise ValueError("feats must be [B, C, H, W]")
    lib = _lib.load()
    feats = feats.contiguous().float()
    B, C, H, W = feats.shape
    score = torch.empty((B, H, W), dtype=torch.float32, device=feats.device)
    _lib.check(lib.dml_knn_cosine_score(feats.data_ptr(), score.data_ptr(), B, C, H, W, int(neighbor_size), _st(feats)),
               "dml_knn_cosine_score")
    return score


# dense_crf_gauss's workspace, one per device: {device index: ((B, C, H, W), uint8 tensor)}.  A frame of another shape replaces
# it, so a driver that walks a dataset holds one workspace, not one per size.
_CRF_WORK = {}


def dense_crf_gauss(scores: torch.Tensor, sxy=3.0, compat: float = 3.0, iters: int = 100, first_class: int = 0,
                    clip: float = 1e-5, return_map: bool = False):
    """Dense-CRF confidence of scores [B, K, H, W] (fp32, CUDA) over the classes first_class .. K - 1 -> conf [B, H, W]
    (dml_crf_gauss): the unary -log(clipped softmax) of pydensecrf's unary_from_softmax, one spatial Gaussian pairwise term
    (sxy, a float or an (sx, sy) pair as addPairwiseGaussian takes it; Potts compat), `iters` mean-field steps and the
    maximum over the classes -- anomaly/eval_ood_traditional.py:492-510 of the reference with its defaults sxy = 3,
    compat = 3, inference(100).  The Gaussian filter is computed exactly, as two 1-D passes per step, where pydensecrf's
    lattice approximates it; y is the row and x the column (the reference swaps them in DenseCRF2D(h, w, ch)), and
    first_class=1 is --exclude_back without a copy (the reference stops there).  return_map=True also returns the int64
    arg-max map [B, H, W], counted from first_class.  The workspace is kept per device and shape; calls that share it
    must be ordered on one stream."""
    _need_cuda(scores)
    if scores.dim() != 4:
        raise ValueError("scores must be [B, K, H, W]")
    if scores.dtype != torch.float32:
        raise TypeError("scores must be float32, not %s" % (scores.dtype,))
    sx, sy = (sxy if isinstance(sxy, (tuple, list)) else (sxy, sxy))
    lib = _lib.load()
    scores = scores.contiguous()
    B, K, H, W = scores.shape
    C = K - int(first_class)
    nbytes = lib.dml_crf_gauss_workspace_bytes(B, C, H, W)
    _lib.check(min(nbytes, 0), "dml_crf_gauss_workspace_bytes")
    key = (B, C, H, W)
    held = _CRF_WORK.get(scores.device.index)
    if held is None or held[0] != key:
        _CRF_WORK.pop(scores.device.index, None)
        held = (key, torch.empty(nbytes, dtype=torch.uint8, device=scores.device))
        _CRF_WORK[scores.device.index] = held
    conf = torch.empty((B, H, W), dtype=torch.float32, device=scores.device)
    lab = torch.empty((B, H, W), dtype=torch.int64, device=scores.device) if return_map else None
    _lib.check(lib.dml_crf_gauss(scores.data_ptr(), conf.data_ptr(), lab.data_ptr() if return_map else None,
                                 held[1].data_ptr(), B, K, H, W, int(first_class), float(sx), float(sy), float(compat),
                                 int(iters), float(clip), _st(scores)), "dml_crf_gauss")
    return (conf, lab) if return_map else conf


def open_set_predict(conf: torch.Tensor, preds: torch.Tensor, threshold: float, unknown_id: int) -> torch.Tensor:
    """The open-set prediction of anomaly/eval_ood_traditional.py:537-549 of the reference (`pred[conf < thre] = 13`;
    test_embedding.py:385-386 is the same with the sign of its score turned): preds (int64, CUDA) where conf (float32, CUDA,
    as many elements) >= threshold, `unknown_id` elsewhere -- a NaN confidence is unknown -> int64, shaped like preds.
    One launch of dml_open_set_sweep with a single threshold and no histogram (unknown_id in 0 .. 32, the library's class
    range); metrics.OpenSetSweepMetrics scores the same prediction for a list of thresholds without materialising it."""
    import ctypes
    _need_cuda(conf)
    _need_cuda(preds)
    if conf.dtype != torch.float32 or preds.dtype != torch.int64:
        raise TypeError("conf must be float32 and preds int64, not %s / %s" % (conf.dtype, preds.dtype))
    if conf.numel() != preds.numel():
        raise ValueError("conf and preds differ in size")
    lib = _lib.load()
    conf, preds = conf.contiguous(), preds.contiguous()
    out = torch.empty_like(preds)
    t = (ctypes.c_float * 1)(float(threshold))
    _lib.check(lib.dml_open_set_sweep(conf.data_ptr(), preds.data_ptr(), None, preds.numel(), t, 1, None, 0,
                                      max(2, int(unknown_id) + 1), int(unknown_id), None, out.data_ptr(), 0, _st(conf)),
               "dml_open_set_sweep")
    return out


ECDF_MODES = {"hard": 0, "sigmoid": 1, "ecdf": 2}


def _need_cuda_tensor(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA tensor: the ECDF score runs on the HIP path only (no CPU fallback)" % what)


def ecdf_certainty_score(logits: torch.Tensor, table: torch.Tensor, clip: float, first_class: int = 0) -> torch.Tensor:
    """conf [B, H, W] = sum_k softmax_k * table[bin(s)][k - first_class] over the classes first_class .. K - 1 of logits
    [B, K, H, W] (fp32, CUDA), with s = -sum_k logit_k and bin() the NB equal bins of [0, clip] (dml_ecdf_score; the header has the
    bitwise definition).  table [NB, Kp] fp32 is what EcdfCalibrator.table returns: the certainty of every (bin, class), Kp the
    class count rounded up to a multiple of 4.  One launch, one read of the logits; a pixel whose s is NaN comes back NaN."""
    _need_cuda_tensor(logits, "logits")
    _need_cuda_tensor(table, "table")
    if logits.dim() != 4 or table.dim() != 2:
        raise ValueError("logits must be [B, K, H, W] and table [NB, Kp]")
    if logits.dtype != torch.float32 or table.dtype != torch.float32:
        raise TypeError("logits and table must be float32")
    lib = _lib.load()
    logits, table = logits.contiguous(), table.contiguous()
    B, K, H, W = logits.shape
    conf = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
    _lib.check(lib.dml_ecdf_score(logits.data_ptr(), table.data_ptr(), conf.data_ptr(), B, K, H, W, int(first_class),
                                  table.shape[1], float(clip), table.shape[0], _st(logits)), "dml_ecdf_score")
    return conf


def _em_two_gaussians(x, c, floor, tol=1e-9, max_steps=500):
    """EM of a two-component 1-D Gaussian mixture on the points x with the weights c (float64, at least two c > 0), the variances
    kept at or above `floor`.  Deterministic: the components start as the two halves of the sample split at its weighted median.
    Stops when the log-likelihood gains less than tol * |log-likelihood| or after max_steps.
    -> (pi [2], mu [2], var [2], trace: the log-likelihood before every M-step and of the returned parameters last)"""
    N = c.sum()
    cum = np.cumsum(c)
    med = int(np.searchsorted(cum, 0.5 * N))
    low = np.arange(x.size) <= med
    if not c[~low].sum() > 0:                  # the median bin is the last occupied one: it goes to the upper half
        low = np.arange(x.size) < med
    pi, mu, var = np.empty(2), np.empty(2), np.empty(2)
    for j, half in enumerate((low, ~low)):
        wj = c[half].sum()
        pi[j] = wj / N
        mu[j] = (c[half] * x[half]).sum() / wj
        var[j] = max((c[half] * (x[half] - mu[j]) ** 2).sum() / wj, floor)
    trace, prev = [], None
    for _ in range(max_steps):
        with np.errstate(divide="ignore"):
            logp = np.log(pi)[:, None] - 0.5 * np.log(2.0 * np.pi * var)[:, None] - (x[None] - mu[:, None]) ** 2 / (2.0 * var[:, None])
        top = logp.max(axis=0)
        lse = top + np.log(np.exp(logp - top).sum(axis=0))
        ll = float((c * lse).sum())
        trace.append(ll)
        if prev is not None and ll - prev < tol * abs(prev):
            break
        prev = ll
        r = np.exp(logp - lse) * c                                          # responsibilities times the counts
        nj = r.sum(axis=1)
        for j in range(2):
            if nj[j] > 0.0:                                                 # a component that died keeps its place
                mu[j] = (r[j] * x).sum() / nj[j]
                var[j] = max((r[j] * (x - mu[j]) ** 2).sum() / nj[j], floor)
        pi = nj / N
    return pi, mu, var, trace


def fit_gmm_thresholds(hist, clip: float) -> np.ndarray:
    """The per-class threshold of the reference's commented recipe (main_embedding.py:209-219: GaussianMixture(n_components=2),
    thre = mean - sqrt(variance) of the component with the smaller variance) from the histogram [Kn, NB] of EcdfCalibrator:
    EM on the bin centres (b + 1/2) w, w = clip / NB, weighted by the counts -- a fit of a few kilobytes on the host, once per
    calibration.  Deterministic where sklearn's k-means initialisation is not: see _em_two_gaussians; the variance floor is
    w^2 / 12 (a bin's own spread) + 1e-6 (sklearn's reg_covar).  A class with fewer than two occupied bins gets its smallest
    occupied bin centre, an empty class 0 -> float64 [Kn]."""
    hist = np.asarray(hist, dtype=np.float64)
    Kn, NB = hist.shape
    w = float(clip) / NB
    x = (np.arange(NB) + 0.5) * w
    out = np.zeros(Kn)
    for cl in range(Kn):
        occ = np.flatnonzero(hist[cl] > 0)
        if occ.size < 2:
            out[cl] = x[occ[0]] if occ.size else 0.0
            continue
        _, mu, var, _ = _em_two_gaussians(x, hist[cl], w * w / 12.0 + 1e-6)
        j = int(np.argmin(var))
        out[cl] = mu[j] - np.sqrt(var[j])
    return out


class EcdfCalibrator:
    """The calibrated certainty score the reference keeps commented (main_embedding.py:106-113,172-226,249-260;
    test_embedding.py:155-163,361-364): per class, the empirical CDF of the distance sums s = -sum_k logit_k of the calibration
    pixels that are labelled and predicted that class, then conf = sum_cl softmax_cl * Certainty(E_cl(s)).  Unlike the per-frame
    min-max scores its value means the same on every frame.

        cal = EcdfCalibrator(num_classes, clip=400.0)
        for logits, labels in calibration_frames:          # CUDA tensors; every pixel counts, nothing is copied to the host
            cal.update(logits, labels)
        conf = cal.score(logits)                           # mode="hard": E if E <= cut else 1;  "sigmoid": around the GMM threshold
        cal.save(path); cal = EcdfCalibrator.load(path)    # calibrate once, reuse

    The ECDF is a histogram over `nbins` equal bins of [0, clip] (int64 [Kn, nbins] on the device, Kn = num_classes -
    first_class, Kn * nbins <= 32768), exact and independent of the order of the frames.  first_class=1 is --exclude_back."""

    def __init__(self, num_classes: int, clip: float, nbins: int = 1024, first_class: int = 0):
        self.num_classes, self.clip, self.nbins, self.first_class = int(num_classes), float(clip), int(nbins), int(first_class)
        kn = self.num_classes - self.first_class
        if self.first_class < 0 or not 1 <= kn <= _lib.ECDF_MAX_CLASSES:
            raise ValueError("between 1 and %d classes from first_class on, not %d" % (_lib.ECDF_MAX_CLASSES, kn))
        if not 1 <= self.nbins <= _lib.ECDF_MAX_BINS or kn * self.nbins > _lib.ECDF_MAX_CELLS:
            raise ValueError("nbins must be in 1 .. %d with classes x nbins <= %d" % (_lib.ECDF_MAX_BINS, _lib.ECDF_MAX_CELLS))
        if not (self.clip > 0.0 and np.isfinite(self.clip)):
            raise ValueError("clip must be positive and finite")
        self.n_known = kn
        self.hist = torch.zeros((kn, self.nbins), dtype=torch.int64)
        self._invalidate()

    def _invalidate(self):
        """what is derived from the histogram: the table last built and the fitted thresholds"""
        self._tables = {}
        self._fitted = None

    def _device(self, device=None):
        if device is None:
            device = self.hist.device if self.hist.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:              # "cuda" is the current device, not another one than cuda:0
            device = torch.device("cuda", torch.cuda.current_device())
        if self.hist.device != device:
            self.hist = self.hist.to(device)
            self._invalidate()
        return device

    def update(self, logits: torch.Tensor, labels: torch.Tensor):
        """count the pixels of logits [B, K, H, W] (fp32) whose labels [B, H, W] (int64) equal their prediction (dml_ecdf_collect)"""
        _need_cuda_tensor(logits, "logits")
        _need_cuda_tensor(labels, "labels")
        if logits.dtype != torch.float32 or labels.dtype != torch.int64:
            raise TypeError("logits must be float32 and labels int64, not %s / %s" % (logits.dtype, labels.dtype))
        if logits.dim() != 4 or logits.shape[1] != self.num_classes:
            raise ValueError("logits must be [B, %d, H, W]" % self.num_classes)
        B, K, H, W = logits.shape
        if labels.numel() != B * H * W:
            raise ValueError("labels must be [B, H, W]")
        lib = _lib.load()
        self._device(logits.device)
        self._invalidate()
        logits, labels = logits.contiguous(), labels.contiguous()
        _lib.check(lib.dml_ecdf_collect(logits.data_ptr(), labels.data_ptr(), self.hist.data_ptr(), B, K, H, W, self.first_class,
                                        self.clip, self.nbins, _st(logits)), "dml_ecdf_collect")

    def counts(self) -> np.ndarray:
        """the per-class sample sizes, int64 [Kn]"""
        return self.hist.sum(dim=1).cpu().numpy()

    def fit_thresholds(self) -> np.ndarray:
        """fit_gmm_thresholds on the histogram: float64 [Kn], the `thresholds` of the sigmoid mode.  Fitted once per calibration:
        the result is kept until the next update (one copy of the histogram to the host, which waits for the stream)"""
        if self._fitted is None:
            self._fitted = fit_gmm_thresholds(self.hist.cpu().numpy(), self.clip)
        return self._fitted.copy()

    def table(self, mode: str = "hard", cut: float = 0.15, slope: float = 50.0, thresholds=None, device=None) -> torch.Tensor:
        """The certainty of every (bin, class) as a device tensor [nbins, Kp] fp32, Kp = Kn rounded up to a multiple of 4
        (dml_ecdf_table).  mode "hard": E if E <= cut else 1 (main_embedding.py:107-109); "sigmoid": 1 / (1 + exp(-slope (E -
        E(threshold_cl)))) (test_embedding.py:156-161), thresholds [Kn] or None for fit_thresholds(); "ecdf": E itself.  Kept
        until the next update."""
        if mode not in ECDF_MODES:
            raise ValueError("mode must be one of %s, not %r" % (sorted(ECDF_MODES), mode))
        device = self._device(device)
        if mode == "sigmoid" and thresholds is None:
            thresholds = self.fit_thresholds()
        thr = None
        if mode == "sigmoid":
            thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
            if thr.size != self.n_known:
                raise ValueError("one threshold per class: %d, not %d" % (self.n_known, thr.size))
        key = (mode, float(cut), float(slope), None if thr is None else thr.tobytes())
        if key not in self._tables:
            lib = _lib.load()
            kp = (self.n_known + 3) // 4 * 4
            tab = torch.empty((self.nbins, kp), dtype=torch.float32, device=device)
            tdev = None if thr is None else torch.from_numpy(thr).to(device)
            _lib.check(lib.dml_ecdf_table(self.hist.data_ptr(), tab.data_ptr(), None if tdev is None else tdev.data_ptr(),
                                          self.n_known, kp, self.nbins, self.clip, ECDF_MODES[mode], float(cut), float(slope),
                                          torch.cuda.current_stream(device).cuda_stream), "dml_ecdf_table")
            self._tables = {key: tab}
        return self._tables[key]

    def score(self, logits: torch.Tensor, mode: str = "hard", cut: float = 0.15, slope: float = 50.0, thresholds=None) -> torch.Tensor:
        """conf [B, H, W] of logits [B, K, H, W]: ecdf_certainty_score with this calibration's table"""
        _need_cuda_tensor(logits, "logits")
        if logits.dim() != 4 or logits.shape[1] != self.num_classes:
            raise ValueError("logits must be [B, %d, H, W]" % self.num_classes)
        tab = self.table(mode, cut, slope, thresholds, device=logits.device)
        return ecdf_certainty_score(logits, tab, self.clip, self.first_class)

    def state_dict(self):
        return {"hist": self.hist.detach().cpu().clone(), "num_classes": self.num_classes, "clip": self.clip, "nbins": self.nbins,
                "first_class": self.first_class}

    def load_state_dict(self, state):
        hist = torch.as_tensor(state["hist"]).to(torch.int64)
        want = (int(state["num_classes"]), float(state["clip"]), int(state["nbins"]), int(state["first_class"]))
        if want != (self.num_classes, self.clip, self.nbins, self.first_class) or tuple(hist.shape) != (self.n_known, self.nbins):
            raise ValueError("the state is of another calibration: %r" % (want,))
        self.hist = hist.clone().to(self.hist.device)
        self._invalidate()

    def save(self, path):
        """the int64 histogram and the constructor's arguments as one .npz (written to `path` as it is given)"""
        with open(path, "wb") as f:
            np.savez(f, hist=self.hist.cpu().numpy(), num_classes=np.int64(self.num_classes), clip=np.float64(self.clip),
                     nbins=np.int64(self.nbins), first_class=np.int64(self.first_class))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cal = cls(int(z["num_classes"]), float(z["clip"]), int(z["nbins"]), int(z["first_class"]))
            cal.load_state_dict({"hist": z["hist"], "num_classes": cal.num_classes, "clip": cal.clip, "nbins": cal.nbins,
                                 "first_class": cal.first_class})
        return cal


def _nhwc_pitch(t):
    """the pixel pitch, in elements, of a [B, h, w, C] tensor that is dense but for that pitch (a channel slice of a wider
    buffer), or None for any other layout; dimensions of size 1 do not count"""
    B, h, w, C = t.shape
    if C > 1 and t.stride(3) != 1:
        return None
    ld = None
    for size, dim, pixels in ((w, 2, 1), (h, 1, w), (B, 0, h * w)):
        if size > 1:
            if ld is None:
                if t.stride(dim) % pixels:
                    return None
                ld = t.stride(dim) // pixels
            elif t.stride(dim) != pixels * ld:
                return None
    ld = C if ld is None else ld
    return ld if ld >= C else None


def rec_cosine_score(feats1, feats2, out_hw) -> torch.Tensor:
    """The cosine map of anomaly/eval_ood_rec.py:96-125,143-146 of the reference (dml_rec_cosine): feats1[s] / feats2[s]
    are the pyramid concats of the s-th resized copy of a frame and of its reconstruction, [B, h_s, w_s, C] channels last,
    fp32 or bf16 (a channel slice of a wider buffer is taken as it is).  Each list is resized bilinearly to out_hw
    (F.interpolate, align_corners=False) and averaged, the two means are normalised over the channels and compared by
    F.cosine_similarity -> [B, Hq, Wq] fp32; a pixel where either mean is all zero gives 0.  One launch; nothing of the
    size C x Hq x Wq is allocated."""
    import ctypes
    feats1, feats2 = list(feats1), list(feats2)
    n = len(feats1)
    if n == 0 or len(feats2) != n:
        raise ValueError("feats1 and feats2 must be two lists of the same, non-zero length")
    if n > _lib.REC_MAX_SCALES:
        raise ValueError("at most %d scales" % _lib.REC_MAX_SCALES)
    for t in feats1 + feats2:
        _need_cuda(t)
    dtype, dev = feats1[0].dtype, feats1[0].device
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("the concats must be float32 or bfloat16, not %s" % (dtype,))
    B, C = feats1[0].shape[0], feats1[0].shape[-1]
    keep, geo = [], []
    for a, b in zip(feats1, feats2):
        if a.dim() != 4 or a.shape != b.shape or a.shape[0] != B or a.shape[-1] != C:
            raise ValueError("every scale needs two [B, h, w, C] tensors of one shape: %s / %s" % (tuple(a.shape), tuple(b.shape)))
        if a.dtype != dtype or b.dtype != dtype or a.device != dev or b.device != dev:
            raise ValueError("the concats must share one dtype and one device")
        _, h, w, _ = a.shape
        ld = _nhwc_pitch(a)
        pair = [a, b]
        if ld is None or _nhwc_pitch(b) != ld:         # one pitch for both inputs of a scale
            pair, ld = [a.contiguous(), b.contiguous()], C
        keep.extend(pair)
        geo.append((h, w, ld))
    lib = _lib.load()
    Hq, Wq = int(out_hw[0]), int(out_hw[1])
    cos = torch.empty((B, Hq, Wq), dtype=torch.float32, device=dev)
    p1 = (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep[0::2]])
    p2 = (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep[1::2]])
    hs, ws, lds = ((ctypes.c_int * n)(*[g[i] for g in geo]) for i in range(3))
    _lib.check(lib.dml_rec_cosine(p1, p2, hs, ws, lds, n, B, C, _lib.DML_BF16 if dtype == torch.bfloat16 else _lib.DML_F32,
                                  cos.data_ptr(), Hq, Wq, _st(cos)), "dml_rec_cosine")
    return cos


def rec_confidence(scores: torch.Tensor, cos: torch.Tensor, threshold: float = 0.999, prob: str = "logit",
                   first_class: int = 0) -> torch.Tensor:
    """The confidence of anomaly/eval_ood_rec.py:127-150 of the reference (dml_rec_confidence): scores [B, K, H, W] fp32,
    cos [B, Hq, Wq] (rec_cosine_score) -> conf [B, H, W] = msp where msp > threshold, else cos resized bilinearly to
    (H, W).  msp is the maximum over the classes first_class .. K - 1 (first_class=1 is --exclude_back without a copy) of
    the scores themselves for prob="logit" or of their softmax for prob="softmax".  "logit" is the reference's literal
    statement: its scores are negative squared distances, never above 0, so with the reference's threshold of 0.999 the
    gate never opens and conf is the resized cosine map alone; "softmax" is what the name msp and the 0.999 intend."""
    _need_cuda(scores)
    _need_cuda(cos)
    if scores.dim() != 4 or cos.dim() != 3 or cos.shape[0] != scores.shape[0]:
        raise ValueError("scores must be [B, K, H, W] and cos [B, Hq, Wq]")
    if prob not in ("softmax", "logit"):
        raise ValueError("prob must be 'softmax' or 'logit', not %r" % (prob,))
    if scores.dtype != torch.float32 or cos.dtype != torch.float32:
        raise TypeError("scores and cos must be float32")
    lib = _lib.load()
    scores, cos = scores.contiguous(), cos.contiguous()
    B, K, H, W = scores.shape
    conf = torch.empty((B, H, W), dtype=torch.float32, device=scores.device)
    _lib.check(lib.dml_rec_confidence(scores.data_ptr(), cos.data_ptr(), conf.data_ptr(), B, K, H, W, cos.shape[1], cos.shape[2],
                                      int(first_class), float(threshold), 1 if prob == "logit" else 0, _st(scores)),
               "dml_rec_confidence")
    return conf


def mean_prototype(shots) -> np.ndarray:
    """test_embedding.py:254-257."""
    return np.mean(np.asarray(shots, dtype=np.float64), axis=0)


def novel_relabel(preds: torch.Tensor, logits: torch.Tensor, feats: torch.Tensor, proto, thresh=-1.5,
                  new_label=16) -> torch.Tensor:
    """In place: preds[p] = new_label where -|f_p - proto|^2 > thresh and > max_k logit_k."""
    _need_cuda(logits)
    lib = _lib.load()
    logits, feats = logits.contiguous().float(), feats.contiguous().float()
    B, K, H, W = logits.shape
    C = feats.shape[-1]
    pr = torch.as_tensor(np.asarray(proto), dtype=torch.float32, device=logits.device).contiguous()
    assert preds.is_contiguous() and preds.dtype == torch.int64
    _lib.check(lib.dml_novel_relabel(feats.data_ptr(), logits.data_ptr(), pr.data_ptr(), preds.data_ptr(), B, C, K,
                                     H, W, float(thresh), int(new_label), _st(logits)), "dml_novel_relabel")
    return preds


def extract_prototype(features: torch.Tensor, labels_true: torch.Tensor, class_id: int, min_fraction: float = 0.05):
    """One shot of a novel-class prototype: the mean of `features_out` over the pixels labelled `class_id`, or None
    when the class covers less than `min_fraction` of the image -- the recipe the reference keeps commented out at
    test_embedding.py:413-425 (`features.cpu().numpy()[labels_true == 15]`, `np.mean(..., axis=0)`, json).  The
    reduction runs on the device; collect the returned lists and `json.dump` them as the reference does."""
    _need_cuda(features)
    lib = _lib.load()
    f = features.contiguous().float()
    C = f.shape[-1]
    f = f.view(-1, C)
    lab = labels_true.contiguous().view(-1)
    if lab.dtype != torch.int64 or lab.numel() != f.shape[0] or not lab.is_cuda:
        raise ValueError("labels_true must be an int64 CUDA tensor with one entry per pixel of `features`")
    sums = torch.empty(C, dtype=torch.float64, device=f.device)
    cnt = torch.empty(1, dtype=torch.int64, device=f.device)
    _lib.check(lib.dml_class_feature_sum(f.data_ptr(), lab.data_ptr(), f.shape[0], C, int(class_id), sums.data_ptr(),
                                         cnt.data_ptr(), _st(f)), "dml_class_feature_sum")
    n = int(cnt.item())
    if n == 0 or n / f.shape[0] <= min_fraction:
        return None
    return (sums / n).float().cpu().tolist()


def _protos_labels(protos, new_labels, device):
    """[N, C] float32 prototypes and [N] int64 labels on the device; (None, None, 0) for no prototype"""
    if protos is None:
        if new_labels is not None and len(new_labels):
            raise ValueError("new_labels without protos")
        return None, None, 0
    if isinstance(protos, torch.Tensor):
        pr = protos.to(device=device, dtype=torch.float32)
    else:
        pr = torch.as_tensor(np.asarray(protos, dtype=np.float32), device=device)
    if pr.dim() != 2:
        raise ValueError("protos must be [N, C]")
    N = pr.shape[0]
    lab = torch.as_tensor(np.asarray(new_labels if new_labels is not None else [], dtype=np.int64).reshape(-1), device=device)
    if lab.numel() != N:
        raise ValueError("one new label per prototype: %d prototypes, %d labels" % (N, lab.numel()))
    if N == 0:
        return None, None, 0
    return pr.contiguous(), lab, N


def open_world_post(logits: torch.Tensor, feats: torch.Tensor, protos=None, new_labels=None, thresh=-1.5,
                    vs_known=True, clip=1000.0, inclusive=False, want_msp=True, want_score=True):
    """argmax_msp + dissum_score + the relabel against N <= 8 few-shot prototypes in one pass over the logits and one
    over the features (dml_open_world_post).  protos [N, C], new_labels [N]: prototype j relabels a pixel to
    new_labels[j] when its -|f - p_j|^2 is strictly above every other prototype's, above `thresh` and -- with
    vs_known -- above the best known-class logit (test_embedding.py:445; vs_known=False is the text of the 2- and
    3-class rules at :510-511,:520-522).  Returns (preds, msp, score); msp / score are None when not wanted."""
    _need_cuda(logits)
    lib = _lib.load()
    logits = logits.contiguous().float()
    B, K, H, W = logits.shape
    pr, lab, N = _protos_labels(protos, new_labels, logits.device)
    if N:
        feats = feats.contiguous().float()
        C = feats.shape[-1]
        if pr.shape[1] != C or feats.numel() != B * H * W * C:
            raise ValueError("feats must be [B, H, W, C] and protos [N, C]")
    else:
        C = int(feats.shape[-1]) if feats is not None else 1
    dev = logits.device
    preds = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    msp = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_msp else None
    score = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_score else None
    work = torch.empty(2 * B, dtype=torch.float32, device=dev) if want_score else None
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    _lib.check(lib.dml_open_world_post(logits.data_ptr(), ptr(feats) if N else None, ptr(pr), ptr(lab), preds.data_ptr(),
                                       ptr(msp), ptr(score), ptr(work), B, C, K, H, W, N, float(thresh),
                                       1 if vs_known else 0, float(clip), 1 if inclusive else 0, _st(logits)),
               "dml_open_world_post")
    return preds, msp, score


def novel_relabel_multi(preds: torch.Tensor, logits: torch.Tensor, feats: torch.Tensor, protos, new_labels, thresh=-1.5,
                        vs_known=True) -> torch.Tensor:
    """In place, for callers that already hold predictions: open_world_post's relabel rule alone."""
    _need_cuda(logits)
    lib = _lib.load()
    logits, feats = logits.contiguous().float(), feats.contiguous().float()
    B, K, H, W = logits.shape
    C = feats.shape[-1]
    pr, lab, N = _protos_labels(protos, new_labels, logits.device)
    if N and (pr.shape[1] != C or feats.numel() != B * H * W * C):
        raise ValueError("feats must be [B, H, W, C] and protos [N, C]")
    assert preds.is_contiguous() and preds.dtype == torch.int64 and preds.numel() == B * H * W
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    _lib.check(lib.dml_novel_relabel_multi(feats.data_ptr(), logits.data_ptr(), ptr(pr), ptr(lab), preds.data_ptr(), B, C,
                                           K, H, W, N, float(thresh), 1 if vs_known else 0, _st(logits)),
               "dml_novel_relabel_multi")
    return preds


def extract_prototypes(features: torch.Tensor, labels_true: torch.Tensor, class_ids, min_fraction: float = 0.05):
    """extract_prototype for up to 8 classes in one read of the features and one device -> host copy:
    {class_id: shot (list of C floats) or None when the class covers at most `min_fraction` of the pixels}."""
    _need_cuda(features)
    lib = _lib.load()
    ids = [int(c) for c in class_ids]
    if len(set(ids)) != len(ids):
        _lib.check(-1, "dml_class_feature_sums (duplicate class ids)")
    f = features.contiguous().float()
    C = f.shape[-1]
    f = f.view(-1, C)
    lab = labels_true.contiguous().view(-1)
    if lab.dtype != torch.int64 or lab.numel() != f.shape[0] or not lab.is_cuda:
        raise ValueError("labels_true must be an int64 CUDA tensor with one entry per pixel of `features`")
    M = len(ids)
    # sums [M, C] and the counts behind them in one double buffer, so that a single copy brings both to the host
    buf = torch.empty(M * C + M, dtype=torch.float64, device=f.device)
    cid = torch.tensor(ids, dtype=torch.int64, device=f.device)
    _lib.check(lib.dml_class_feature_sums(f.data_ptr(), lab.data_ptr(), f.shape[0], C, cid.data_ptr(), M, buf.data_ptr(),
                                          buf.data_ptr() + 8 * M * C, _st(f)), "dml_class_feature_sums")
    host = buf.cpu().numpy()
    sums, counts = host[:M * C].reshape(M, C), host[M * C:].view(np.uint64)
    out = {}
    for m, c in enumerate(ids):
        n = int(counts[m])
        out[c] = None if n == 0 or n / f.shape[0] <= min_fraction else \
            torch.from_numpy(sums[m] / n).float().tolist()
    return out
