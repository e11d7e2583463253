"""DML losses on the HIP path.

CrossEntropyLoss mirrors the LIVE behaviour of the reference's utils/loss.py:25-42: CE(ignore_index, mean
over valid pixels) / n; alpha/beta/gamma are accepted and -- exactly as in the reference, whose VAR / Inter /
Center terms sit behind an early `return` (loss.py:42-82) -- do not change the value.
DMLLoss is the live DCE + VL loss of anomaly/models/models.py:42-78: CE/n + alpha * VAR/n.
Both run dml_loss_fwd / dml_loss_bwd (one fused pass each instead of a per-image per-class Python loop).
DMLLoss(beta=, gamma=) adds the Inter and Center terms of loss.py:43-79 there on dml_metric_fwd / dml_metric_bwd (csrc/metric_terms.hip).
FocalLoss is utils/loss.py:7-23 there, on dml_focal_loss_fwd / dml_focal_loss_bwd (csrc/focal_loss.hip); the sum reduction
CrossEntropyLoss(size_average=False) of loss.py:36,42 is that loss with alpha = 1, gamma = 0, divided by the image count.
CrossEntropyLoss_dis is loss.py:84-122 there with its feature-distillation term (:104-117) on dml_distill_fwd / dml_distill_bwd
(csrc/distill_loss.hip), off by default as in the reference.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from dmlnet import _lib


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


_COUNTS = {}


def _image_count(device, n):
    """a cached one-element fp64 device tensor holding `n` (device-to-device copies never wait for the stream)"""
    key = (str(device), int(n))
    t = _COUNTS.get(key)
    if t is None:
        t = torch.full((1,), float(n), dtype=torch.float64, device=device)
        _COUNTS[key] = t
    return t


class _DMLLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target, alpha, ignore_index, group, fused=False):
        if not logit.is_cuda:
            raise RuntimeError("the DML loss runs on the HIP path only (no CPU fallback)")
        lib = _lib.load()
        logit = logit.contiguous().float()
        target = target.contiguous().long()
        B, K, H, W = logit.shape
        if target.shape != (B, H, W):
            raise RuntimeError("target shape %s does not match logits %s" % (tuple(target.shape), tuple(logit.shape)))
        sums = torch.empty(5, dtype=torch.float64, device=logit.device)
        part = torch.empty(_lib.LOSS_BLOCKS * 4, dtype=torch.float32, device=logit.device)
        st = _stream(logit)
        _lib.check(lib.dml_loss_fwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), part.data_ptr(), B, K, H, W,
                                    int(ignore_index), st), "dml_loss_fwd")
        n_images = float(B)
        if group is not None:
            import torch.distributed as dist
            # the reference normalises by the size of the gathered batch (utils/loss.py:38-41 on DataParallel's
            # gather); shards may be uneven (parallel.shard_range spreads a remainder), so the image count travels
            # with the sums (sums[4], read by the kernels on the device: no host sync) instead of assuming B * world
            # (not `sums[4] = float(B)`: assigning a Python scalar to a CUDA element copies from pageable host memory and BLOCKS the
            # host until the stream has drained -- the whole forward, 26 ms per step at 16 x 768 x 768 -- tools/probe_allreduce_host_block.py)
            sums[4:5].copy_(_image_count(logit.device, B), non_blocking=True)
            dist.all_reduce(sums, group=group if group is not True else None)
            n_images = 0.0
        loss = torch.empty((), dtype=torch.float32, device=logit.device)
        _lib.check(lib.dml_loss_finalize(sums.data_ptr(), loss.data_ptr(), float(alpha), n_images, st),
                   "dml_loss_finalize")
        ctx.save_for_backward(logit, target, sums)
        ctx.cfg = (float(alpha), int(ignore_index), n_images, bool(fused))
        return loss

    @staticmethod
    def backward(ctx, gout):
        logit, target, sums = ctx.saved_tensors
        alpha, ignore_index, n_images, fused = ctx.cfg
        if fused:
            # no gradient tensor: a marker the model's backward resolves in its fused head kernel (dmlnet/lazy_grad.py)
            from dmlnet import lazy_grad
            return lazy_grad.issue(logit, target, sums, gout.contiguous().float(), alpha, ignore_index, n_images), \
                None, None, None, None, None
        lib = _lib.load()
        B, K, H, W = logit.shape
        g = torch.empty_like(logit)
        gout = gout.contiguous().float()
        _lib.check(lib.dml_loss_bwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), gout.data_ptr(),
                                    g.data_ptr(), B, K, H, W, ignore_index, alpha, n_images, _stream(logit)),
                   "dml_loss_bwd")
        return g, None, None, None, None, None


class _DMLMetricLossFn(torch.autograd.Function):
    """CE/n + alpha VAR/n + (beta Inter + gamma Center)/n in one function: dml_loss_fwd + dml_metric_fwd and their finalizes;
    backward dml_loss_bwd, then dml_metric_bwd adds the Inter gradient into the same buffer and writes the feature gradient."""

    @staticmethod
    def forward(ctx, logit, target, feats, alpha, beta, gamma, ignore_index, group):
        if not logit.is_cuda:
            raise RuntimeError("the DML loss runs on the HIP path only (no CPU fallback)")
        lib = _lib.load()
        logit = logit.contiguous().float()
        target = target.contiguous().long()
        B, K, H, W = logit.shape
        if target.shape != (B, H, W):
            raise RuntimeError("target shape %s does not match logits %s" % (tuple(target.shape), tuple(logit.shape)))
        if not 1 <= K <= 32:
            raise ValueError("the Inter and Center terms take 1 <= classes <= 32, got %d" % K)
        C = 1
        ctx.feats_dtype = None if feats is None else feats.dtype
        if gamma != 0:
            feats = feats.detach().contiguous().float()
            if feats.dim() != 4 or tuple(feats.shape[:3]) != (B, H, W):
                raise RuntimeError("features %s are not [B, H, W, C] of logits %s" % (tuple(feats.shape), tuple(logit.shape)))
            C = feats.shape[3]
            if not 1 <= C <= 32:
                raise ValueError("the Center term takes 1 <= channels <= 32, got %d" % C)
        else:
            feats = None
        dev = logit.device
        sums = torch.empty(5, dtype=torch.float64, device=dev)
        part = torch.empty(_lib.LOSS_BLOCKS * 4, dtype=torch.float32, device=dev)
        msums = torch.empty(2 * B + 3, dtype=torch.float64, device=dev)
        work = torch.empty(_lib.metric_work_doubles(K, C), dtype=torch.float64, device=dev)
        means = torch.empty((B, K, C), dtype=torch.float32, device=dev) if feats is not None else None
        counts = torch.empty((B, K), dtype=torch.int32, device=dev) if feats is not None else None
        st = _stream(logit)
        _lib.check(lib.dml_loss_fwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), part.data_ptr(), B, K, H, W,
                                    int(ignore_index), st), "dml_loss_fwd")
        _lib.check(lib.dml_metric_fwd(logit.data_ptr() if beta != 0 else None, None if feats is None else feats.data_ptr(),
                                      target.data_ptr(), None if feats is None else means.data_ptr(),
                                      None if feats is None else counts.data_ptr(), msums.data_ptr(), work.data_ptr(), B, K, C, H, W,
                                      int(ignore_index), st), "dml_metric_fwd")
        n_images = float(B)
        if group is not None:
            import torch.distributed as dist
            # as in _DMLLossFn.forward: the image count travels with the sums, on the device
            sums[4:5].copy_(_image_count(dev, B), non_blocking=True)
            grp = group if group is not True else None
            dist.all_reduce(sums, group=grp)
            dist.all_reduce(msums[2 * B:], group=grp)
            n_images = 0.0
        both = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.dml_loss_finalize(sums.data_ptr(), both.data_ptr(), float(alpha), n_images, st), "dml_loss_finalize")
        _lib.check(lib.dml_metric_finalize(msums.data_ptr(), B, float(beta), float(gamma), n_images, both.data_ptr() + 4, st),
                   "dml_metric_finalize")
        ctx.save_for_backward(logit, target, sums, msums, feats, means)
        ctx.cfg = (float(alpha), float(beta), float(gamma), int(ignore_index), n_images)
        return both[0] + both[1]

    @staticmethod
    def backward(ctx, gout):
        logit, target, sums, msums, feats, means = ctx.saved_tensors
        alpha, beta, gamma, ignore_index, n_images = ctx.cfg
        lib = _lib.load()
        B, K, H, W = logit.shape
        C = 1 if feats is None else feats.shape[3]
        st = _stream(logit)
        g = torch.empty_like(logit)
        gout = gout.contiguous().float()
        _lib.check(lib.dml_loss_bwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), gout.data_ptr(),
                                    g.data_ptr(), B, K, H, W, ignore_index, alpha, n_images, st), "dml_loss_bwd")
        gf = torch.empty_like(feats) if feats is not None and ctx.needs_input_grad[2] else None
        if beta != 0 or gf is not None:
            _lib.check(lib.dml_metric_bwd(None if gf is None else feats.data_ptr(), target.data_ptr(),
                                          None if gf is None else means.data_ptr(), msums.data_ptr(), gout.data_ptr(),
                                          g.data_ptr() if beta != 0 else None, None if gf is None else gf.data_ptr(), B, K, C, H, W,
                                          ignore_index, beta, gamma, n_images, st), "dml_metric_bwd")
        if gf is not None and gf.dtype != ctx.feats_dtype:
            gf = gf.to(ctx.feats_dtype)
        return g, None, gf, None, None, None, None, None


class DMLLoss(nn.Module):
    """loss = CE/n + alpha*VAR/n + beta*Inter/n + gamma*Center/n, per image i with N = H W pixels (the ignored ones counted):
    VAR_i = (1/N) sum_{valid p} dist^2(p, own prototype), Inter_i = (1/N) sum_{valid p} sum_{k != y_p} logit[i,k,p],
    Center_i = (1/N) sum_{valid p} |features_in[i,p] - mean of features_in[i] over the pixels of class y_p|^2 -- the three terms of
    the reference's utils/loss.py:43-79.  features_in [B,H,W,C] is taken flat over H W: the reference indexes features_in[i] with
    flat pixel indices along its first dimension, which fails for an image with a class pixel at index >= H; the geometry it
    intended is the one computed here.  An image without a valid pixel and a class of one pixel contribute 0 to Center.

    beta = gamma = 0 (the default) is the loss as it was: the same kernels, value and gradient bit for bit, features_in unused.
    Otherwise dml_metric_fwd / dml_metric_bwd (csrc/metric_terms.hip) run beside dml_loss_fwd / dml_loss_bwd; for gamma != 0
    features_in is required and receives a gradient, and fused_backward falls back to the materialised logit gradient (the fused
    head backward takes no gradient on the features), as CrossEntropyLoss(size_average=False) does.

    `sync` (True or a process group): sums are all-reduced so that every rank sees the loss of the global
    batch -- the value nn.DataParallel's gather gives the reference (main_embedding.py:466-467)."""

    def __init__(self, alpha=0.01, ignore_index=-1, sync=None, fused_backward=False, beta=0.0, gamma=0.0):
        super().__init__()
        beta, gamma = float(beta), float(gamma)
        if not (math.isfinite(beta) and math.isfinite(gamma)):
            raise ValueError("DMLLoss needs finite beta and gamma, got beta=%r gamma=%r" % (beta, gamma))
        self.alpha, self.ignore_index, self.sync = alpha, ignore_index, sync
        self.beta, self.gamma = beta, gamma
        # True: d(loss)/d(logits) is not materialised; valid when this loss is the only consumer of `logit`, as in the
        # reference's drivers (dmlnet/lazy_grad.py)
        self.fused_backward = fused_backward

    def forward(self, logit, target, features_in=None):
        if self.beta == 0 and self.gamma == 0:
            return _DMLLossFn.apply(logit, target, self.alpha, self.ignore_index, self.sync, self.fused_backward)
        if self.gamma != 0 and features_in is None:
            raise ValueError("DMLLoss needs features_in for gamma != 0")
        return _DMLMetricLossFn.apply(logit, target, features_in if self.gamma != 0 else None, self.alpha, self.beta, self.gamma,
                                      self.ignore_index, self.sync)


class _FocalLossFn(torch.autograd.Function):
    """-> (loss, pixel count): the count (B H W of the global batch, a device double) is not differentiable"""

    @staticmethod
    def forward(ctx, logit, target, alpha, gamma, size_average, ignore_index, group):
        if not logit.is_cuda:
            raise RuntimeError("the focal loss runs on the HIP path only (no CPU fallback)")
        lib = _lib.load()
        logit = logit.contiguous().float()
        target = target.contiguous().long()
        B, K, H, W = logit.shape
        if target.shape != (B, H, W):
            raise RuntimeError("target shape %s does not match logits %s" % (tuple(target.shape), tuple(logit.shape)))
        sums = torch.empty(4, dtype=torch.float64, device=logit.device)
        part = torch.empty(_lib.FOCAL_PARTIALS, dtype=torch.float32, device=logit.device)
        st = _stream(logit)
        _lib.check(lib.dml_focal_loss_fwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), part.data_ptr(), B, K, H, W,
                                          int(ignore_index), alpha, gamma, st), "dml_focal_loss_fwd")
        if group is not None:
            import torch.distributed as dist
            # the divisor of the global batch travels in sums[2], which the forward kernel left on the device: no host
            # synchronisation and no Python scalar assigned to a CUDA element (see _DMLLossFn.forward)
            dist.all_reduce(sums, group=group if group is not True else None)
        loss = torch.empty((), dtype=torch.float32, device=logit.device)
        _lib.check(lib.dml_focal_loss_finalize(sums.data_ptr(), loss.data_ptr(), int(size_average), st),
                   "dml_focal_loss_finalize")
        ctx.save_for_backward(logit, target, sums)
        ctx.cfg = (alpha, gamma, int(size_average), int(ignore_index))
        pixels = sums[2]
        ctx.mark_non_differentiable(pixels)
        return loss, pixels

    @staticmethod
    def backward(ctx, gout, _gpixels):
        logit, target, sums = ctx.saved_tensors
        alpha, gamma, size_average, ignore_index = ctx.cfg
        lib = _lib.load()
        B, K, H, W = logit.shape
        g = torch.empty_like(logit)
        gout = gout.contiguous().float()
        _lib.check(lib.dml_focal_loss_bwd(logit.data_ptr(), target.data_ptr(), sums.data_ptr(), gout.data_ptr(),
                                          g.data_ptr(), B, K, H, W, ignore_index, alpha, gamma, size_average,
                                          _stream(logit)), "dml_focal_loss_bwd")
        return g, None, None, None, None, None, None


class FocalLoss(nn.Module):
    """fl = alpha (1 - pt)^gamma ce per valid pixel, 0 on an ignored one; size_average: sum fl / (B H W), the ignored pixels
    counted (the reference's .mean() of a reduction='none' map), else sum fl.  Where pt rounds to 1 the gradient is the
    analytic limit (0 for gamma > 0), not the NaN the reference's autograd has for 0 < gamma < 1.

    The third argument of forward is accepted and ignored: the embedding drivers call criterion(outputs, labels, features).
    `sync` (True or a process group): the sums are all-reduced, every rank sees the global batch's loss and divisor.
    d loss / d logits is always materialised (there is no fused_backward here)."""

    def __init__(self, alpha=1, gamma=0, size_average=True, ignore_index=255, sync=None):
        super().__init__()
        alpha, gamma = float(alpha), float(gamma)
        if not (math.isfinite(alpha) and math.isfinite(gamma)) or gamma < 0:
            raise ValueError("FocalLoss needs a finite alpha and a finite gamma >= 0, got alpha=%r gamma=%r" % (alpha, gamma))
        self.alpha, self.gamma = alpha, gamma
        self.ignore_index, self.size_average, self.sync = ignore_index, size_average, sync

    def forward(self, inputs, targets, features_in=None):
        if inputs.dim() != 4 or inputs.shape[1] < 1:
            raise ValueError("FocalLoss takes logits [B, K, H, W] with K >= 1, got %s" % (tuple(inputs.shape),))
        return _FocalLossFn.apply(inputs, targets, self.alpha, self.gamma, bool(self.size_average), self.ignore_index,
                                  self.sync)[0]


class _DistillFn(torch.autograd.Function):
    """(student features, teacher features, labels, teacher logits or None) -> (dis, labels the mask was taken from): the labels
    with their ignored pixels filled when teacher logits are given, the labels themselves otherwise.  Neither the teacher nor
    the labels are differentiable."""

    @staticmethod
    def forward(ctx, feats_s, feats_t, target, teacher_logits, ignore_index, novel_id, group):
        if not feats_s.is_cuda:
            raise RuntimeError("the distillation loss runs on the HIP path only (no CPU fallback)")
        lib = _lib.load()
        s = feats_s.detach().contiguous().float()
        t = feats_t.detach().contiguous().float()
        target = target.contiguous().long()
        if s.dim() != 4 or t.dim() != 4 or s.shape[:3] != t.shape[:3] or tuple(target.shape) != tuple(s.shape[:3]):
            raise RuntimeError("features [B, H, W, C] of teacher %s and student %s and labels %s do not match"
                               % (tuple(t.shape), tuple(s.shape), tuple(target.shape)))
        B, Hh, Ww, Cs = s.shape
        Ct = t.shape[3]
        if not 1 <= Ct <= Cs <= 32:
            raise ValueError("the distillation loss takes 1 <= teacher channels <= student channels <= 32, got %d and %d" % (Ct, Cs))
        lg_ptr, filled = None, target
        if teacher_logits is not None:
            lg = teacher_logits.detach().contiguous().float()
            if tuple(lg.shape) != (B, Ct, Hh, Ww):
                raise RuntimeError("teacher logits %s do not match teacher features %s" % (tuple(lg.shape), tuple(t.shape)))
            lg_ptr, filled = lg.data_ptr(), torch.empty_like(target)
        sums = torch.empty(2 * B + 2, dtype=torch.float64, device=s.device)
        part = torch.empty(_lib.DISTILL_PARTIALS, dtype=torch.float32, device=s.device)
        st = _stream(s)
        _lib.check(lib.dml_distill_fwd(lg_ptr, t.data_ptr(), s.data_ptr(), target.data_ptr(),
                                       filled.data_ptr() if lg_ptr is not None else None, sums.data_ptr(), part.data_ptr(),
                                       B, Ct, Cs, Hh, Ww, int(ignore_index), int(novel_id), st), "dml_distill_fwd")
        n_images = float(B)
        if group is not None:
            import torch.distributed as dist
            # sum_i S_i / cnt_i and the image count of the global batch: the kernel left both on the device (sums[2B], sums[2B+1]),
            # so nothing comes to the host and no Python scalar is assigned to a CUDA element (see _DMLLossFn.forward)
            dist.all_reduce(sums[2 * B:], group=group if group is not True else None)
            n_images = 0.0
        dis = torch.empty((), dtype=torch.float32, device=s.device)
        _lib.check(lib.dml_distill_finalize(sums.data_ptr(), B, n_images, dis.data_ptr(), st), "dml_distill_finalize")
        ctx.save_for_backward(t, s, filled, sums)
        ctx.cfg = (int(novel_id), n_images)
        ctx.mark_non_differentiable(filled)
        return dis, filled

    @staticmethod
    def backward(ctx, gout, _gfilled):
        t, s, filled, sums = ctx.saved_tensors
        novel_id, n_images = ctx.cfg
        lib = _lib.load()
        B, Hh, Ww, Cs = s.shape
        g = torch.empty_like(s)
        gout = gout.contiguous().float()
        _lib.check(lib.dml_distill_bwd(t.data_ptr(), s.data_ptr(), filled.data_ptr(), sums.data_ptr(), gout.data_ptr(),
                                       g.data_ptr(), B, t.shape[3], Cs, Hh, Ww, novel_id, n_images, _stream(s)),
                   "dml_distill_bwd")
        return g, None, None, None, None, None, None


class CrossEntropyLoss_dis(nn.Module):
    """The two-model loss of the reference's main_distillation.py (utils/loss.py:84-122 there): CE(logit, target) / n, plus
    dis_weight * dis with  dis = (1/n) sum_i (1/cnt_i) sum_{p: target != novel_id} |features_2 - pad(features_1)|^2  -- the
    feature-distillation term the reference wrote behind an early `return` (:104-117, coefficient 0.01).  dis_weight = 0 (the
    default) is the reference's live behaviour: the value and gradient of CrossEntropyLoss, bit for bit, and no kernel of
    csrc/distill_loss.hip is launched.  An image without a masked-in pixel contributes 0 (the reference: NaN).

    forward(logit, target, features_1, features_2, teacher_logits=None): features_1 [B,H,W,Ct] is the teacher's embedding
    (detached), features_2 [B,H,W,Cs] the student's (the gradient goes there), Ct <= Cs <= 32.  With `teacher_logits`
    ([B,Ct,H,W]) the ignored pixels of `target` take the teacher's prediction (main_distillation.py:428-430) inside the
    distillation forward launch, for any dis_weight, and the cross entropy reads the filled labels; `target` itself is not
    written.  alpha, beta, gamma are accepted and unused, as in the reference.
    `sync` (True or a process group): the sums of both terms are all-reduced, every rank sees the global batch's loss.
    The cross entropy's gradient is always materialised: the fused head backward takes no gradient on the features."""

    def __init__(self, alpha=0, beta=0, gamma=0, size_average=True, ignore_index=255, dis_weight=0.0, novel_id=16, sync=None):
        super().__init__()
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.ignore_index, self.size_average, self.sync = ignore_index, size_average, sync
        self.dis_weight, self.novel_id = float(dis_weight), int(novel_id)
        if not math.isfinite(self.dis_weight):
            raise ValueError("CrossEntropyLoss_dis needs a finite dis_weight, got %r" % (dis_weight,))
        self._ce = CrossEntropyLoss(size_average=size_average, ignore_index=ignore_index, sync=sync)

    def forward(self, logit, target, features_1=None, features_2=None, teacher_logits=None):
        dis = None
        if self.dis_weight != 0 or teacher_logits is not None:
            if features_1 is None or features_2 is None:
                raise ValueError("CrossEntropyLoss_dis needs features_1 and features_2 for dis_weight != 0 or teacher_logits")
            if self.dis_weight == 0:
                features_2 = features_2.detach()                      # the fill alone: nothing reaches the features
            dis, target = _DistillFn.apply(features_2, features_1, target, teacher_logits, self.ignore_index, self.novel_id,
                                           self.sync)
        ce = self._ce(logit, target)
        return ce if self.dis_weight == 0 else ce + self.dis_weight * dis


class CrossEntropyLoss(nn.Module):
    def __init__(self, alpha=0, beta=0, gamma=0, size_average=True, ignore_index=255, sync=None, fused_backward=False):
        super().__init__()
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.ignore_index, self.size_average, self.sync = ignore_index, size_average, sync
        self.fused_backward = fused_backward

    def forward(self, logit, target, features_in=None):
        if not self.size_average:
            # the reference's sum reduction over n (utils/loss.py:36,42 there): sum nll / n -- the focal kernels with alpha = 1,
            # gamma = 0; n of the global batch is its pixel count over H W, on the device.  The gradient is materialised
            # whatever fused_backward says: the fused head backward knows the mean reduction only.
            total, pixels = _FocalLossFn.apply(logit, target, 1.0, 0.0, False, self.ignore_index, self.sync)
            return total * (float(logit.shape[2] * logit.shape[3]) / pixels).float()
        return _DMLLossFn.apply(logit, target, 0.0, self.ignore_index, self.sync, self.fused_backward)
