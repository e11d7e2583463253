"""DML losses on the HIP path.

CrossEntropyLoss mirrors the LIVE behaviour of the reference's utils/loss.py:25-42: CE(ignore_index, mean
over valid pixels) / n; alpha/beta/gamma are accepted and -- exactly as in the reference, whose VAR / Inter /
Center terms sit behind an early `return` (loss.py:42-82) -- do not change the value.
DMLLoss is the live DCE + VL loss of anomaly/models/models.py:42-78: CE/n + alpha * VAR/n.
Both run dml_loss_fwd / dml_loss_bwd (one fused pass each instead of a per-image per-class Python loop).
FocalLoss is utils/loss.py:7-23 there, on dml_focal_loss_fwd / dml_focal_loss_bwd (csrc/focal_loss.hip); the sum reduction
CrossEntropyLoss(size_average=False) of loss.py:36,42 is that loss with alpha = 1, gamma = 0, divided by the image count.
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


class DMLLoss(nn.Module):
    """loss = CE/n + alpha*VAR/n, VAR = sum_i (1/HW_i) sum_{valid p} dist^2(p, own prototype).

    `sync` (True or a process group): sums are all-reduced so that every rank sees the loss of the global
    batch -- the value nn.DataParallel's gather gives the reference (main_embedding.py:466-467)."""

    def __init__(self, alpha=0.01, ignore_index=-1, sync=None, fused_backward=False):
        super().__init__()
        self.alpha, self.ignore_index, self.sync = alpha, ignore_index, sync
        # True: d(loss)/d(logits) is not materialised; valid when this loss is the only consumer of `logit`, as in the
        # reference's drivers (dmlnet/lazy_grad.py)
        self.fused_backward = fused_backward

    def forward(self, logit, target, features_in=None):
        return _DMLLossFn.apply(logit, target, self.alpha, self.ignore_index, self.sync, self.fused_backward)


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
