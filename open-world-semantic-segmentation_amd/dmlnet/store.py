"""Flat parameter storage: every parameter, gradient and momentum of a model in one fp32 buffer each."""
import itertools
from typing import List, Optional

import torch
import torch.nn as nn


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


class ParamStore:
    """All parameters in ONE fp32 buffer (conv weights physically K-R-S-C), gradients and SGD momentum
    in two more.  nn.Parameters become views, so `state_dict()` keeps the reference's 674 keys and OIHW
    shapes, the optimizer is one streaming kernel per LR group and the gradient all-reduce works on
    contiguous buckets."""

    ALIGN = 64

    def __init__(self, model: nn.Module):
        self.model = model
        heads = model.head_modules() if hasattr(model, "head_modules") else [model.classifier]
        self.params: List[nn.Parameter] = list(model.backbone.parameters())
        for h in heads:
            self.params += list(h.parameters())
        self.n_backbone = len(list(model.backbone.parameters()))
        self.offsets: List[int] = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += _round_up(p.numel(), self.ALIGN)
        self.total = off
        self.split = self.offsets[self.n_backbone] if self.n_backbone < len(self.params) else off
        self.flat_p: Optional[torch.Tensor] = None
        self.flat_g: Optional[torch.Tensor] = None
        self.flat_v: Optional[torch.Tensor] = None     # momentum, created by the optimizer
        self.bn_modules = [m for m in itertools.chain(model.backbone.modules(), *[h.modules() for h in heads])
                           if isinstance(m, nn.BatchNorm2d)]
        self.flat_rs: Optional[torch.Tensor] = None
        self.flat_nbt: Optional[torch.Tensor] = None
        self.version = 0            # bumped by FusedSGD.step(); see Plan.refresh_weights
        self.grad_views: List[torch.Tensor] = []

    @staticmethod
    def _view(flat, off, p):
        n = p.numel()
        seg = flat[off:off + n]
        if p.dim() == 4:
            o, i, kh, kw = p.shape
            return seg.view(o, kh, kw, i).permute(0, 3, 1, 2)
        return seg.view(p.shape)

    def is_bound(self, device) -> bool:
        if self.flat_p is None or self.flat_p.device != device:
            return False
        base = self.flat_p.data_ptr()
        for idx in (0, len(self.params) // 2, len(self.params) - 1):
            p = self.params[idx]
            if p.device != device or p.data_ptr() != base + 4 * self.offsets[idx] or p.dtype != torch.float32:
                return False
        return True

    @torch.no_grad()
    def bind(self, device):
        """(Re)build the flat buffers from the current parameter values and re-point the modules at them."""
        flat_p = torch.zeros(self.total, dtype=torch.float32, device=device)
        for p, off in zip(self.params, self.offsets):
            src = p.detach().to(device=device, dtype=torch.float32)
            if src.dim() == 4:
                src = src.permute(0, 2, 3, 1)
            flat_p[off:off + p.numel()].copy_(src.reshape(-1))
        for p, off in zip(self.params, self.offsets):
            p.data = self._view(flat_p, off, p)
            p.grad = None
        self.flat_p = flat_p
        self.flat_g = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.grad_views = [self._view(self.flat_g, off, p) for p, off in zip(self.params, self.offsets)]
        self.flat_v = None
        # running statistics
        n_rs = sum(2 * m.num_features for m in self.bn_modules)
        flat_rs = torch.zeros(n_rs, dtype=torch.float32, device=device)
        flat_nbt = torch.zeros(len(self.bn_modules), dtype=torch.int64, device=device)
        off = 0
        for i, m in enumerate(self.bn_modules):
            c = m.num_features
            flat_rs[off:off + c].copy_(m.running_mean.detach().to(device))
            flat_rs[off + c:off + 2 * c].copy_(m.running_var.detach().to(device))
            m.running_mean.data = flat_rs[off:off + c]
            m.running_var.data = flat_rs[off + c:off + 2 * c]
            flat_nbt[i] = int(m.num_batches_tracked)
            m.num_batches_tracked.data = flat_nbt[i]
            off += 2 * c
        self.flat_rs, self.flat_nbt = flat_rs, flat_nbt
        self.version += 1

    def grad_ptr_of(self, p: nn.Parameter) -> int:
        idx = self._index(p)
        return self.flat_g.data_ptr() + 4 * self.offsets[idx]

    def _index(self, p):
        if not hasattr(self, "_idmap"):
            self._idmap = {id(q): i for i, q in enumerate(self.params)}
        return self._idmap[id(p)]

    # gradient bookkeeping around a backward pass ----------------------------------------------
    def begin_backward(self) -> str:
        """Returns 'fresh' (flat_g zeroed, grads will be attached) or 'accumulate'."""
        states = set()
        for p, gv in zip(self.params, self.grad_views):
            if p.grad is None:
                states.add("none")
            elif p.grad.data_ptr() == gv.data_ptr():
                states.add("ours")
            else:
                states.add("foreign")
        if states <= {"none"}:
            self.flat_g.zero_()
            return "fresh"
        if states <= {"ours"}:
            return "accumulate"
        # mixed: fold whatever the user had into our buffer, then accumulate on top of it
        with torch.no_grad():
            for p, gv in zip(self.params, self.grad_views):
                if p.grad is None:
                    gv.zero_()
                elif p.grad.data_ptr() != gv.data_ptr():
                    gv.copy_(p.grad)
        return "accumulate"

    def end_backward(self):
        for p, gv in zip(self.params, self.grad_views):
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                p.grad = gv
