"""The pieces a plan is built from: buffers (`Act`), the fp16 planes of f16x2 plans, conv lowering, the conv + BatchNorm unit both ways."""
# `PlanPieces` knows no network: dmlnet/deeplab.py, dmlnet/engine_ppm.py and the tests' plans of one block or one head (tests/helpers.py)
# put these pieces together.
import contextlib
import ctypes as C
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from ._lib import DML_BF16, DML_F32, STAT_ROWS, ConvDesc, WgradDesc
from .launch_list import BoundArgs
from .switches import PlanSwitches

_PAD_CIN = 8         # stem input channels 3 -> 8 so that a 16-byte vector never straddles a filter tap


class _S2DConv:
    """The stem's k x k stride-2 convolution (resnet.py:139: 7x7, padding 3, on the 3 image channels) in space-to-depth form: a
    (k + 1) / 2 square stride-1 convolution on [B][H/2][W/2][4 C] (dml_pack_input_s2d) with the weights regrouped per step
    (dml_s2d_weights) and the weight gradient scattered back into the parameter's layout (dml_s2d_wgrad).  Same products on
    K = 192 instead of the 392 of the image padded to 8 channels.  Quacks like the nn.Conv2d the plan builder reads."""

    def __init__(self, conv: nn.Conv2d, Ho: int, Wo: int):
        k, p = conv.kernel_size[0], conv.padding[0]
        self.real, self.k = conv, k
        self.kernel_size, self.stride, self.dilation = ((k + 1) // 2,) * 2, (1, 1), (1, 1)
        self.padding = ((p + 1) // 2,) * 2
        self.in_channels, self.out_channels = 4 * conv.in_channels, conv.out_channels
        self.weight, self.bias = conv.weight, conv.bias
        self.out_hw = (Ho, Wo)

    @staticmethod
    def fits(conv: nn.Conv2d, H: int, W: int) -> bool:
        k, p = conv.kernel_size[0], conv.padding[0]
        return (conv.kernel_size == (k, k) and k % 2 == 1 and conv.stride == (2, 2) and conv.padding == (p, p) and p == (k - 1) // 2
                and p % 2 == 1 and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and H % 2 == 0 and W % 2 == 0)


def _dt(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return DML_F32
    if dtype == torch.bfloat16:
        return DML_BF16
    raise ValueError("compute dtype must be torch.float32 or torch.bfloat16, got %r" % (dtype,))


class Act:
    """An NHWC activation (or gradient) living in a plan-owned buffer; may be a channel slice."""
    __slots__ = ("t", "ptr", "B", "H", "W", "C", "ld", "f32", "es", "grad", "grad_init", "root", "g32", "h2", "amax", "h2_used")

    def __init__(self, t, ptr, B, H, W, C, ld, f32, es):
        self.t, self.ptr, self.B, self.H, self.W, self.C, self.ld, self.f32, self.es = t, ptr, B, H, W, C, ld, f32, es
        self.grad = None            # Act holding d(loss)/d(this)
        self.grad_init = False      # has any producer written the gradient yet?
        self.root = self            # concat buffer this is a slice of
        self.g32 = None             # fp32 staging of the gradient while it still has producers to come (Plan.stage_grad32)
        self.h2 = None              # (fp16 hi / lo planes, work) of this fp32 tensor once a conv has asked for them (Plan.h2_of)
        self.amax = None            # its `work` buffer when the producers of the tensor collect max |x| into work[0] (Plan.amax_of)
        self.h2_used = False        # has a conv asked for the planes?  (planes written by the producer itself: Plan.h2_direct)

    @property
    def M(self):
        return self.B * self.H * self.W

    def slice(self, c0, c):
        a = Act(self.t, self.ptr + c0 * self.es, self.B, self.H, self.W, c, self.ld, self.f32, self.es)
        a.root = self.root
        return a


class HeadRec:
    """per-head pieces of a plan (activations, units, the argument lists patched per call)"""


class ConvUnit:
    __slots__ = ("conv", "bn", "x", "y", "z", "relu", "res", "w", "wt", "scale", "shift", "mean", "invstd",
                 "Cp", "drop", "apply_args", "gscale_slots", "dz", "dy", "mask", "frozen", "dtype", "up")


# the fp16 planes of a tensor come with a `work` buffer of 1025 floats (dml_h2_split): 1024 partial maxima of |x|, then the
# word the conv kernels read -- 1 / scale of the planes
H2_WORK_FLOATS = 1025
UNSCALE_OFFSET = 4 * 1024         # bytes from a work buffer's start to its 1 / scale word
NO_PLANES = (None, 0, 0, None)    # the planes arguments of a BatchNorm kernel that writes none (see PlanPieces.planes_args)


def unscale_ptr(work) -> int:
    return work.data_ptr() + UNSCALE_OFFSET


def root_count(n) -> float:
    """sqrt(n) in fp32, nudged up: the factor by which a batch-statistics BatchNorm output can exceed |gamma| (DmlH2BoundDesc)"""
    return float(np.float32(np.sqrt(np.float32(n))) * np.float32(1.0001))


class PlanPieces:
    def __init__(self, engine: "Engine", B: int, H: int, W: int, dtype: torch.dtype, training: bool, predict_heads=None):
        self.e = engine
        self.sw = PlanSwitches()
        # prediction plan (Engine.predict): the first `predict_heads` heads up to their final 1x1 convolution, then ONE
        # dml_incremental_predict over their low-resolution embeddings instead of a dml_upsample_dist_fwd per head
        self.predict_heads = predict_heads
        if predict_heads is not None and training:
            raise ValueError("a prediction plan is an inference plan")
        self.lib = engine.lib
        self.B, self.H, self.W = B, H, W
        self._set_dtype(dtype)
        self.training = training
        self.device = engine.store.flat_p.device
        self.fwd, self.bwd = [], []    # the op lists: (entry point, BoundArgs) in issue order
        self.prep: list = []          # weight preparation (re-run when the masters change)
        self.keep: list = []           # keeps ctypes structs / tensors alive
        self.units: List[ConvUnit] = []
        self.momentum_slots = []       # (args_list, index, bn)
        self.prepped_version = None
        self.param_last_op = {}        # param index -> index of the last backward op that adds to its gradient
        self.prep_table = None
        self.side = {}                 # backward op index -> True if it must first wait for the main stream
        self._side_events = None
        self._nat, self._ev_handles, self._ev_objs = {}, None, None
        self.drop_units = []
        self.sync = bool(engine.sync_bn and training and dist.is_available() and dist.is_initialized()
                         and dist.get_world_size(engine.sync_group) > 1)
        self.world = dist.get_world_size(engine.sync_group) if self.sync else 1
        self.last_dgrad = {}           # gradient buffer address -> ConvDesc of the data gradient that wrote it last
        self.res_src = {}              # id(block input) -> (dz of the block output, its ReLU mask): identity-branch gradient
        #                                that conv1's data gradient adds in its epilogue (DmlConvDesc.res_*)
        # fp32 plans: products of the forward / data-gradient convolutions on the bf16 matrix cores through a three-term
        # split of both operands (DmlConvDesc.f32_split; fp32-level error, not the exact fp32 MFMA): Engine.f32_split
        # (2: two fp16 planes per operand, written by dml_h2_split before the first conv that reads a tensor: Plan.h2_of)
        self.f32_split = int(engine.f32_split) if dtype == torch.float32 else 0
        self.prep_h2 = []              # dml_h2_split argument lists of the weight copies, run after every dml_prep_weights
        self.prep_h2_table = None      # (device array of DmlH2Desc, count) built from them: dml_h2_split_table
        # `work` buffers of dml_h2_split (1025 floats per tensor), carved from one allocation so that ONE fill at the head of
        # the forward zeroes every amax word the step's producers will raise (dml_bn_apply / dml_bn_bwd_apply, `amax`)
        self.h2_slots = (torch.zeros(H2_WORK_FLOATS * 1024, dtype=torch.float32, device=self.device) if self.f32_split == 2
                         else None)
        self.h2_used = 0
        self.direct_planes = []        # (activation, argument list, index of its `planes` argument): cleared when nobody asks
        self.prep_gather = []          # dml_gather_taps argument lists: sub-filters of the transposed weight copies, refreshed with them
        self._bound_words, self._bound_used = None, 0
        self.stage32 = training and dtype == torch.bfloat16 and self.sw.grad_stage32      # (PlanSwitches.grad_stage32)
        self.pre_prep = []             # host steps of refresh_weights that run before the copies are made (padded_final_conv)
        self.nbt_inc = None            # per-BatchNorm increments of num_batches_tracked where some layers are frozen (build)
        # shared scratch for BN partial statistics (forward: ceil(M/rows)*N*2 floats, rows = 64 or 48 (dml_conv_stat_rows):
        # <= 2/3 B*H*W for every layer of this network; backward: <= ~1100*N*2)
        self.scratch = torch.empty(max(B * H * W * 3 // 4 + 16384, 1100 * 2048 * 2 + 65536), dtype=torch.float32,
                                   device=self.device)
        self.sp = self.scratch.data_ptr()
        # split-K partials of the weight gradients (one launch at a time uses it: all of them run on one stream)
        self.wgrad_ws = torch.empty(64 * (1 << 20) if training else 1, dtype=torch.float32, device=self.device)
        # K-split of partially filled last rounds in the main-stream convolutions (DmlConvDesc.tail_*): one workspace and
        # one counter array for the whole plan (the launches that use them are serialised on the caller's stream)
        self.tail_ws = torch.empty(512 * 128 * 128 if training else 1, dtype=torch.float32, device=self.device)
        self.tail_cnt = torch.zeros(128, dtype=torch.int32, device=self.device)
        self._wg_pending = []
        self.build()
        self.bytes = sum(t.numel() * t.element_size() for t in self.keep if isinstance(t, torch.Tensor))

    def _set_dtype(self, dtype):
        # storage type of the tensors made from here on: element size `es`, elements per 16-byte vector `vec`
        self.dtype, self.dt = dtype, _dt(dtype)
        self.es = 2 if dtype == torch.bfloat16 else 4
        self.vec = 16 // self.es

    @contextlib.contextmanager
    def precision(self, dtype):
        """a unit may keep its tensors in fp32 inside a bf16 plan (the ASPP image-pooling branch, see _head_fwd)"""
        saved = self.dtype
        self._set_dtype(dtype)
        try:
            yield self
        finally:
            self._set_dtype(saved)

    @property
    def planes_mode(self) -> bool:
        """fp32 tensors as two fp16 planes per conv operand (f16x2); evaluated at use: precision() changes `dtype` in mid-build"""
        return self.f32_split == 2 and self.dtype == torch.float32

    # ---- allocation helpers
    def new(self, B, H, W, C, f32=False, ld=None, zero=False) -> Act:
        ld = ld or C
        dtype = torch.float32 if f32 else self.dtype
        alloc = torch.zeros if zero else torch.empty
        t = alloc(B * H * W * ld, dtype=dtype, device=self.device)
        self.keep.append(t)
        return Act(t, t.data_ptr(), B, H, W, C, ld, f32 or self.dtype == torch.float32, t.element_size())

    def dbuf(self, n):
        return self.fbuf(n, zero=True, dtype=torch.float64)

    def py_op(self, ops, fn):
        """A host-side step of the plan (a collective): called as fn(stream), runs on the caller's current stream."""
        def op(stream):
            fn()
            return 0
        ops.append((op, BoundArgs()))

    def fbuf(self, n, zero=False, dtype=torch.float32):
        t = (torch.zeros if zero else torch.empty)(max(int(n), 1), dtype=dtype, device=self.device)
        self.keep.append(t)
        return t

    def device_table(self, arr):
        """a host array of descriptors as bytes on the plan's device (the caller keeps the tensor alive)"""
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)

    def grad_of(self, a: Act) -> Act:
        """Gradient buffer of an activation (slices share their concat buffer's gradient)."""
        root = a.root
        if root.grad is None:
            root.grad = self.new(root.B, root.H, root.W, root.C)
        if a is root:
            return root.grad
        return root.grad.slice((a.ptr - root.ptr) // a.es, a.C)

    def stage_grad32(self, a: Act):
        """Declare d(loss)/d(a) a gradient with several producers (bf16 plans): the producers accumulate into an fp32
        staging tensor and the last one (conv_dgrad(final=True), or a conversion) rounds the total once into the bf16
        gradient the consumers read.  Rounding after every producer -- what a bf16 accumulate does -- costs about twice
        the noise power: d(out) collects the pooled term and four ASPP data gradients, and the BatchNorm backward that
        differences it amplifies whatever rounding noise it carries (profiles/r02_bf16_noise_by_depth.txt)."""
        if not self.stage32 or a is not a.root or a.g32 is not None or a.C % 8 or a.C <= 32 or a.f32:
            return
        a.g32 = self.new(a.B, a.H, a.W, a.C, f32=True)

    def call(self, ops, fn, *args):
        lst = BoundArgs(args)
        ops.append((fn, lst))
        return lst

    # ---- the frame of every forward: two table launches at its head whose tables are known once the forward is built
    def begin_forward(self, bn_eval_table: bool):
        # bn_eval_table: some BatchNorm normalises with its running statistics (cbr appends to `bn_eval`)
        self.bn_eval, self.bn_eval_args = [], None
        self.h2_bound_tab, self.h2_bound_args = [], None
        if self.h2_slots is not None and self.training:
            # every amax word of the step starts from zero (Plan.amax_of; the backward's words are raised after the forward)
            self.call(self.fwd, self.lib.dml_fill_f32, self.h2_slots.data_ptr(), self.h2_slots.numel(), 0.0)
            # the plane scales of every residual-free BatchNorm output (they depend on gamma / beta / count only): one launch,
            # table filled in by end_forward
            self.h2_bound_args = self.call(self.fwd, self.lib.dml_h2_bound_bn_table, 0, 0)
        if bn_eval_table:
            self.bn_eval_args = self.call(self.fwd, self.lib.dml_bn_eval_coeffs_table, 0, 0)      # filled in by end_forward

    def end_forward(self):
        if self.h2_bound_args is not None and self.h2_bound_tab:
            self.h2_bound_table = self.device_table((_lib.H2BoundDesc * len(self.h2_bound_tab))(*self.h2_bound_tab))
            self.h2_bound_args[0], self.h2_bound_args[1] = self.h2_bound_table.data_ptr(), len(self.h2_bound_tab)
        if self.bn_eval:
            self.bn_eval_table = self.device_table((_lib.BnEvalDesc * len(self.bn_eval))(*self.bn_eval))
            self.bn_eval_args[0], self.bn_eval_args[1] = self.bn_eval_table.data_ptr(), len(self.bn_eval)

    # ---- fp32 plans with fp32_products = "f16x2": fp16 hi / lo planes of a conv operand (DmlConvDesc.x_planes)
    def h2_ok(self, C, N, taps, dgrad=False):
        """shapes the planes kernel takes (conv_ws_planes_eligible); the others run the three-term split on the fp32 tensors.
        dgrad: a data-gradient launch (mode 1), whose K = taps x C must be at least two K stages (2 x BK = 64)"""
        return self.planes_mode and C % 32 == 0 and N % 64 == 0 and taps <= 32 and (not dgrad or taps * C >= 64)

    @staticmethod
    def planes_fit(M, ld):
        """both fp16 planes of an [M][ld] tensor within the 31-bit byte offsets of the planes kernels (launch_conv / dml_conv_wgrad
        fall back to the fp32 tensors beyond): a tensor may exist as planes ONLY when this holds"""
        return 4 * M * ld < (1 << 31) - 4096

    def bound_state(self):
        """two zeroed 32-bit words (running maximum, ticket) of one dml_bn_*finalize_bound launch: left zero by every call"""
        if self._bound_words is None:
            self._bound_words = torch.zeros(2 * 1024, dtype=torch.int32, device=self.device)
            self.keep.append(self._bound_words)
        assert self._bound_used < 1024, "out of bound-state words"
        p = self._bound_words.data_ptr() + 8 * self._bound_used
        self._bound_used += 1
        return p

    def h2_work(self):
        assert self.h2_used < 1024, "out of dml_h2_split work buffers"
        w = self.h2_slots[self.h2_used * H2_WORK_FLOATS:(self.h2_used + 1) * H2_WORK_FLOATS]
        self.h2_used += 1
        return w

    def amax_of(self, a: Act):
        """pointer for the `amax` argument of the kernel that writes activation `a` (None outside f16x2 plans): every
        producer of a root tensor raises the same word, and the split then needs no maximum pass of its own"""
        if not self.planes_mode or not a.f32 or a is not a.root:
            return None         # (a slice of a concat buffer: its other producers -- resize, broadcast -- do not report a maximum)
        root = a.root
        if root.amax is None:
            root.amax = self.h2_work()
        return root.amax.data_ptr()

    def h2_of(self, a: Act, ops):
        """(planes pointer, plane stride in elements, pointer to 1 / scale) of activation `a`; the split of its ROOT tensor is
        appended to `ops` the first time a conv asks -- every tensor of a plan is complete before its first consumer and never
        rewritten within a step, so one split per tensor and step serves all its consumers (forward conv, weight gradient)."""
        root = a.root
        root.h2_used = True
        if root.h2 is None:
            planes = torch.empty(2 * root.M * root.ld, dtype=torch.float16, device=self.device)
            known = root.amax is not None           # its producers collected max |x| (amax_of)
            work = root.amax if known else self.h2_work()
            self.keep.append(planes)
            self.call(ops, self.lib.dml_h2_split, root.ptr, root.M, root.C, root.ld, planes.data_ptr(), root.M * root.ld, root.ld,
                      0, work.data_ptr(), 1 if known else 0)
            root.h2 = (planes, work)
        planes, work = root.h2
        return planes.data_ptr() + (a.ptr - root.ptr) // 2, root.M * root.ld, unscale_ptr(work)

    def h2_direct(self, B, H, W, C, fp32_too: bool, work=None) -> Act:
        """a new fp32 activation whose producer (dml_bn_apply / dml_bn_bwd_apply) writes the fp16 planes itself; without
        `fp32_too` the fp32 tensor does not exist -- the Act then points at the planes (same extent: 2 x 2 bytes per element)
        and only planes consumers may read it"""
        planes = torch.empty(2 * B * H * W * C, dtype=torch.float16, device=self.device)
        self.keep.append(planes)
        a = self.new(B, H, W, C) if fp32_too else Act(planes, planes.data_ptr(), B, H, W, C, C, True, 4)
        a.h2 = (planes, work if work is not None else self.h2_work())
        return a

    @staticmethod
    def planes_args(a: Act):
        """(planes pointer, plane stride, row length, pointer to 1 / scale) for the BatchNorm kernel that writes `a` (h2_direct)"""
        planes, work = a.h2
        return planes.data_ptr(), a.M * a.C, a.C, unscale_ptr(work)

    def h2_weight(self, w, rows, K):
        """planes of a prepared fp32 weight copy [rows][K] (tile-major), refreshed with the copies (refresh_weights)"""
        if getattr(w, "h2", None) is None:
            planes = torch.empty(2 * rows * K, dtype=torch.float16, device=self.device)
            work = torch.zeros(H2_WORK_FLOATS, dtype=torch.float32, device=self.device)
            self.keep += [planes, work]
            self.prep_h2.append((w.data_ptr(), rows, K, K, planes.data_ptr(), rows * K, K, 1, work.data_ptr(), 0))
            self.prepped_version = None
            w.h2 = (planes, work)
        planes, work = w.h2
        return planes.data_ptr(), rows * K, unscale_ptr(work)

    def set_planes(self, dsc, x: Act, w, rows, K, ops):
        """DmlConvDesc.f32_split / x_planes / w_planes of a conv of this plan reading activation x and weight copy w[rows][K]"""
        dsc.f32_split = min(self.f32_split, 1)
        if self.h2_ok(x.C, rows, dsc.R * dsc.S, dgrad=dsc.mode == 1):
            dsc.f32_split = 2
            dsc.x_planes, dsc.x_plane_stride, dsc.x_unscale = self.h2_of(x, ops)
            dsc.w_planes, dsc.w_plane_stride, dsc.w_unscale = self.h2_weight(w, rows, K)

    # ---- graph pieces ------------------------------------------------------------------------
    def conv_geom(self, conv: nn.Conv2d, x: Act):
        kh, kw = conv.kernel_size
        s, d, p = conv.stride[0], conv.dilation[0], conv.padding[0]
        Ho = (x.H + 2 * p - d * (kh - 1) - 1) // s + 1
        Wo = (x.W + 2 * p - d * (kw - 1) - 1) // s + 1
        if isinstance(conv, _S2DConv):
            Ho, Wo = conv.out_hw                  # (the zero taps of the regrouped filter reach one row / column further)
        return kh, kw, s, d, p, Ho, Wo

    def prep_weight(self, conv: nn.Conv2d, Cp: int, need_wt: bool, src_ptr=None, N=None, x_bytes=0, dy_bytes=0):
        """compute copies w[N][RS][Cp] (and wt[Cp][RS][N] for the data gradient) of a master weight; `src_ptr` / `N`
        override the source and the row count (the final conv's rows are padded to a multiple of 8, see build()).
        `x_bytes` / `dy_bytes`: extents of the forward / data-gradient operand tensors of this conv."""
        N, Cm = N or conv.out_channels, conv.in_channels
        kh, kw = conv.kernel_size
        if isinstance(conv, _S2DConv):
            assert Cp == Cm and self.dtype == torch.float32 and not need_wt
            w = torch.empty(N * kh * kw * Cm, dtype=torch.float32, device=self.device)
            w.tiled = False
            self.keep.append(w)
            self.call(self.fwd, self.lib.dml_s2d_weights, conv.weight.data_ptr(), w.data_ptr(), N, conv.k, conv.real.in_channels)
            return w, None
        w = torch.empty(N * kh * kw * Cp, dtype=self.dtype, device=self.device)
        wt = torch.empty(N * kh * kw * Cp, dtype=self.dtype, device=self.device) if need_wt else None
        # tile-major copies for the LDS-DMA kernels (DmlConvDesc.w_tiled): bf16, the GEMM's K a multiple of 32 per filter tap and
        # its row count a multiple of 64 -- the shapes those kernels take; conv_fwd / conv_dgrad pass the flag on.  Those kernels
        # address their operands with 31-bit byte offsets (launch_conv's `small` test): a conv whose activation or weight tensor
        # reaches 2 GiB falls back to the register-staged kernel, which reads the plain layout only -- no tile-major copy then.
        lim = 1 << 31
        dma = (self.sw.tiled_weights and self.dtype == torch.bfloat16 and kh * kw <= 32 and N * kh * kw * Cp * 2 < lim)
        w.tiled = bool(dma and Cp % 32 == 0 and N % 64 == 0 and x_bytes < lim)
        if wt is not None:
            wt.tiled = bool(dma and N % 32 == 0 and Cp % 64 == 0 and dy_bytes < lim)
        self.keep += [w, wt]
        self.prep.append((src_ptr or conv.weight.data_ptr(), w.data_ptr(), wt.data_ptr() if wt is not None else 0, N,
                          kh * kw, Cm, Cp, self.dt, 1 if w.tiled else 0, 1 if (wt is not None and wt.tiled) else 0))
        return w, wt

    def padded_final_conv(self, fin: nn.Conv2d, K: int, Kp: int, need_wt: bool):
        """A final 1x1 conv whose class count K is no multiple of 8 (the factory default is 21) computes Kp channels from a
        zero-padded copy of its weight / bias, so the embedding's pad channels are exactly 0, the prototypes are padded with
        zeros too, and every kernel keeps its 16-byte channel vectors.  Returns prep_weight's copies and the bias pointer."""
        cin = fin.in_channels
        wpad, bpad = self.fbuf(Kp * cin, zero=True), self.fbuf(Kp, zero=True)

        def stage():
            wpad[:K * cin].copy_(fin.weight.detach().reshape(-1))
            if fin.bias is not None:
                bpad[:K].copy_(fin.bias.detach())
        self.pre_prep.append(stage)
        w, wt = self.prep_weight(fin, cin, need_wt, src_ptr=wpad.data_ptr(), N=Kp)
        return w, wt, bpad.data_ptr() if fin.bias is not None else None

    def issue_conv(self, ops, dsc, tail=True):
        """what every conv launch sets alike (ws_min_tiles; `tail`: the K-split of a partially filled last round), then the launch"""
        dsc.ws_min_tiles = self.sw.ws_min_tiles
        if tail:
            dsc.tail_ws, dsc.tail_ws_elems = self.tail_ws.data_ptr(), self.tail_ws.numel()
            dsc.tail_counters, dsc.tail_counters_len = self.tail_cnt.data_ptr(), self.tail_cnt.numel()
        self.keep.append(dsc)
        self.call(ops, self.lib.dml_conv_igemm, C.byref(dsc))

    def conv_fwd(self, x: Act, conv: nn.Conv2d, y: Act, w, stats_ptr, bias_ptr=None, post=None, N=None):
        kh, kw, s, d, p, Ho, Wo = self.conv_geom(conv, x)
        assert (Ho, Wo) == (y.H, y.W), ((Ho, Wo), (y.H, y.W))
        dsc = ConvDesc(x=x.ptr, w=w.data_ptr(), y=y.ptr, bias=bias_ptr, stats=stats_ptr, B=x.B, Hi=x.H, Wi=x.W, C=x.C, ldx=x.ld, Ho=Ho, Wo=Wo,
                       N=N or conv.out_channels, ldy=y.ld, R=kh, S=kw, stride=s, dil=d, pad=p, dtype=self.dt,
                       y_f32=1 if (y.f32 and self.dtype != torch.float32) else 0, accum=0, mode=0)
        self.set_planes(dsc, x, w, dsc.N, kh * kw * x.C, self.fwd)
        dsc.w_tiled = 1 if getattr(w, "tiled", False) else 0
        if post is not None:           # inference epilogue: BN(running stats) + residual + ReLU (DmlConvDesc.post_*)
            scale, shift, mean, res, relu = post
            dsc.post_scale, dsc.post_shift, dsc.post_mean = scale.data_ptr(), shift.data_ptr(), mean.data_ptr()
            dsc.post_res, dsc.post_ldres = (res.ptr, res.ld) if res is not None else (None, 0)
            dsc.post_relu = 1 if relu else 0
        self.issue_conv(self.fwd, dsc, tail=self.training)
        return dsc

    def conv_dgrad(self, dy: Act, conv: nn.Conv2d, wt, x: Act, final=True):
        """d(loss)/dx (+)= conv^T(dy); x.grad is created on demand.  `final`: no producer of this gradient comes after
        this one (only looked at for staged gradients, stage_grad32)."""
        gx = self.grad_of(x)
        kh, kw, s, d, p, _, _ = self.conv_geom(conv, x)
        if self.s2_classes_ok(dy, conv, x, kh, kw, s, d, p):
            return self.conv_dgrad_s2_classes(dy, conv, wt, x, gx, kh, kw, p)
        dsc = ConvDesc(x=dy.ptr, w=wt.data_ptr(), y=gx.ptr, bias=None, stats=None, B=dy.B, Hi=dy.H, Wi=dy.W, C=dy.C, ldx=dy.ld, Ho=x.H, Wo=x.W, N=x.C,
                       ldy=gx.ld, R=kh, S=kw, stride=s, dil=d, pad=p, dtype=self.dt, y_f32=0,
                       accum=1 if x.root.grad_init else 0, mode=1)
        self.set_planes(dsc, dy, wt, x.C, kh * kw * dy.C, self.bwd)
        dsc.w_tiled = 1 if getattr(wt, "tiled", False) else 0
        g32 =x.g32 if x is x.root else None
        convert = False
        if g32 is not None and not (final and not x.root.grad_init):
            if final and dy.C % 32 == 0 and kh * kw <= 32:
                # last producer: conv + fp32 sum of the others, rounded once (DmlConvDesc.acc32, LDS-DMA kernels)
                dsc.accum, dsc.acc32, dsc.acc32_ld = 0, g32.ptr, g32.ld
            else:
                dsc.y, dsc.ldy, dsc.y_f32 = g32.ptr, g32.ld, 1
                convert = final
        else:
            g32 = None
        res = self.res_src.pop(id(x), None)
        if res is not None:
            # the identity branch's share of this gradient (block output gradient x ReLU mask) is added in the epilogue
            assert not x.root.grad_init and x is x.root and g32 is None
            rdz, rmask = res
            dsc.res_dz, dsc.res_mask, dsc.res_ld = rdz.ptr, rmask.data_ptr(), rdz.ld
        x.root.grad_init = True
        self.issue_conv(self.bwd, dsc)
        if convert:
            self.round_staged(x)
        self.last_dgrad.pop(self.grad_of(x.root).ptr, None)
        if x is x.root and g32 is None:
            self.last_dgrad[gx.ptr] = dsc         # whole-tensor gradient: candidate for the fused BN-backward reduce

    # ---- data gradient of a stride-2 convolution as one stride-1 launch per pixel-parity class (DmlConvDesc.sub_grid)
    def s2_classes_ok(self, dy, conv, x, kh, kw, s, d, p):
        """f16x2 plans, 3x3 / pad 1 and 1x1 / pad 0 at stride 2 on even maps, shapes the two-plane kernel takes.  A pixel of dX only sees
        the taps of its own row / column parity: the 3x3 becomes four launches of 1, 2, 2 and 4 taps (nine tap products per four pixels
        instead of 36, most of them on zeros), the 1x1 one launch on the even pixels -- which requires that the gradient already holds
        its other producers' sum (it only ADDS there)."""
        if not (self.sw.s2_classes and s == 2 and d == 1 and kh == kw and (kh, p) in ((3, 1), (1, 0))
                and self.planes_mode and not isinstance(conv, _S2DConv)):
            return False
        if x is not x.root or x.g32 is not None or x.H != 2 * dy.H or x.W != 2 * dy.W or dy.C % 32 or x.C % 64:
            return False
        # every class is a launch of the planes kernel, whose data gradients need K = taps x dy.C >= 2 x BK = 64
        # (conv_ws_planes_eligible); the smallest class has one tap (3x3: odd rows and columns, 1x1: the even pixels)
        if dy.C < 64:
            return False
        if kh == 1 and not x.root.grad_init:
            return False
        return self.planes_fit(dy.M, dy.ld) and 16 * dy.M * x.C < (1 << 31) - 4096

    def conv_dgrad_s2_classes(self, dy, conv, wt, x, gx, kh, kw, p):
        accum = 1 if x.root.grad_init else 0
        xpl = self.h2_of(dy, self.bwd)
        descs = []
        for cy in (0, 1):
            for cx in (0, 1):
                rs = [r for r in range(kh) if (r - cy - p) % 2 == 0]
                ss = [t for t in range(kw) if (t - cx - p) % 2 == 0]
                if not rs or not ss:
                    continue                         # (1x1: only the even pixels receive anything; the gradient is accumulated into)
                taps = [r * kw + t for r in rs for t in ss]
                # the class's operand: rows = dX channels, K = its taps x dY channels, from the transposed copy wt[C][R S][N]
                sub = self.fbuf(x.C * len(taps) * dy.C)
                self.prep_gather.append((wt.data_ptr(), sub.data_ptr(), x.C, kh * kw, dy.C, len(taps), *(taps + [0] * (4 - len(taps)))))
                self.prepped_version = None
                dsc = ConvDesc(x=dy.ptr, w=sub.data_ptr(), y=gx.ptr, bias=None, stats=None, B=dy.B, Hi=dy.H, Wi=dy.W, C=dy.C, ldx=dy.ld,
                               Ho=dy.H, Wo=dy.W, N=x.C, ldy=gx.ld, R=len(rs), S=len(ss), stride=1, dil=1, pad=(cy + p - rs[0]) // 2,
                               dtype=self.dt, y_f32=0, accum=accum, mode=1)
                dsc.pad_w_set, dsc.pad_w = 1, (cx + p - ss[0]) // 2
                dsc.sub_grid, dsc.sub_y, dsc.sub_x = 1, cy, cx
                dsc.f32_split = 2
                dsc.x_planes, dsc.x_plane_stride, dsc.x_unscale = xpl
                dsc.w_planes, dsc.w_plane_stride, dsc.w_unscale = self.h2_weight(sub, x.C, len(taps) * dy.C)
                self.issue_conv(self.bwd, dsc)
                descs.append(dsc)
        x.root.grad_init = True
        prev = self.last_dgrad.pop(gx.ptr, None)
        if len(descs) == 4:
            self.last_dgrad[gx.ptr] = descs           # the four classes cover the tensor: candidates for the fused BN-backward sums
        elif (len(descs) == 1 and accum and prev is not None and not isinstance(prev, list) and not prev.sub_grid
              and self.sw.bnr_inc
              and prev.y == gx.ptr and prev.N == x.C and prev.ldy == gx.ld and prev.f32_split == 2 and not prev.res_dz):
            # 1x1: the class launch only visits the even pixels, but the BatchNorm-backward sums are linear in the gradient -- the
            # producer before it (a whole-tensor data gradient) emits the sums of the total stored SO FAR over all pixels, this launch those
            # of its increment over its own (DmlConvDesc.bnr_inc); unit_bwd hands both their partial groups
            descs[0].bnr_inc = 1
            self.last_dgrad[gx.ptr] = [prev, descs[0]]

    def round_staged(self, x: Act):
        """fp32 staging tensor -> the bf16 gradient (a staged gradient whose last producer cannot do it itself)"""
        g = self.grad_of(x)
        assert x is x.root and g.ld == g.C and x.g32.ld == g.C
        self.call(self.bwd, self.lib.dml_convert_dtype, x.g32.ptr, g.ptr, g.M * g.C, DML_F32, DML_BF16)

    def conv_wgrad(self, x: Act, dy: Act, conv: nn.Conv2d, Cp: int, pad_rows: int = 0):
        """pad_rows: dy carries `pad_rows` >= out_channels channels (zero beyond); the padded rows of the gradient
        go to a scratch tensor and only the real ones are added to the parameter's gradient."""
        kh, kw, s, d, p, Ho, Wo = self.conv_geom(conv, x)
        Cm = conv.in_channels
        gptr = self.e.store.grad_ptr_of(conv.weight)
        h2 = None
        if self.planes_mode and x.C % 8 == 0 and (pad_rows or conv.out_channels) % 8 == 0:
            # both operands as fp16 planes (the forward already split x; dy is split once for this and the data gradient).  The
            # splits are appended HERE, before `first`: they belong to the main stream, whose data gradient reads dy's planes too
            h2 = self.h2_of(x, self.bwd) + self.h2_of(dy, self.bwd)
        first = len(self.bwd)
        Nw, tmp = conv.out_channels, None
        s2d = isinstance(conv, _S2DConv)
        assert not (s2d and pad_rows)
        if s2d or (pad_rows and pad_rows != Nw):        # the gradient goes to a scratch tensor first, in the layout the kernel writes
            Nw = pad_rows or Nw
            tmp = self.fbuf(Nw * kh * kw * Cm)
            self.call(self.bwd, self.lib.dml_fill_f32, tmp.data_ptr(), tmp.numel(), 0.0)
        dsc = WgradDesc(x=x.ptr, dy=dy.ptr, dw=tmp.data_ptr() if tmp is not None else gptr, B=x.B, Hi=x.H, Wi=x.W, C=x.C,
                        ldx=x.ld, Ho=Ho, Wo=Wo,
                        N=Nw, ldy=dy.ld, R=kh, S=kw, stride=s, dil=d, pad=p, dtype=self.dt, splitk=0,
                        Cm=Cm, ws=self.wgrad_ws.data_ptr(), ws_elems=self.wgrad_ws.numel(),
                        f32_split=min(self.f32_split, 1) if self.dtype == torch.float32 else 0)
        if h2 is not None:
            dsc.f32_split = 2
            (dsc.x_planes, dsc.x_plane_stride, dsc.x_unscale, dsc.dy_planes, dsc.dy_plane_stride, dsc.dy_unscale) = h2
        self.keep.append(dsc)
        if tmp is None and self.sw.group_wgrad and self.lib.dml_conv_wgrad_group_eligible(C.byref(dsc)):
            # joins the next grouped launch (dml_conv_wgrad_group): the weight gradients of a few consecutive layers
            # share one round of workgroups, so each needs a handful of split-K slabs instead of ~28
            Ktot = kh * kw * x.C
            base = (Nw // 256) * ((Ktot + 255) // 256)
            self._wg_pending.append((dsc, conv, base))
            if sum(b for _, _, b in self._wg_pending) >= self.sw.group_tiles or len(self._wg_pending) >= 12:
                self.flush_wgrad()
            return
        self.call(self.bwd, self.lib.dml_conv_wgrad, C.byref(dsc))
        if s2d:
            self.call(self.bwd, self.lib.dml_s2d_wgrad, tmp.data_ptr(), gptr, conv.out_channels, conv.k, conv.real.in_channels)
        elif tmp is not None:
            self.call(self.bwd, self.lib.dml_unpad_wgrad, tmp.data_ptr(), gptr, conv.out_channels, kh * kw, Cm, Cm)
        # weight gradients only feed the optimizer: they run on a side stream, next to the HBM-bound BN backward
        # and the data gradient of the following layers (Plan.run_backward)
        for i in range(first, len(self.bwd)):
            self.side[i] = (i == first)
        self.mark_grad(conv.weight)

    def flush_wgrad(self):
        """emit the pending weight-gradient jobs as one grouped launch on the side stream"""
        pend, self._wg_pending = self._wg_pending, []
        if not pend:
            return
        arr = (C.c_void_p * len(pend))(*[C.addressof(d) for d, _, _ in pend])
        self.keep.append(arr)
        i = len(self.bwd)
        args = self.call(self.bwd, self.lib.dml_conv_wgrad_group, C.addressof(arr), len(pend), self.wgrad_ws.data_ptr(),
                         self.wgrad_ws.numel())
        args.meta = [d for d, _, _ in pend]                 # bench.py: FLOPs / bytes of the launch
        self.side[i] = True
        for _, conv, _ in pend:
            self.param_last_op[self.e.store._index(conv.weight)] = i

    def mark_grad(self, p):
        self.param_last_op[self.e.store._index(p)] = len(self.bwd) - 1

    def cbr(self, x: Act, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu=True, res: Optional[Act] = None,
            out: Optional[Act] = None, drop: Optional[nn.Dropout] = None, need_dgrad=True, planes_only=False,
            pool_fused=False) -> ConvUnit:
        """conv -> BN(batch or running stats) -> (+res) -> (ReLU) -> (dropout); z may be a concat slice.
        planes_only: only planes consumers read z (the convolutions of an f16x2 plan) -- no fp32 z where the BN writes planes.
        pool_fused: the caller applies the BatchNorm inside its pooling pass (the stem, Plan.build): conv and statistics only, the unit
        has no z (its mask is the caller's to fill)."""
        lib = self.lib
        u = ConvUnit()
        u.conv, u.bn, u.x, u.relu, u.res, u.drop = conv, bn, x, relu, res, drop
        u.dtype = self.dtype
        u.gscale_slots, u.mask, u.apply_args = [], None, None        # (filled in below where the unit has them)
        u.Cp = x.C                       # x already carries any channel padding
        kh, kw, s, d, p, Ho, Wo = self.conv_geom(conv, x)
        N = conv.out_channels
        u.w, u.wt = self.prep_weight(conv, u.Cp, self.training and need_dgrad, x_bytes=x.M * x.ld * x.es,
                                     dy_bytes=x.B * Ho * Wo * N * x.es)
        # f16x2 training: this BN writes z's fp16 planes itself (Plan.h2_direct) -- batch statistics bound the output
        direct = (self.sw.h2_direct and self.training and bn.training and self.planes_mode
                  and out is None and N % 8 == 0 and drop is None
                  and (res is None or (res is res.root and res.amax is not None)) and not pool_fused)
        planes_only = planes_only and direct and self.planes_fit(x.B * Ho * Wo, N)
        if pool_fused:
            assert self.training and bn.training and relu and res is None and out is None and drop is None and not self.sync
            u.z = None
        elif direct:
            u.z = self.h2_direct(x.B, Ho, Wo, N, fp32_too=not planes_only)
            if not planes_only or res is not None:
                # max |z| is published where something may ask for it: a conv reading the fp32 tensor through dml_h2_split, or the
                # next block's residual unit (its plane scale: dml_h2_bound_bn) -- also when z itself exists as planes only
                u.z.amax = u.z.h2[1]           # (the amax words and the scale word share the tensor's work buffer)
        else:
            u.z = out if out is not None else self.new(x.B, Ho, Wo, N)
        u.y = self.new(x.B, Ho, Wo, N) if self.training else None      # inference never materialises it
        M = x.B * Ho * Wo
        u.scale, u.shift = self.fbuf(N), self.fbuf(N)
        g_ptr, b_ptr = bn.weight.data_ptr(), bn.bias.data_ptr()
        mean_ptr = bn.running_mean.data_ptr()
        u.frozen = self.training and not bn.training
        if u.frozen:
            # BatchNorm2d.eval() inside a training step (main_self_distillation.py:432-435 of the reference): normalise
            # with the running statistics, leave them alone; gamma / beta still train.  scale / shift / invstd come from
            # the coefficient table launch at the head of the plan (two rows: the second with gamma = beta = None
            # yields 1/sqrt(var + eps) itself), the backward is the batch-statistics one without its correction terms.
            u.mean, u.invstd = bn.running_mean, self.fbuf(N)
            dummy = self.fbuf(N)
            self.bn_eval.append(_lib.BnEvalDesc(g_ptr, b_ptr, bn.running_var.data_ptr(), u.scale.data_ptr(),
                                                u.shift.data_ptr(), N, float(bn.eps)))
            self.bn_eval.append(_lib.BnEvalDesc(None, None, bn.running_var.data_ptr(), u.invstd.data_ptr(),
                                                dummy.data_ptr(), N, float(bn.eps)))
            self.conv_fwd(x, conv, u.y, u.w, None)
        elif self.training:
            u.mean, u.invstd = self.fbuf(N), self.fbuf(N)
            mean_ptr = u.mean.data_ptr()
            bound_done = False
            dsc = self.conv_fwd(x, conv, u.y, u.w, self.sp)
            # rows per statistics partial of THIS launch (48 on the wave-specialised kernel, STAT_ROWS otherwise)
            rows = lib.dml_conv_stat_rows(C.byref(dsc))
            groups = (M + rows - 1) // rows
            assert groups * N * 2 <= self.scratch.numel(), "BN statistics scratch too small"
            # what the three finalize launches take alike, after four arguments of their own: gamma .. invstd, the momentum among them
            tail = (g_ptr, b_ptr, bn.running_mean.data_ptr(), bn.running_var.data_ptr(), 0.1, float(bn.eps),
                    u.scale.data_ptr(), u.shift.data_ptr(), u.mean.data_ptr(), u.invstd.data_ptr())
            if self.sync:
                # statistics over every rank's samples (equal shards): local (mean, M2) -> all_gather -> Chan merge
                mom, allmom = self.dbuf(N * 2), self.dbuf(self.world * N * 2)
                self.call(self.fwd, lib.dml_bn_moments, self.sp, M, N, rows, mom.data_ptr())
                grp = self.e.sync_group
                self.py_op(self.fwd, lambda a=allmom, b=mom, g=grp: dist.all_gather_into_tensor(a, b, group=g))
                args = self.call(self.fwd, lib.dml_bn_finalize_moments, allmom.data_ptr(), self.world, M, N, *tail)
            elif direct and self.sw.fuse_bound and not (res is None and self.h2_bound_args is not None):
                # f16x2: the plane scale of z from its bound (dml_h2_bound_bn) comes out of the SAME launch -- the finalize block
                # that arrives last writes it (dml_bn_finalize_bound: one dependent one-block launch less per residual unit)
                args = self.call(self.fwd, lib.dml_bn_finalize_bound, self.sp, M, N, rows, *tail, M * self.world, 1.0,
                                 res.amax.data_ptr() if res is not None else None, u.z.h2[1].data_ptr(), self.bound_state())
                bound_done = True
            else:
                args = self.call(self.fwd, lib.dml_bn_finalize, self.sp, M, N, rows, *tail)
            self.momentum_slots.append((args, 8, bn))       # (the per-step momentum: the 0.1 above)
        else:
            # inference: scale / shift of every BN come from ONE table launch at the head of the plan, and BN +
            # residual + ReLU run in the conv epilogue -- one launch per unit instead of three, no y tensor
            self.bn_eval.append(_lib.BnEvalDesc(g_ptr, b_ptr, bn.running_var.data_ptr(), u.scale.data_ptr(),
                                                u.shift.data_ptr(), N, float(bn.eps)))
            self.conv_fwd(x, conv, u.z, u.w, None, post=(u.scale, u.shift, bn.running_mean, res, relu))
            self.units.append(u)
            return u
        # ReLU bitmask (bf16 training): the two BN backward passes read 1 byte per 8 elements instead of z
        if self.training and relu and N % self.vec == 0:
            # one byte per 16-byte vector of z: 8 bits in bf16 plans, 4 in fp32 plans (the BN backward reads it instead of z)
            u.mask = torch.empty(M * (N // self.vec), dtype=torch.uint8, device=self.device)
            self.keep.append(u.mask)
        mask_ptr = u.mask.data_ptr() if u.mask is not None else None
        if pool_fused:
            self.units.append(u)
            return u
        pl = NO_PLANES
        if direct:
            work = u.z.h2[1]
            if bound_done:
                pass
            elif res is None and self.h2_bound_args is not None:
                self.h2_bound_tab.append(_lib.H2BoundDesc(g_ptr, b_ptr, work.data_ptr(), N, root_count(M * self.world), 1.0, 0))
            else:
                self.call(self.fwd, lib.dml_h2_bound_bn, g_ptr, b_ptr, N, M * self.world, 1.0,
                          res.amax.data_ptr() if res is not None else None, work.data_ptr())
            pl = self.planes_args(u.z)
        only = direct and planes_only
        if out is not None and out.root.t.dtype == torch.float16:
            # `out` is a channel slice of a tensor that exists as fp16 planes ONLY (the decoder's concat buffer of an f16x2 training
            # plan, _head_fwd): this BatchNorm writes its slice of the planes, scaled by the tensor's one scale (dml_h2_bound_bn_multi)
            assert self.training and bn.training and drop is None and self.dtype == torch.float32 and N % 8 == 0
            pp, pstride, punscale = self.h2_of(out, self.fwd)
            pl = (pp, pstride, out.ld, punscale)
            only = True
        # a residual operand that exists as planes only (the previous block's output, block_fwd): hi + lo, unscaled
        res_pl = (0, None)
        if res is not None and res.t.dtype == torch.float16:
            assert res is res.root and res.h2 is not None and self.dtype == torch.float32
            res_pl = (res.M * res.ld, unscale_ptr(res.h2[1]))
        u.apply_args = self.call(self.fwd, lib.dml_bn_apply, u.y.ptr, res.ptr if res is not None else None,
                                 None if only else u.z.ptr, u.scale.data_ptr(), u.shift.data_ptr(), mean_ptr, mask_ptr, M, N,
                                 u.y.ld, res.ld if res is not None else 0, u.z.ld, 1 if relu else 0, self.dt, 0.0, 0,
                                 self.amax_of(u.z) if (self.training and (not only or u.z.amax is not None)) else None, *pl,
                                 *res_pl)
        if direct and not only:
            self.direct_planes.append((u.z, u.apply_args, 17))
        if drop is not None and self.training:
            self.drop_units.append(u)
        self.units.append(u)
        return u

    # ---- dy of a unit's BatchNorm backward and its finalize launch: shared by unit_bwd and stem_bwd_fused.  Three steps, because the
    # reduce pass (each caller's own kernel) runs between the first two, and the marks of gamma / beta between the last two in unit_bwd
    def new_dy(self, u: ConvUnit, planes: bool, only: bool):
        # planes: the BatchNorm backward writes dy's fp16 planes itself, scaled from a bound (dml_h2_bound_bn_bwd) of max |g|, which its
        # reduce pass raises into the word `gwork`; only: no fp32 dy beside them.  Returns (dy, gwork)
        if planes:
            return self.h2_direct(u.y.B, u.y.H, u.y.W, u.y.C, fp32_too=not only), self.h2_work()
        return self.new(u.y.B, u.y.H, u.y.W, u.y.C), None

    def bn_bwd_finalize(self, u: ConvUnit, sp, nblk, count, coef, dy: Act, gwork) -> bool:
        """partial sums -> gamma / beta gradients and the apply pass's coefficients (count: 0 for a frozen BatchNorm).  Returns whether
        the launch also set dy's plane scale (f16x2: dml_h2_bound_bn_bwd in the finalize launch's last block, DML_FUSE_BOUND)"""
        st, bn = self.e.store, u.bn
        args = (sp, nblk, count, u.y.C, bn.weight.data_ptr(), u.mean.data_ptr(), u.invstd.data_ptr(), st.grad_ptr_of(bn.weight),
                st.grad_ptr_of(bn.bias), coef.data_ptr())
        if gwork is not None and self.sw.fuse_bound:
            self.call(self.bwd, self.lib.dml_bn_bwd_finalize_bound, *args, u.y.M * self.world, gwork.data_ptr(),
                      dy.h2[1].data_ptr(), self.bound_state())
            return True
        self.call(self.bwd, self.lib.dml_bn_bwd_finalize, *args)
        return False

    def dy_planes(self, u: ConvUnit, coef, dy: Act, gwork, bound_done: bool):
        """planes arguments of the apply pass that writes dy; the plane scale first where the finalize launch has not set it"""
        if gwork is None:
            return NO_PLANES
        if not bound_done:
            self.call(self.bwd, self.lib.dml_h2_bound_bn_bwd, coef.data_ptr(), u.invstd.data_ptr(), u.y.C, u.y.M * self.world,
                      gwork.data_ptr(), dy.h2[1].data_ptr())
        return self.planes_args(dy)

    def unit_bwd(self, u: ConvUnit, dz: Optional[Act], dres: Optional[Act] = None, dres_accum=False, need_dgrad=True, final=True,
                 up_mask=None, dz_from=None):
        """Backward of `cbr`: BN (two passes) -> weight gradient -> data gradient into u.x.grad (`final`: conv_dgrad).
        up_mask: `dz` is the gradient of a LATER ReLU's output and `up_mask` that ReLU's 1-bit mask -- this unit's own output gradient
        is dz (.) mask, formed on the fly by the two BN passes (block_bwd: the downsample branch reads the block output's gradient).
        dz_from = (de, w, K), with dz None: the output gradient is the data gradient of a 1x1 convolution with K output channels
        behind this unit, de [M][Kp] times its weight w [K][N], and the two BN passes form it themselves (_head_bwd, dml_head_bn_bwd_*)."""
        if u.dtype != self.dtype:
            with self.precision(u.dtype):
                return self.unit_bwd(u, dz, dres, dres_accum, need_dgrad, final, up_mask, dz_from)
        lib, st = self.lib, self.e.store
        N, M = u.conv.out_channels, u.y.M
        bn = u.bn
        # f16x2: the BN backward writes dy's fp16 planes itself, scaled from a bound (dml_h2_bound_bn_bwd); dy exists in fp32
        # only if one of its two consumers (weight gradient, data gradient) cannot read planes
        kh, kw = u.conv.kernel_size
        dy_direct = self.sw.h2_direct and self.planes_mode and N % 8 == 0
        only = (dy_direct and u.x.C % 8 == 0 and self.planes_fit(M, N) and self.planes_fit(u.x.root.M, u.x.root.ld)
                and (not need_dgrad or self.h2_ok(N, u.x.C, kh * kw, dgrad=True)))
        dy, gwork = self.new_dy(u, dy_direct, only)
        u.dz, u.dy = dz, dy
        u.up = None                    # (block_bwd sets it: the unit whose ReLU mask gates `dz` for this unit, unit_bwd's up_mask)
        coef = self.fbuf(4 * N)
        nblk = C.c_int(0)
        self.keep.append(nblk)
        mk = u.mask.data_ptr() if u.mask is not None else None
        relu_eff = u.relu
        if up_mask is not None:
            assert not u.relu and u.drop is None and dres is None
            mk, relu_eff = up_mask.data_ptr(), True
        # The data gradient that wrote dz last can emit this BN's backward sums from its epilogue (DmlConvDesc.bnr_*):
        # one pass over dz / y / mask less.  Conditions: it wrote the whole tensor, bf16 with the 1-bit ReLU mask,
        # no dropout scale, at most 4096 row groups (on the 192 x 192 layers the finalize would fold 9216 groups in two
        # stages, which works, but the fused sums then cost the data gradients more than the stand-alone reduce:
        # 363.5 vs 364.5 images/s).
        if dz_from is not None:
            assert dz is None and dres is None and up_mask is None and u.drop is None and (u.mask is not None or not u.relu)
        prod = self.last_dgrad.get(dz.ptr) if (self.sw.fuse_bn_reduce and dz is not None and u.z is u.z.root and up_mask is None) else None
        # (a stride-2 data gradient issued as four parity-class launches: each writes the sums of its own rows, conv_dgrad_s2_classes)
        prods = prod if isinstance(prod, list) else ([prod] if prod is not None else [])
        prod = prods[0] if prods else None
        prows = lib.dml_conv_stat_rows(C.byref(prod)) if prod is not None else STAT_ROWS      # rows per partial of that launch
        Gs = [(pd.B * pd.Ho * pd.Wo + prows - 1) // prows for pd in prods] if len(prods) > 1 else [(M + prows - 1) // prows]
        G = sum(Gs)
        de, de_w, de_k = dz_from if dz_from is not None else (None, None, 0)
        whole = (prod is not None and (u.mask is not None or not u.relu) and u.drop is None
                 and prod.N == N and prod.ldy == N and dz.ld == N and prod.y == dz.ptr)
        fused = whole and len(prods) == 1 and self.dtype == torch.bfloat16 and N % 8 == 0 and N > 32 and G <= 4096
        # fp32 tensors: the two-plane kernel's epilogue does the same (4-channel mask bytes, 48-row groups, max |g| for dy's bound).
        # Up to 16384 groups since round 5 (the 192 x 192 layers: 12288 groups, folded in two stages by dml_bn_bwd_finalize): with the
        # row epilogue's vector mask loads the fused sums win there too, 83.90 -> 83.60 ms (profiles/r05_ab_bnr_maxg.txt)
        fused = fused or (whole and self.dtype == torch.float32 and prod.f32_split == 2 and prows == 48 and N % 64 == 0
                          and G <= 16384 and u.y.ld % 4 == 0)
        a1 = None
        if fused:
            part = self.fbuf(G * N * 2)
            g0 = 0
            for pd, gc in zip(prods, Gs):
                pd.bnr_y, pd.bnr_mask = u.y.ptr, mk
                pd.bnr_mean, pd.bnr_invstd = u.mean.data_ptr(), u.invstd.data_ptr()
                pd.bnr_partials, pd.bnr_ldy, pd.bnr_relu = part.data_ptr() + g0 * N * 8, u.y.ld, 1 if u.relu else 0
                if gwork is not None:
                    pd.bnr_gmax = gwork.data_ptr()
                g0 += gc
            nblk = C.c_int(G)
            self.keep.append(nblk)
            sp = part.data_ptr()
        elif de is not None:
            sp = self.sp
            self.call(self.bwd, lib.dml_head_bn_bwd_reduce, de.ptr, de_w, u.y.ptr, mk, u.mean.data_ptr(), u.invstd.data_ptr(),
                      self.sp, M, N, de_k, de.C, de.ld, N, u.y.ld, 1 if relu_eff else 0, C.byref(nblk),
                      gwork.data_ptr() if gwork is not None else None)
        else:
            sp = self.sp
            a1 = self.call(self.bwd, lib.dml_bn_bwd_reduce, dz.ptr, u.y.ptr, u.z.ptr, mk, u.mean.data_ptr(),
                           u.invstd.data_ptr(), self.sp, M, N, dz.ld, u.y.ld, u.z.ld, 1 if relu_eff else 0, 1.0,
                           self.dt, C.byref(nblk), gwork.data_ptr() if gwork is not None else None)
        if self.sync and not u.frozen:
            sums = self.dbuf(N * 2)
            self.call(self.bwd, lib.dml_bn_bwd_sums, sp, nblk, N, sums.data_ptr(), st.grad_ptr_of(bn.weight),
                      st.grad_ptr_of(bn.bias))
            grp = self.e.sync_group
            self.py_op(self.bwd, lambda t=sums, g=grp: dist.all_reduce(t, group=g))
            self.call(self.bwd, lib.dml_bn_bwd_coef, sums.data_ptr(), M * self.world, N, bn.weight.data_ptr(),
                      u.mean.data_ptr(), u.invstd.data_ptr(), coef.data_ptr())
            bound_done = False
        else:
            bound_done = self.bn_bwd_finalize(u, sp, nblk, 0 if u.frozen else M, coef, dy, gwork)
        self.mark_grad(bn.weight)
        self.mark_grad(bn.bias)
        pl = self.dy_planes(u, coef, dy, gwork, bound_done)
        if de is not None:
            assert dy_direct
            self.call(self.bwd, lib.dml_head_bn_bwd_apply, de.ptr, de_w, u.y.ptr, mk, coef.data_ptr(), None if only else dy.ptr,
                      M, N, de_k, de.C, de.ld, N, u.y.ld, dy.ld, 1 if relu_eff else 0, *pl)
        else:
            a3 = self.call(self.bwd, lib.dml_bn_bwd_apply, dz.ptr, u.y.ptr, u.z.ptr, mk, coef.data_ptr(),
                           None if only else dy.ptr, dres.ptr if dres is not None else None, M, N, dz.ld, u.y.ld, u.z.ld, dy.ld,
                           dres.ld if dres is not None else 0, 1 if relu_eff else 0, 1.0,
                           1 if dres_accum else 0, self.dt, None if dy_direct else self.amax_of(dy), *pl)
            u.gscale_slots += ([(a1, 13)] if a1 is not None else []) + [(a3, 15)]
        if dres is not None:
            self.last_dgrad.pop(dres.ptr, None)   # written by the BN kernel, not by a data gradient
        self.conv_wgrad(u.x, dy, u.conv, u.Cp)
        if need_dgrad:
            self.conv_dgrad(dy, u.conv, u.wt, u.x, final=final)

    def stem_bwd_fused(self, u: ConvUnit, dp: Act, argmax):
        """Backward of the fused stem (Plan.build, fuse_stem): max pool + BatchNorm backward without d(z0).  Both BatchNorm passes gather
        a pixel's gradient from d(p0) and the argmax bytes and gate it with the stem's ReLU mask -- what dml_maxpool3x3s2_bwd followed by
        unit_bwd computes, bit for bit, partial sums included -- then the weight gradient as in unit_bwd.  dy exists in
        fp32 and / or as planes, whichever the weight gradient reads (conv_wgrad)."""
        lib = self.lib
        N, M, y = u.conv.out_channels, u.y.M, u.y
        planes = u.x.C % 8 == 0 and N % 8 == 0                # conv_wgrad's test: both operands as planes
        only = planes and self.planes_fit(M, N) and self.planes_fit(u.x.root.M, u.x.root.ld)
        dy, gwork = self.new_dy(u, planes, only)
        u.dz, u.dy, u.up = None, dy, None
        coef = self.fbuf(4 * N)
        nblk = C.c_int(0)
        self.keep.append(nblk)
        self.call(self.bwd, lib.dml_stem_bn_bwd_reduce, dp.ptr, argmax.data_ptr(), u.mask.data_ptr(), y.ptr, u.mean.data_ptr(),
                  u.invstd.data_ptr(), self.sp, y.B, y.H, y.W, N, y.ld, C.byref(nblk),
                  gwork.data_ptr() if gwork is not None else None)
        bound_done = self.bn_bwd_finalize(u, self.sp, nblk, M, coef, dy, gwork)       # (never synchronised: Plan.build, fuse_stem)
        pl = self.dy_planes(u, coef, dy, gwork, bound_done)
        self.mark_grad(u.bn.weight)
        self.mark_grad(u.bn.bias)
        self.call(self.bwd, lib.dml_stem_bn_bwd_apply, dp.ptr, argmax.data_ptr(), u.mask.data_ptr(), y.ptr, coef.data_ptr(),
                  None if only else dy.ptr, y.B, y.H, y.W, N, y.ld, dy.ld, *pl)
        self.conv_wgrad(u.x, dy, u.conv, u.Cp)
