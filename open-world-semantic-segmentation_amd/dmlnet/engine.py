"""Static-plan executor for DeepLabV3+/ResNet-101 + distance head on MI355X.

One `Plan` per (batch, H, W, dtype, training) holds every activation / gradient buffer (NHWC, sized once:
288 GB of HBM makes recomputation or buffer reuse unnecessary at 768x768 bs=16) and two flat lists of
pre-bound C-ABI calls -- forward and backward -- that are replayed each step on the caller's current HIP
stream.  PyTorch only supplies device memory, streams and the autograd hook; every FLOP runs in
libdmlnet_hip.so.  This module is the import surface; one concern per module behind it ("The engine's modules").
"""
# store.py        ParamStore: parameters, gradients and momentum in flat buffers
# launch_list.py  BoundArgs / NativeList: the packed op lists dml_plan_run replays
# switches.py     the DML_* environment switches, read in one place
# plan_pieces.py  PlanPieces: buffers, fp16 planes, conv lowering, the conv + BatchNorm unit both ways
# deeplab.py      DeepLabNetwork: the network as a sequence of those pieces (build, block_*, _head_*)
# replay.py       Replay: weight refresh and the replay of a built plan
import weakref
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib, lazy_grad
from .deeplab import DeepLabNetwork
from .launch_list import BoundArgs, NativeList, _pack_word  # noqa: F401  (re-exported)
from .plan_pieces import _PAD_CIN, Act, ConvUnit, HeadRec, PlanPieces, _S2DConv  # noqa: F401  (re-exported)
from .replay import Replay
from .store import ParamStore, _round_up  # noqa: F401  (re-exported)
from .switches import EngineSwitches


class Plan(DeepLabNetwork, Replay, PlanPieces):
    """One (batch, H, W, dtype, training) of a model: PlanPieces.__init__ allocates and calls build(), which subclasses replace."""
    # (engine_ppm.PPMPlan, the tests' plans of one block or one head; bench.py, tests and tools patch attributes of THIS class)

    def _exec(self, ops, stream, start=0, stop=None, hook=None, skip_ranges=(), side_stream=None):
        """Issue ops[start:stop] in order: natively, unless the engine is told to stay in Python or Plan.run has been replaced."""
        # (bench.py's profiled pass replaces it.  The test is on the class Plan itself, not type(self): the tests' PiecePlan overrides
        # `run` as an instance method with another meaning)
        stop = len(ops) if stop is None else stop
        if not self.e.native or Plan.run is not Plan._py_run:
            return self._exec_python(Plan.run, ops, stream, start, stop, hook, skip_ranges, side_stream)
        return self._exec_native(ops, stream, start, stop, hook, skip_ranges, side_stream)


class Engine:
    """Owns the parameter store and the plan cache of one model instance."""

    plan_cls = Plan

    def __init__(self, model: nn.Module):
        self.model = model
        self.lib = _lib.load()
        self.store = ParamStore(model)
        self.plans = {}
        self._protos = {}
        self.reducer = None             # parallel.GradReducer, attached for multi-GPU runs
        # starting values from the environment (EngineSwitches); set_compute_dtype, bench.py and the tests assign them afterwards
        sw = EngineSwitches()
        self.overlap_wgrad, self.native, self.f32_split = sw.overlap_wgrad, sw.native, sw.f32_split
        self.sync_bn, self.sync_group = False, None     # synchronised BatchNorm statistics over the process group
        self._side, self._branch = {}, {}       # side stream / branch streams per device
        self.step_count = 0
        self.seed = 0x5DEECE66D

    def rank_seed(self) -> int:
        """dropout seed of this rank: the reference's DataParallel replicas draw independent masks per sample
        (network/utils.py:354 under main_embedding.py:425), so the data-parallel ranks must not share one"""
        rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
        return (self.seed ^ (rank * 0xD1B54A32D192ED03)) & 0xFFFFFFFFFFFFFFFF

    def side_stream(self, device):
        if device not in self._side:
            # (stream priorities were tried: this runtime offers {normal, high} only, and neither a high-priority main
            # stream nor a high-priority side stream changed the step time -- tools/ab_bench.sh)
            self._side[device] = torch.cuda.Stream(device=device)
        return self._side[device]

    def branch_streams(self, device, n):
        pool = self._branch.setdefault(device, [])
        while len(pool) < n:
            pool.append(torch.cuda.Stream(device=device))
        return pool[:n]

    def prototypes(self, k: int) -> torch.Tensor:
        """centers = 3 * I_K (network/utils.py:103-106); built once per device instead of every forward."""
        dev = self.store.flat_p.device
        key = (k, dev)
        if key not in self._protos:
            self._protos[key] = 3.0 * torch.eye(k, dtype=torch.float32, device=dev)
        return self._protos[key]

    def head_modules(self):
        m = self.model
        return m.head_modules() if hasattr(m, "head_modules") else [m.classifier]

    def prototypes_padded(self, k: int, kp: int) -> torch.Tensor:
        """the same centers with the embedding axis zero-padded to kp (kernels' view; see Plan.build)"""
        if kp == k:
            return self.prototypes(k)
        dev = self.store.flat_p.device
        key = (k, kp, dev)
        if key not in self._protos:
            m = torch.zeros((k, kp), dtype=torch.float32, device=dev)
            m[:, :k] = self.prototypes(k)
            self._protos[key] = m
        return self._protos[key]

    def bn_modes(self) -> int:
        """Bit i set = the i-th BatchNorm2d normalises with its running statistics (module in eval()) -- part of the
        plan key, because a training plan is built around each layer's mode."""
        sig = 0
        for i, m in enumerate(self.store.bn_modules):
            if not m.training:
                sig |= 1 << i
        return sig

    def plan_for(self, x: torch.Tensor, dtype: torch.dtype, training: bool, predict_heads=None) -> Plan:
        if not self.store.is_bound(x.device):
            self.store.bind(x.device)
            self.plans.clear()
            self._protos.clear()
        B, Cin, H, W = x.shape
        key = (B, H, W, dtype, training, bool(self.sync_bn), self.bn_modes() if training else 0, int(self.f32_split))
        if predict_heads is not None:
            # a plan of its own: the inference plan behind model(x) keeps its launch list, buffers and results
            key += ("predict", int(predict_heads))
        plan = self.plans.get(key)
        if plan is None:
            plan = self.plans[key] = self.plan_cls(self, B, H, W, dtype, training,
                                                   predict_heads=None if predict_heads is None else int(predict_heads))
        return plan

    def predict(self, x: torch.Tensor, dtype: torch.dtype, n_heads: int) -> torch.Tensor:
        """Merged prediction [B,H,W] int64 of heads 0 .. n_heads-1 (test_self_distillation.py:292-297 of the reference; one
        head: its argmax) through the prediction plan: no logits or features at full resolution."""
        self._check_input(x)
        if not 1 <= n_heads <= min(len(self.head_modules()), _lib.PREDICT_MAX_HEADS):
            raise ValueError("predict over %d heads: the model has %d, one launch merges at most %d"
                             % (n_heads, len(self.head_modules()), _lib.PREDICT_MAX_HEADS))
        x = x.contiguous().float()
        plan = self.plan_for(x, dtype, False, predict_heads=n_heads)
        if getattr(plan, "predict_args", None) is None:
            raise NotImplementedError("%s has no prediction plan" % type(plan).__name__)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        plan.refresh_weights(stream, overlap=False)
        B, _, H, W = x.shape
        preds = torch.empty((B, H, W), dtype=torch.int64, device=x.device)
        plan.predict_args[2] = preds.data_ptr()
        plan.images_args[0] = x.data_ptr()
        plan.run_forward(stream)
        plan.last_input = x
        return preds

    @staticmethod
    def _check_input(x: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("DMLNet HIP engine needs a ROCm device tensor (got %s); the CPU restatement lives "
                               "in oracle/ and is test infrastructure only" % x.device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected input [B,3,H,W], got %s" % (tuple(x.shape),))

    def forward(self, x: torch.Tensor, dtype: torch.dtype, training: bool):
        self._check_input(x)
        synced = bool(self.sync_bn and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.sync_group) > 1)
        x = x.contiguous().float()
        plan = self.plan_for(x, dtype, training)
        if training and x.shape[0] < 2 and not synced:
            for u in plan.units:
                if u.bn.training and u.y.M < 2:
                    # same failure as the reference: a batch-statistics BatchNorm over one value per channel -- at batch 1 the
                    # one of ASPPPooling (network/utils.py:318-329), unless it runs on its running statistics (eval())
                    # (synchronised statistics span the ranks: one image per rank is a legal batch there)
                    raise ValueError("Expected more than 1 value per channel when training, got input size "
                                     "torch.Size([%d, %d, %d, %d])" % (u.y.B, u.bn.num_features, u.y.H, u.y.W))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        plan.refresh_weights(stream, overlap=training)
        B, _, H, W = x.shape
        logits, feats = [], []
        for rec in plan.heads:
            # a deferred loss gradient of this head's PREVIOUS forward that never reached backward() (the loss was dropped,
            # or a second forward ran first) is void now: its features buffer is about to be replaced
            lazy_grad.drop_for(rec.logits_ref() if getattr(rec, "logits_ref", None) is not None else None)
            lg = torch.empty((B, rec.K, H, W), dtype=torch.float32, device=x.device)
            ft = torch.empty((B, H, W, rec.Kp), dtype=torch.float32, device=x.device)
            # The plan must not own the tensors it hands out: returned from the autograd node they carry its grad_fn, whose context
            # holds model and plan -- a cycle through C++ objects the garbage collector cannot see, and every dropped model would
            # keep its plans (tens of GB at the benchmark size) for the life of the process.  An alias without autograd identity
            # (same storage, same version counter) for the features, a weak reference for the identity test on the logits.
            rec.feats_p = ft.detach()        # the kernels' (channel-padded) features; the backward reads them again
            rec.feats_version = None
            rec.logits_ref = weakref.ref(lg)
            rec.head_args[2], rec.head_args[3] = lg.data_ptr(), ft.data_ptr()
            logits.append(lg)
            feats.append(ft)
        plan.images_args[0] = x.data_ptr()
        if training:
            for args, idx, bn in plan.momentum_slots:
                if bn.momentum is None:
                    raise NotImplementedError("BatchNorm2d(momentum=None) is not supported")
                args[idx] = float(bn.momentum)
            self.step_count += 1
            for u in plan.drop_units:
                p = float(u.drop.p) if u.drop.training else 0.0      # F14: dropout module in eval() => off
                u.apply_args[14] = p
                u.apply_args[15] = (self.rank_seed() + 0x9E3779B97F4A7C15 * self.step_count) & 0xFFFFFFFFFFFFFFFF
                for (a, i) in u.gscale_slots:
                    a[i] = 1.0 / (1.0 - p) if p > 0 else 1.0
            if plan.nbt_inc is None:
                self.store.flat_nbt.add_(1)
            else:
                self.store.flat_nbt.add_(plan.nbt_inc)      # layers with fixed statistics do not count the batch
        plan.run_forward(stream)
        plan.last_input = x
        for hi, rec in enumerate(plan.heads):
            rec.feats_version = rec.feats_p._version
            if rec.Kp != rec.K:             # features_out has exactly num_classes channels (utils.py:95-97)
                feats[hi] = feats[hi][..., :rec.K].contiguous()
        return plan, logits, feats

    def backward(self, plan: Plan, glogits: List[Optional[torch.Tensor]], gfeats: List[Optional[torch.Tensor]]):
        """glogits / gfeats: one entry per head (None where the loss does not reach that output)."""
        dev = plan.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        keep, skip = [], []
        last = len(plan.heads) - 1
        for hi, rec in enumerate(plan.heads):
            gl, gf = glogits[hi], gfeats[hi]
            if gl is None and gf is None and hi != last:
                skip.append(plan.head_bwd_range[hi])         # accumulating segment: nothing to add
                continue
            lazy = lazy_grad.take(gl)
            if lazy is not None and (lazy.logits is not rec.logits_ref()
                                     or tuple(lazy.logits.shape) != (plan.B, rec.K, plan.H, plan.W)):
                # the marker belongs to another forward of this plan than the one whose activations it holds now (a second
                # train-mode forward ran before this backward): the stored tensors are not the ones the loss saw
                raise RuntimeError("backward through logits of an earlier forward: the plan's activations were replaced by "
                                   "a later forward of the same shape (run backward before the next forward)")
            if lazy is not None and rec.fused_args is not None and gf is None and rec.feats_p._version == rec.feats_version:
                # deferred loss gradient + a shape the fused kernel covers: one pass, no d(loss)/d(logits) tensor (the kernel
                # recomputes the logits from the features handed to the user: an in-place edit of those since the forward
                # sends the step down the materialising path below, which uses the logits the loss saw)
                a = rec.fused_args
                a[0], a[1], a[2], a[3] = rec.feats_p.data_ptr(), lazy.labels.data_ptr(), lazy.sums.data_ptr(), lazy.gout.data_ptr()
                a[13], a[14], a[15] = int(lazy.ignore_index), float(lazy.alpha), float(lazy.n_images)
                skip.append(rec.unfused_range)
                keep += [lazy]
                continue
            if lazy is not None:                             # deferred, but not fusable here: materialise it
                gl = torch.empty((plan.B, rec.K, plan.H, plan.W), dtype=torch.float32, device=dev)
                _lib.check(self.lib.dml_loss_bwd(lazy.logits.data_ptr(), lazy.labels.data_ptr(), lazy.sums.data_ptr(),
                                                 lazy.gout.data_ptr(), gl.data_ptr(), plan.B, rec.K, plan.H, plan.W,
                                                 int(lazy.ignore_index), float(lazy.alpha), float(lazy.n_images), stream),
                           "dml_loss_bwd")
            elif gl is not None and lazy_grad.outstanding_for(rec.logits_ref()):
                lazy_grad.drop_for(rec.logits_ref())
                raise RuntimeError("the loss was built with fused_backward=True but the logits have another consumer: its "
                                   "gradient was added to the deferred-gradient marker.  Construct the loss with "
                                   "fused_backward=False")
            if rec.fused_range is not None:
                skip.append(rec.fused_range)
            if gl is None:
                gl = torch.zeros((plan.B, rec.K, plan.H, plan.W), dtype=torch.float32, device=dev)
            gl = gl.contiguous()
            if gf is not None:
                gf = gf.contiguous()
                if rec.Kp != rec.K:
                    gp = torch.zeros((plan.B, plan.H, plan.W, rec.Kp), dtype=torch.float32, device=dev)
                    gp[..., :rec.K] = gf
                    gf = gp
            a = rec.head_bwd_args
            a[0] = gl.data_ptr()
            a[1] = gf.data_ptr() if gf is not None else None
            a[2] = rec.feats_p.data_ptr()
            keep += [gl, gf]
        self._keep_bwd = keep
        if not any(p.requires_grad for p in self.model.backbone.parameters()):
            skip.append(plan.backbone_bwd_range)
            skip += [(i, i + 1) for i in plan.to_backbone_ops]
        plan.skip_ranges = skip
        state = self.store.begin_backward()
        if self.reducer is not None:
            if state == "accumulate" and self.reducer.world > 1:
                # the bucketed all-reduce works in place on the flat gradient: a second backward without zero_grad()
                # would sum the already reduced gradients over the ranks again (x world), unlike the single-GPU path
                raise RuntimeError("gradient accumulation over several backward passes is not supported with the "
                                   "data-parallel reducer attached: call optimizer.zero_grad() (set_to_none=True) "
                                   "before every backward")
            self.reducer.run_backward(plan, stream)
        else:
            plan.run_backward()
        self.store.end_backward()
