"""The engine's DML_* environment switches in one place: the Python twin of csrc/conv_choice.h's ConvSwitches."""
import os
from dataclasses import dataclass, field

# A record reads the environment when it is made: PlanSwitches once per Plan.__init__, EngineSwitches once per Engine.__init__.
# Every switch is an A/B or test lever: the default is the product's path, and the tests run each fallback (tests/test_gpu_model.py,
# PLAN_SWITCHES; tests/test_plan_fingerprint.py).  The library's own switches (DML_CONV_*) are read in csrc/, dmlnet/parallel.py keeps
# the data-parallel ones and DML_LIB_PATH selects the library in dmlnet/_lib.py.


def _on(name):      # a switch that is on unless set to 0
    return field(default_factory=lambda: os.environ.get(name, "1") != "0")


def _int(name, default):
    return field(default_factory=lambda: int(os.environ.get(name, default)))


@dataclass(frozen=True)
class PlanSwitches:
    # f16x2: a batch-statistics BatchNorm writes the fp16 planes of its output (forward) / of dy (backward) itself, scaled
    # from a bound known beforehand (dml_h2_bound_bn): no dml_h2_split pass over those tensors, and no fp32 copy at all where
    # only convolutions read them.  DML_H2_DIRECT=0: every tensor through dml_h2_split (A/B, tests)
    h2_direct: bool = _on("DML_H2_DIRECT")
    fuse_res_grad: bool = _on("DML_FUSE_RES_GRAD")        # conv1's data gradient adds the identity branch's gradient itself (block_bwd)
    # f16x2 training: a block output that only convolutions and the NEXT block's residual add read exists as planes only -- the
    # residual add takes (hi + lo) / s, the value those convolutions see (dml_bn_apply, res_unscale).  DML_RES_PLANES=0: off
    res_planes: bool = _on("DML_RES_PLANES")
    fuse_bn_reduce: bool = _on("DML_FUSE_BN_REDUCE")      # the BN-backward sums from the data gradient's epilogue (unit_bwd)
    # f16x2: the plane-scale bound of a BatchNorm output / of dy computed by the finalize launch's last block instead of a
    # one-block launch of its own behind it (dml_bn_finalize_bound / dml_bn_bwd_finalize_bound).  DML_FUSE_BOUND=0: off (A/B)
    fuse_bound: bool = _on("DML_FUSE_BOUND")
    # f16x2: data gradients of the stride-2 convolutions as stride-1 launches per pixel-parity class (conv_dgrad_s2_classes).
    # DML_S2_CLASSES=0: off (A/B, tests)
    s2_classes: bool = _on("DML_S2_CLASSES")
    bnr_inc: bool = _on("DML_BNR_INC")                    # the 1x1 class launch emits the BN-backward sums of its increment
    # f16x2 training: the stem's BatchNorm + ReLU + max pool as one pass each way (dml_bn_relu_maxpool3x3s2_fwd / dml_stem_bn_bwd_*):
    # z0 and d(z0), 604 MB each at 16 x 384 x 384 x 64, are never written.  DML_FUSE_STEM=0: off (A/B, tests)
    fuse_stem: bool = _on("DML_FUSE_STEM")
    # f16x2 training: the decoder unit's BatchNorm backward forms the embedding conv's data gradient itself (dml_head_bn_bwd_*)
    # instead of reading it back twice from a 604 MB tensor.  DML_FUSE_HEAD_DGRAD=0: off (A/B, tests)
    fuse_head_dgrad: bool = _on("DML_FUSE_HEAD_DGRAD")
    cat_planes: bool = _on("DML_CAT_PLANES")              # the decoder's concat buffer as fp16 planes only (_head_fwd)
    prep_overlap: bool = _on("DML_PREP_OVERLAP")          # weight copies of layer2.. on the side stream (refresh_weights, A/B)
    ds_grad_from_dz: bool = _on("DML_DS_GRAD_FROM_DZ")    # the downsample branch's BN backward reads dz and the ReLU mask (block_bwd, A/B)
    # the stem conv in space-to-depth form (_S2DConv).  "1": every fp32 plan, "0": none, unset: the f16x2 plans
    stem_s2d: str = field(default_factory=lambda: os.environ.get("DML_STEM_S2D", ""))
    # bf16 plans, DML_GRAD_STAGE32=1: a gradient with several producers is summed in fp32 and rounded ONCE by its last
    # producer, as autograd does in the reference (resnet.py:112-113, network/utils.py:360).  Off by default: measured
    # over 10 + 4 seeds (tests/tools/bf16_noise_seeds.py, profiles/r03_bf16_noise_seeds.txt) the per-tensor gradient
    # noise is the same to three digits with a rounding after every producer (median 1 - cos 0.0788 vs 0.0789 at
    # 4 x 256^2, 0.0995 vs 0.0995 at 2 x 768^2; emulation 0.077 / 0.097), while the fp32 staging tensors move 3 GB more
    # per step (41.2 -> 42.0 ms).  The excess noise round 2 attributed to these roundings came from the bf16 rounding
    # of the image-pooling branch's B x C tensors (_head_fwd).
    grad_stage32: bool = field(default_factory=lambda: os.environ.get("DML_GRAD_STAGE32", "0") == "1")
    # bf16 weight copies of the LDS-DMA layers in the tile-major layout (DmlPrepDesc.w_tiled): the weight half of every DMA
    # instruction becomes one contiguous KB (whole cache lines) instead of sixteen 64-byte row segments.  DML_W_TILED=0: off;
    # also off under DML_CONV_V1 (the library's register-staged kernels read the plain layout only)
    tiled_weights: bool = field(default_factory=lambda: os.environ.get("DML_W_TILED", "1") != "0" and os.environ.get("DML_CONV_V1") is None)
    fork_branches: bool = _on("DML_FORK_BRANCHES")        # the ASPP branches of a small inference plan side by side (_head_fwd)
    # DmlConvDesc.ws_min_tiles for every conv of the plan: 0 = the library's rule for its wave-specialised kernel, 1 = take it
    # whenever the shape allows (the GPU tests run the small fixtures through it), 2147483647 = never
    ws_min_tiles: int = _int("DML_WS_MIN_TILES", "0")
    group_wgrad: bool = _on("DML_GROUP_WGRAD")            # weight gradients of consecutive layers in one grouped launch (conv_wgrad)
    # 256 x 256 output tiles per grouped launch.  17 = one layer3 bottleneck (4 + 9 + 4): its three weight gradients
    # share a launch right after its backward, while their operands are still cache-hot.  Larger groups move fewer
    # slabs but start later: whole step 17: 371.0, 34: 369.9, 48: 369.8, ungrouped 370.3 images/s (interleaved runs)
    group_tiles: int = _int("DML_GROUP_TILES", "17")


F32_PRODUCTS = {"exact": 0, "bf16x3": 1, "f16x2": 2}


@dataclass(frozen=True)
class EngineSwitches:
    overlap_wgrad: bool = _on("DML_OVERLAP_WGRAD")        # weight gradients on the side stream (Plan.run_backward)
    native: bool = _on("DML_NATIVE_PLAN")                 # replay launch lists through dml_plan_run
    # fp32 compute dtype only: "bf16x3" products (model.set_compute_dtype(torch.float32, fp32_products="bf16x3"))
    # or "f16x2" (fp32_products="f16x2"): two fp16 planes per operand, three MFMAs per block (DmlConvDesc.x_planes)
    f32_split: int = field(default_factory=lambda: F32_PRODUCTS[os.environ.get("DML_F32_PRODUCTS", "exact").lower()])


def ppm_graph() -> bool:
    """DML_PPM_GRAPH: the body of a pyramid-pooling scale replayed as one hipGraph (PPMEngine._replay_body)"""
    return os.environ.get("DML_PPM_GRAPH", "1") == "1"
