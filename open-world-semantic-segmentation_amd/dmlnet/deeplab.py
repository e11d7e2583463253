"""The DeepLabV3+/ResNet-101 network with its distance heads as a plan: which pieces (dmlnet/plan_pieces.py) in which order."""
# Graph structure follows the reference modules (paths relative to /root/reference/DeepLabV3Plus-Pytorch):
#   backbone  network/backbone/resnet.py:75-115,139-143,171-193   (Bottleneck, stem, stride->dilation)
#   head      network/utils.py:8-32,308-361                       (DeepLabHeadV3Plus, ASPP)
#   distance  network/utils.py:84-118                             (upsample + prototype distances)
import ctypes as C
import itertools

import torch
import torch.nn as nn

from . import _lib
from ._lib import DML_BF16, DML_F32
from .plan_pieces import _PAD_CIN, Act, HeadRec, _S2DConv, root_count
from .store import _round_up


class DeepLabNetwork:
    """`build` and its parts, mixed into dmlnet.engine.Plan beside PlanPieces"""

    def block_fwd(self, x: Act, blk: nn.Module, out_planes_only=False):
        """one Bottleneck (resnet.py:95-115): 1x1 -> 3x3 -> 1x1, + identity or downsample branch, ReLU.
        out_planes_only: the block output is read by planes convolutions and the next block's residual add only (build())."""
        # (f16x2: u1.z / u2.z feed one convolution each -- where that one reads planes, the fp32 tensors are never written)
        n1, n2, n3 = blk.conv1.out_channels, blk.conv2.out_channels, blk.conv3.out_channels
        kk = blk.conv2.kernel_size[0] * blk.conv2.kernel_size[1]
        u1 = self.cbr(x, blk.conv1, blk.bn1, planes_only=self.h2_ok(n1, n2, kk))
        u2 = self.cbr(u1.z, blk.conv2, blk.bn2, planes_only=self.h2_ok(n2, n3, 1))
        ud = None
        if blk.downsample is not None:
            ud = self.cbr(x, blk.downsample[0], blk.downsample[1], relu=False)
            idt = ud.z
        else:
            idt = x
        u3 = self.cbr(u2.z, blk.conv3, blk.bn3, relu=True, res=idt, planes_only=out_planes_only)
        return (x, u1, u2, u3, ud)

    def block_bwd(self, rec):
        """backward of block_fwd: consumes d(block output), produces d(block input)"""
        xb, u1, u2, u3, ud = rec
        dz = self.grad_of(u3.z)
        ud_from_dz = False
        if ud is not None:
            # The downsample branch's output gradient is the block output's gradient under the block's ReLU mask.  Instead of having
            # bn3's backward apply write that copy (4 bytes per element of the block output: 1.4 GB per step over the four blocks) the
            # branch's BN backward reads dz and the mask itself (unit_bwd, up_mask)
            ud_from_dz = (self.sw.ds_grad_from_dz and u3.relu and u3.mask is not None and u3.drop is None and not ud.relu
                          and ud.drop is None and ud.z is ud.z.root and ud.conv.out_channels == u3.conv.out_channels)
            if ud_from_dz:
                self.unit_bwd(u3, dz, dres=None)
            else:
                dres = self.grad_of(ud.z)
                self.unit_bwd(u3, dz, dres=dres, dres_accum=False)
                ud.z.grad_init = True
        elif (self.sw.fuse_res_grad and not xb.root.grad_init and xb is xb.root
              and u3.relu and u3.mask is not None and u3.drop is None and xb.C % 8 == 0 and xb.C > 32
              and dz.ld == xb.C and self.conv_geom(u1.conv, xb)[:3] == (1, 1, 1)
              and (self.dtype == torch.bfloat16
                   # f16x2: conv1's data gradient on the two-plane kernel takes res_* too.  (Round 4 measured this as a LOSS, 183.5 ->
                   # 179.0 images/s: the row epilogue fetched its ReLU masks with one byte load per lane and four rows, a third of
                   # its memory instructions.  With the masks of a sub-tile in one 16-byte load per row, conv_epilogue_rows, it wins:
                   # 187.6 -> 190.1 images/s, three interleaved rounds, profiles/r05_ab_maskvec_res.txt; without the fusion that
                   # change alone is +0.3 %.)  DML_FUSE_RES_GRAD=0: off
                   or (self.sw.h2_direct and self.h2_ok(u1.conv.out_channels, xb.C, 1, dgrad=True) and xb.C % 64 == 0
                       and self.planes_fit(u1.y.M, u1.conv.out_channels)))):
            # The masked output gradient is this block's contribution to d(xb) through the identity branch.  Instead
            # of having the BN-backward apply write that copy (75 MB per layer3 block) for conv1's data gradient to
            # accumulate onto, conv1's data gradient reads dz and the mask itself (DmlConvDesc.res_*).
            self.unit_bwd(u3, dz, dres=None)
            self.res_src[id(xb)] = (dz, u3.mask)
        else:
            dres = self.grad_of(xb)
            self.unit_bwd(u3, dz, dres=dres, dres_accum=xb.root.grad_init)
            xb.root.grad_init = True
        self.unit_bwd(u2, self.grad_of(u2.z))
        self.unit_bwd(u1, self.grad_of(u1.z), final=ud is None)
        assert not self.res_src, "conv1's data gradient did not take the identity-branch gradient"
        if ud is not None:
            if ud_from_dz:
                self.unit_bwd(ud, dz, up_mask=u3.mask)
                ud.up = u3
            else:
                self.unit_bwd(ud, self.grad_of(ud.z))

    # ---- the network -------------------------------------------------------------------------
    def build(self):
        lib, m, st = self.lib, self.e.model, self.e.store
        B, H, W = self.B, self.H, self.W
        bb, head_modules = m.backbone, self.e.head_modules()[:self.predict_heads]       # (None: every head)
        n_fixed = 0
        for mod in itertools.chain(bb.modules(), *[h.modules() for h in head_modules]):
            if isinstance(mod, nn.BatchNorm2d):
                if mod.training and not self.training:
                    raise NotImplementedError("a BatchNorm2d in train() mode inside an eval() model is not supported")
                n_fixed += 0 if mod.training else 1

        self.begin_forward(bn_eval_table=n_fixed > 0)
        # input packing NCHW fp32 -> NHWC (8 ch); f16x2 plans: space-to-depth, [B][H/2][W/2][12], and the stem conv in that form
        # (_S2DConv).  The same products in another summation order: the exact-fp32 and three-term modes keep the 7x7 stride-2 form
        # on 8 channels so that their results stay what they were (DML_STEM_S2D=1: every fp32 plan, =0: none)
        stem_conv = bb.conv1
        s2d_on = self.sw.stem_s2d == "1" or (self.sw.stem_s2d != "0" and self.f32_split == 2)
        if self.dtype == torch.float32 and s2d_on and _S2DConv.fits(bb.conv1, H, W):
            x_in = self.new(B, H // 2, W // 2, 4 * bb.conv1.in_channels)
            self.images_args = self.call(self.fwd, lib.dml_pack_input_s2d, 0, x_in.ptr, B, bb.conv1.in_channels, H, W)
            stem_conv = _S2DConv(bb.conv1, H // 2, W // 2)
        else:
            x_in = self.new(B, H, W, _PAD_CIN)
            self.images_args = self.call(self.fwd, lib.dml_pack_input, 0, x_in.ptr, B, 3, H, W, _PAD_CIN, self.dt)

        # stem: 7x7 s2 conv + BN + ReLU, 3x3 s2 max pool (resnet.py:139-143,196-199)
        Hs, Ws = self.conv_geom(stem_conv, x_in)[5:]
        Hp, Wp = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
        # f16x2 training: BatchNorm + ReLU + max pool in ONE pass over y (dml_bn_relu_maxpool3x3s2_fwd).  z0 is never written; the kernel
        # also collects max |p0|, so the split of p0 needs no maximum pass and scales its planes exactly as before (the step's results
        # do not move by a bit); the stem's ReLU mask is still written (38 MB: the backward's gate, Plan.stem_bwd_fused)
        fuse_stem = (self.sw.fuse_stem and self.training and self.planes_mode and not self.sync
                     and bb.bn1.training and stem_conv.out_channels == 64)
        stem = self.cbr(x_in, stem_conv, bb.bn1, need_dgrad=False, pool_fused=fuse_stem)
        amax = torch.empty(B * Hp * Wp * 64, dtype=torch.uint8, device=self.device) if self.training else None
        self.keep.append(amax)
        p0 = self.new(B, Hp, Wp, 64)
        if fuse_stem:
            self.call(self.fwd, lib.dml_bn_relu_maxpool3x3s2_fwd, stem.y.ptr, stem.scale.data_ptr(), stem.shift.data_ptr(),
                      stem.mean.data_ptr(), p0.ptr, amax.data_ptr(), stem.mask.data_ptr(), None, 0, None, self.amax_of(p0),
                      B, Hs, Ws, 64, stem.y.ld)
        else:
            z0 = stem.z
            self.call(self.fwd, lib.dml_maxpool3x3s2_fwd, z0.ptr, p0.ptr, amax.data_ptr() if amax is not None else None,
                      B, z0.H, z0.W, 64, self.dt)

        # bottlenecks (resnet.py:95-115)
        blocks = []
        x = p0
        seq = [(li, blk) for li, layer in enumerate((bb.layer1, bb.layer2, bb.layer3, bb.layer4)) for blk in layer]
        self.prep_cut = None
        for i, (li, blk) in enumerate(seq):
            if li == 1 and self.prep_cut is None:
                # everything from layer2 on reads weight copies that refresh_weights prepares on the side stream, under the stem and
                # layer1 (Plan.refresh_weights, overlap): ops before this index only need the copies made so far
                self.prep_cut = (len(self.fwd), len(self.prep), len(self.prep_h2))
            # the output as planes only: another block follows whose conv1 / downsample conv take planes, and it is neither `low`
            # (the decoder's 48-channel projection reads the fp32 tensor) nor `out` (global average pooling does)
            nxt = seq[i + 1] if i + 1 < len(seq) else None
            c3 = blk.conv3.out_channels
            po = (self.sw.res_planes and nxt is not None and not (li == 0 and nxt[0] != 0)
                  and nxt[1].conv1.kernel_size == (1, 1) and self.h2_ok(c3, nxt[1].conv1.out_channels, 1)
                  and (nxt[1].downsample is None or self.h2_ok(c3, nxt[1].downsample[0].out_channels, 1)))
            blocks.append(self.block_fwd(x, blk, out_planes_only=po))
            x = blocks[-1][3].z
            if li == 0 and (nxt is None or nxt[0] != 0):
                low = x
        out = x

        # heads: one for the DMLNet model, several (shared backbone) for the self-distillation model (utils.py:120-193)
        self.heads = [self._head_fwd(h, low, out) for h in head_modules]
        self.K, self.Kp = self.heads[0].K, self.heads[0].Kp
        if self.predict_heads is not None:
            # head i > 0 contributes its own last prototype, class K_i - 1 (16 + (i - 1) for the reference's head widths,
            # test_self_distillation.py:295-297)
            tab = (_lib.PredictHead * len(self.heads))(*[
                _lib.PredictHead(rec.emb.ptr, rec.Kp, rec.K, rec.emb.ld, rec.K - 1) for rec in self.heads])
            self.keep.append(tab)
            self.predict_args = self.call(self.fwd, lib.dml_incremental_predict, C.addressof(tab), len(self.heads), 0, None,
                                          B, self.heads[0].emb.H, self.heads[0].emb.W, H, W)
        self.end_forward()
        if self.training and n_fixed:
            self.nbt_inc = torch.tensor([1 if mod.training else 0 for mod in st.bn_modules], dtype=torch.int64,
                                        device=self.device)
        if not self.training:
            return

        # ------------------------------------------------------------------ backward
        # The LAST head goes first: it initialises d(out) / d(low); the others accumulate into them, so their
        # segments of the plan can be skipped when the loss does not reach them (Engine.backward).
        self.head_bwd_range = {}
        self.to_backbone_ops = []
        # gradients with several producers: d(out) (pooled term + four ASPP data gradients per head), d(low) (decoder
        # projection + layer2.0's conv1 and downsample), and the input of every other block with a downsample branch
        self.stage_grad32(out)
        self.stage_grad32(low)
        for (xb, u1, u2, u3, ud) in blocks:
            if ud is not None:
                self.stage_grad32(xb)
        for hi in reversed(range(len(self.heads))):
            start = len(self.bwd)
            self._head_bwd(self.heads[hi], low, out)
            self.flush_wgrad()                          # a head's segment may be skipped as a whole: keep its jobs inside
            self.head_bwd_range[hi] = (start, len(self.bwd))
        # bottlenecks in reverse (this whole segment, and the head ops that only feed it, are skipped when no backbone
        # parameter requires a gradient: the reference's incremental recipe trains one new head on a fixed trunk,
        # main_self_distillation.py:352-357)
        backbone_start = len(self.bwd)
        if out.g32 is not None and len(self.heads) > 1:
            self.round_staged(out)                      # several heads: which of them runs last is only known per step
        for rec in reversed(blocks):
            self.block_bwd(rec)
        # max pool + stem
        if fuse_stem:
            self.stem_bwd_fused(stem, self.grad_of(p0), amax)
        else:
            dz0 = self.grad_of(z0)
            self.call(self.bwd, lib.dml_maxpool3x3s2_bwd, self.grad_of(p0).ptr, amax.data_ptr(), dz0.ptr, B, z0.H, z0.W,
                      64, self.dt)
            self.unit_bwd(stem, dz0, need_dgrad=False)
        self.flush_wgrad()
        self.backbone_bwd_range = (backbone_start, len(self.bwd))
        for a, args, i in self.direct_planes:       # planes nobody reads (outputs that only feed resizes / concats): not written
            if not a.h2_used:
                args[i] = None

    def _head_fwd(self, head: nn.Module, low: Act, out: Act):
        """DeepLabHeadV3Plus + final upsample + distance head (network/utils.py:8-32,84-118) on the backbone features."""
        lib = self.lib
        B, H, W = self.B, self.H, self.W
        K = head.classifier[3].out_channels
        Kp = _round_up(K, 8)           # embedding channels are carried padded to 16-byte vectors (zeros beyond K)
        if Kp > 32:
            raise NotImplementedError("num_classes=%d: the distance-head kernels hold at most 32 embedding channels and 33 "
                                      "prototypes; the reference's drivers use 16 (main_embedding.py:336)" % K)
        cat2_c = _round_up(48 + 256, 32)                   # 304 -> 320: K tiles of 32 stay inside one tap
        # f16x2 training: the concat buffer exists as fp16 planes only.  Its two producers -- the low-level projection's BatchNorm and
        # the bilinear resize of the ASPP projection -- write their channel slices of the planes themselves, with ONE scale from the
        # larger of the two BatchNorms' bounds (known from gamma / beta / count alone: dml_h2_bound_bn_multi at the head of the
        # forward); the amax + split passes of dml_h2_split over this 755 MB tensor (16 x 768 x 768) are gone.  DML_CAT_PLANES=0: off
        cat_planes = (self.training and self.planes_mode and self.sw.h2_direct and self.sw.cat_planes
                      and head.project[1].training and head.aspp.project[1].training
                      and not self.sync and self.planes_fit(B * low.H * low.W, cat2_c))
        if cat_planes:
            cat2 = self.h2_direct(B, low.H, low.W, cat2_c, fp32_too=False)
            cat2.h2[0].zero_()                              # (the 16 pad channels stay zero: nobody writes them)
            pdrop = float(head.aspp.project[3].p) if isinstance(head.aspp.project[3], nn.Dropout) else 0.0
            tab = (_lib.H2BoundDesc * 2)(
                _lib.H2BoundDesc(head.project[1].weight.data_ptr(), head.project[1].bias.data_ptr(), None, 48,
                                 root_count(B * low.H * low.W * self.world), 1.0, 0),
                _lib.H2BoundDesc(head.aspp.project[1].weight.data_ptr(), head.aspp.project[1].bias.data_ptr(), None, 256,
                                 root_count(B * out.H * out.W * self.world), 1.0 / (1.0 - pdrop) if pdrop < 1.0 else 1.0, 0))
            self.cat_bound_table = self.device_table(tab)
            self.keep.append(self.cat_bound_table)
            self.call(self.fwd, lib.dml_h2_bound_bn_multi, self.cat_bound_table.data_ptr(), 2, cat2.h2[1].data_ptr())
        else:
            cat2 = self.new(B, low.H, low.W, cat2_c, zero=True)
        up_low = self.cbr(low, head.project[0], head.project[1], out=cat2.slice(0, 48))
        aspp = head.aspp
        cat1 = self.new(B, out.H, out.W, 5 * 256)
        branches = []
        # f16x2: the planes of `out` are shared by all four conv branches.  h2_of appends a tensor's split at its FIRST consumer,
        # which would be branch 0 -- inside the first fork range of an inference plan (run_forward: every range on its own
        # stream, each waiting for the main stream only), so branches 1-3 would read planes and the unscale word that
        # branch 0's stream is still writing.  Issue the split here, on the main stream, before the fork point.
        if self.h2_ok(out.C, aspp.convs[0][0].out_channels, 1):
            self.h2_of(out, self.fwd)
        marks = [len(self.fwd)]
        for i in range(4):
            branches.append(self.cbr(out, aspp.convs[i][0], aspp.convs[i][1], out=cat1.slice(256 * i, 256)))
            marks.append(len(self.fwd))
        # image-pooling branch (network/utils.py:318-329): avg-pool -> 1x1 -> BN -> ReLU -> broadcast
        pool_f32 = self.training and self.dtype == torch.bfloat16
        with self.precision(torch.float32 if pool_f32 else self.dtype):
            # bf16 training: this BatchNorm sees B samples per channel.  When two of them are within bf16 resolution of each other the
            # rounded pre-normalisation values collapse, 1/sigma goes to 1/sqrt(eps) and the layer's backward -- whose two
            # correction terms cancel its output gradient almost exactly -- returns a spurious gradient hundreds of times
            # too large that the broadcast spreads over every pixel of d(out) (measured at 768 x 768, 2 images: layer4's
            # bn3 gradients 20x their true norm).  The unit is B x 256 values: it runs in fp32 storage, and so do its
            # input (the pooled features) and its output gradient -- B x C numbers whose sample-to-sample DIFFERENCES
            # decide 1/sigma and the cancellation (dml_reduce_hw_f32); only its output is rounded for the bf16 concat.
            pooled = self.new(B, 1, 1, out.C)
            if pool_f32:
                self.call(self.fwd, lib.dml_reduce_hw_f32, out.ptr, pooled.ptr, B, out.H * out.W, out.C, out.ld, DML_BF16,
                          1.0 / (out.H * out.W))
            else:
                self.call(self.fwd, lib.dml_global_avgpool_fwd, out.ptr, pooled.ptr, B, out.H * out.W, out.C, out.ld, self.dt)
            upool = self.cbr(pooled, aspp.convs[4][1], aspp.convs[4][2])
        pool_z = upool.z
        if pool_f32:
            pool_z = self.new(B, 1, 1, 256)
            self.call(self.fwd, lib.dml_convert_dtype, upool.z.ptr, pool_z.ptr, B * 256, DML_F32, DML_BF16)
        self.call(self.fwd, lib.dml_broadcast_hw, pool_z.ptr, cat1.slice(1024, 256).ptr, B, out.H * out.W, 256,
                  cat1.ld, self.dt)
        marks.append(len(self.fwd))
        if not self.training and self.sw.fork_branches and (out.M + 127) // 128 * 2 < 300:
            # inference on small maps (a branch's grid below ~300 workgroups; 1024 x 2048 at batch 1: 270 vs 261
            # images/s, at batch 4 the grids fill the chip alone and forking costs 1.5 %): the five branches only read
            # `out` and write disjoint channel slices of cat1 (one launch each, the pooled one three) -- independent, so
            # they may overlap (training keeps them in line: its units share the statistics scratch)
            if not hasattr(self, "fwd_forks"):
                self.fwd_forks = []
            # nothing inside a fork range may write a tensor another range reads: the only shared input is `out` (split above)
            assert not any(fn is lib.dml_h2_split and args[0] == out.root.ptr for fn, args in self.fwd[marks[0]:marks[5]]), \
                "the split of the fork's shared input must run before the fork point"
            self.fwd_forks.append([(marks[k], marks[k + 1]) for k in range(5)])
        uproj = self.cbr(cat1, aspp.project[0], aspp.project[1], drop=aspp.project[3])
        up_slice = cat2.slice(48, 256)
        if cat_planes:
            pp, pstride, punscale = self.h2_of(up_slice, self.fwd)
            self.call(self.fwd, lib.dml_bilinear_fwd_planes, uproj.z.ptr, pp, pstride, cat2.ld, punscale, B, out.H, out.W, low.H, low.W,
                      256, uproj.z.ld)
        else:
            self.call(self.fwd, lib.dml_bilinear_fwd, uproj.z.ptr, up_slice.ptr, B, out.H, out.W, low.H, low.W, 256,
                      uproj.z.ld, cat2.ld, self.dt, 0, 0)
        ucls = self.cbr(cat2, head.classifier[0], head.classifier[1])
        fin = head.classifier[3]
        if Kp == K:
            w_fin, wt_fin = self.prep_weight(fin, 256, self.training)
            fin_bias_ptr = fin.bias.data_ptr() if fin.bias is not None else None
        else:
            w_fin, wt_fin, fin_bias_ptr = self.padded_final_conv(fin, K, Kp, self.training)
        emb = self.new(B, low.H, low.W, Kp, f32=True)
        self.conv_fwd(ucls.z, fin, emb, w_fin, None, bias_ptr=fin_bias_ptr, N=Kp)
        protos = self.e.prototypes_padded(K, Kp)
        # fused final upsample + distance head (network/utils.py:88-118); outputs are per-call tensors
        # (a prediction plan stops at the embedding: Plan.build appends one launch for all heads)
        head_args = None
        if self.predict_heads is None:
            head_args = self.call(self.fwd, lib.dml_upsample_dist_fwd, emb.ptr, protos.data_ptr(), 0, 0,
                                       None, None, B, emb.H, emb.W, Kp, K, H, W)
        rec = HeadRec()
        rec.K, rec.Kp, rec.emb, rec.protos, rec.head_args = K, Kp, emb, protos, head_args
        rec.cat1, rec.cat2, rec.up_low, rec.branches, rec.pooled, rec.upool = cat1, cat2, up_low, branches, pooled, upool
        rec.pool_f32 = pool_f32
        rec.uproj, rec.ucls, rec.fin, rec.wt_fin = uproj, ucls, fin, wt_fin
        rec.head_bwd_args, rec.df, rec.feats_p = None, None, None
        return rec

    def _head_bwd(self, rec, low: Act, out: Act):
        lib, st = self.lib, self.e.store
        B, H, W = self.B, self.H, self.W
        K, Kp, emb, fin, wt_fin = rec.K, rec.Kp, rec.emb, rec.fin, rec.wt_fin
        cat1, cat2, up_low, branches, pooled, upool = rec.cat1, rec.cat2, rec.up_low, rec.branches, rec.pooled, rec.upool
        uproj, ucls = rec.uproj, rec.ucls
        df = self.fbuf(B * H * W * Kp)
        rec.df = df
        de = self.new(B, emb.H, emb.W, Kp)
        rec.de = de                     # gradient of the low-resolution embedding
        # Two ways from d(loss)/d(logits) to the low-resolution embedding gradient `de`; Engine.backward skips one.
        # (1) the loss handed over a deferred gradient (dmlnet/lazy_grad.py) and the shape is the fused kernel's (16
        #     prototypes, exact x4 upsample): loss gradient + distance gradient + transposed upsample in one pass;
        # (2) anything else: distance gradient into `df`, then the transposed upsample.
        rec.fused_args, rec.fused_range = None, None
        if Kp == 16 and K == 16 and H == 4 * emb.H and W == 4 * emb.W:
            i0 = len(self.bwd)
            rec.fused_args = self.call(self.bwd, lib.dml_head_bwd_fused, 0, 0, 0, 0, rec.protos.data_ptr(), de.ptr, B,
                                       emb.H, emb.W, Kp, K, H, W, 255, 0.0, 1.0, self.dt)
            rec.fused_range = (i0, i0 + 1)
        i1 = len(self.bwd)
        rec.head_bwd_args = self.call(self.bwd, lib.dml_proto_dist_bwd, 0, None, 0, rec.protos.data_ptr(),
                                       df.data_ptr(), B, Kp, K, H, W)
        self.call(self.bwd, lib.dml_bilinear_bwd, df.data_ptr(), de.ptr, B, emb.H, emb.W, H, W, Kp, Kp, Kp, self.dt, 1, 0)
        rec.unfused_range = (i1, i1 + 2)
        if fin.bias is not None:
            bws = self.fbuf(1024 * Kp)          # per-workgroup partial sums: a fixed-order (reproducible) bias gradient
            if Kp == K:
                self.call(self.bwd, lib.dml_bias_grad_ws, de.ptr, st.grad_ptr_of(fin.bias), de.M, K, de.ld, self.dt,
                          bws.data_ptr(), bws.numel())
            else:
                gb = self.fbuf(Kp)
                self.call(self.bwd, lib.dml_fill_f32, gb.data_ptr(), Kp, 0.0)
                self.call(self.bwd, lib.dml_bias_grad_ws, de.ptr, gb.data_ptr(), de.M, Kp, de.ld, self.dt, bws.data_ptr(),
                          bws.numel())
                self.call(self.bwd, lib.dml_unpad_wgrad, gb.data_ptr(), st.grad_ptr_of(fin.bias), 1, 1, K, Kp)
            self.mark_grad(fin.bias)
        self.conv_wgrad(ucls.z, de, fin, 256, pad_rows=Kp)
        # f16x2 training: d(ucls.z) = de . W is a rank-K product -- the unit's two BatchNorm-backward passes form it from `de` (38 MB) and
        # the conv's master weight instead of reading a 604 MB tensor twice that a data-gradient launch wrote
        if (self.sw.fuse_head_dgrad and self.planes_mode and not self.sync and self.sw.h2_direct
                and ucls.dtype == self.dtype and ucls.z is ucls.z.root and ucls.drop is None and (ucls.mask is not None or not ucls.relu)
                and fin.kernel_size == (1, 1) and fin.stride == (1, 1) and fin.weight.dtype == torch.float32
                and fin.in_channels == ucls.conv.out_channels and fin.in_channels % 8 == 0 and Kp in (8, 16, 24, 32)):
            self.unit_bwd(ucls, None, dz_from=(de, fin.weight.data_ptr(), K))          # -> d cat2
        else:
            self.conv_dgrad(de, fin, wt_fin, ucls.z)
            self.unit_bwd(ucls, self.grad_of(ucls.z))                   # -> d cat2
        dcat2 = self.grad_of(cat2)
        # upsample branch -> d(aspp output)
        dproj = self.grad_of(uproj.z)
        self.call(self.bwd, lib.dml_bilinear_bwd, dcat2.slice(48, 256).ptr, dproj.ptr, B, out.H, out.W, low.H, low.W,
                  256, dcat2.ld, dproj.ld, self.dt, 0, 0)
        uproj.z.grad_init = True
        self.unit_bwd(uproj, dproj)                                      # -> d cat1
        dcat1 = self.grad_of(cat1)
        # pooling branch
        staged = out.g32 is not None
        assert rec.pool_f32 or not staged
        with self.precision(torch.float32 if rec.pool_f32 else self.dtype):      # (pool_f32: the unit lives in fp32 storage, _head_fwd)
            dzp = self.new(B, 1, 1, 256)
            if rec.pool_f32:
                self.call(self.bwd, lib.dml_reduce_hw_f32, dcat1.slice(1024, 256).ptr, dzp.ptr, B, out.H * out.W, 256,
                          dcat1.ld, DML_BF16, 1.0)
            else:
                self.call(self.bwd, lib.dml_reduce_hw, dcat1.slice(1024, 256).ptr, dzp.ptr, B, out.H * out.W, 256, dcat1.ld,
                          self.dt)
            self.unit_bwd(upool, dzp)                                    # -> d pooled (fp32 where the unit is)
            gp = self.grad_of(pooled)
        if rec.pool_f32 and not staged:
            gp32, gp = gp, self.new(B, 1, 1, out.C)
            self.call(self.bwd, lib.dml_convert_dtype, gp32.ptr, gp.ptr, B * out.C, DML_F32, DML_BF16)
        feeders = self.to_backbone_ops                 # backward ops whose only product is d(out) / d(low)
        # The image-pooling branch contributes dv / HW to every pixel of d(out): far below half an ulp of the other four
        # branches' sum in bf16.  It goes in FIRST (while the buffer is still untouched), so that the data gradients
        # accumulate onto it in fp32 before the rounding and the term survives on average; a later head's segment finds
        # the buffer initialised and adds.
        first = not out.root.grad_init
        # (staged: into the fp32 staging tensor, stage_grad32 -- the last ASPP data gradient rounds the sum once)
        dst, dt = (out.g32, DML_F32) if staged else (self.grad_of(out), self.dt)
        self.call(self.bwd, lib.dml_avgpool_bwd_set if first else lib.dml_avgpool_bwd_add, gp.ptr, dst.ptr, B,
                  out.H * out.W, out.C, dst.ld, dt)
        out.root.grad_init = True
        feeders.append(len(self.bwd) - 1)
        for i in range(4):
            self.unit_bwd(branches[i], dcat1.slice(256 * i, 256), final=(i == 3 and len(self.heads) == 1))   # -> d out
            feeders.append(len(self.bwd) - 1)           # unit_bwd ends with the data gradient
        self.last_dgrad.pop(self.grad_of(out).ptr, None)      # several writers: layer4's last BN keeps its own reduce
        # low-level projection -> d low (layer1 output)
        self.unit_bwd(up_low, dcat2.slice(0, 48), final=False)          # layer2.0's data gradients follow
        feeders.append(len(self.bwd) - 1)
