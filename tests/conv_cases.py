"""Case table shared by tests/test_conv_refs.py (CPU) and tests/test_gpu_conv_edges.py (GPU): the forward and data-gradient
convolution of include/dmlnet_hip.h (dml_conv_igemm, mode 0 and mode 1) with its epilogues as a plain numpy definition, the seeded
inputs, the error bars and the cases.  A plain module (no fixtures, no hooks, numpy only); nothing here looks at a kernel's output or
imports the library.  Written the way tests/wgrad_cases.py is, whose split emulations (x3_terms, h2_terms) it re-uses.

The contract, in float64 -- np.pad, strided slices and tensordot (conv_fwd, conv_dgrad), never a kernel's index arithmetic:
  forward (mode 0)   y[b,yo,xo,n] = sum over (r,s,c) of x[b, yo stride - pad + r dil, xo stride - pad_x + s dil, c] w[n,r,s,c], 0 outside
                     the image; then  + bias[n];  stats[g][n] = (sum, M2 about the group's own mean) over every dml_conv_stat_rows() rows;
                     y_f32: a float tensor whatever the dtype;  post_*: act((y - post_mean) post_scale + post_shift [+ post_res])
  data gradient (1)  the launch's x is dY [B,Hi,Wi,C] on the grid of the forward OUTPUT, its w the transposed copy wt[N = Cin][R][S][C = Cout],
                     its y is dX [B,Ho,Wo,N]:  dX[b,p,q,n] = sum over (i,j,r,s,c) with p = i stride - pad + r dil, q = j stride - pad_x + s dil
                     of dY[b,i,j,c] wt[n,r,s,c];  then accum (+ the value y held), acc32 (+ an fp32 staging tensor), res_dz under res_mask,
                     bnr_*: partials (sum g, sum g (bnr_y - mean) invstd) per dml_conv_stat_rows() rows, g = the STORED y under the mask bit --
                     with bnr_inc and accum, g = this launch's own share;  sub_grid: the rows (b, y2, x2) of the launch are the pixels
                     (b, 2 y2 + sub_y, 2 x2 + sub_x) of y and of every epilogue operand (parity_classes: the four launches of a 3 x 3
                     stride-2 data gradient written into one tensor ARE the stride-2 data gradient).

Roundings the contract allows, read in csrc/conv_device.h (conv_epilogue) and csrc/conv_ws.h (conv_epilogue_rows_ops): bias, the value
y held (accum), acc32, res_dz, post_res are each added to the fp32 accumulator in fp32 -- one fp32 rounding per operand -- and a bf16
output is rounded ONCE from that fp32 total (pack_bf16x2 / f32_to_bf16 as the last step; accum reads the bf16 y back as a float first).
The inference epilogue is (acc - mean) * scale + shift, then + res, then the ReLU: three roundings, or two where the compiler contracts.
An fp32 output of an exact case therefore EQUALS the float64 value, a bf16 output its round-to-nearest-even bf16 value.

Two kinds of input, as in wgrad_cases.
  exact  x and w integers in [-3, 3]; bias, residuals, acc32, the old y, res_dz and bnr_y integers in [-8, 8]; bnr_mean / post_mean / post_shift
         integers, bnr_invstd / post_scale powers of two in {1/2, 1, 2}.  Every product is an integer, every partial sum in any order an
         integer (or, after a scale of 1/2, a half-integer) below 2^24: 9 Ktot + |extras| < 2^24 is asserted for every case (EXTRA_MAX).
         The operands are exact in bf16, in the three-term split (mid = lo = 0) and in the two fp16 planes (s = 2^13, lo = 0; the unscale by
         2^-26 is exact).  The sum half of stats and both halves of bnr_partials are exact as well; M2 is not (the group mean is not).
         x3_mid (kind x3): x, w = a + b 2^-8, a in {+-2, +-3}, b = +-1, the channels from 24 on zero: hi = a, mid = b 2^-8, lo = 0; all nine
         products are kept or zero, multiples of 2^-16, at most 24 of them non-zero per output: |partial sums| < 24 * 9.05 < 2^8 -- exact.
         h2_lo (kind planes): x, w = a + b 2^-12, a in {+-2, +-3}, |b| in {1, 2, 3} with the sign of a (|x| stays in a's binade):
         s = t = 2^13, s x = a 2^13 + 2 b, hi = a 2^13 (a multiple of the fp16 spacing 16 of [2^14, 2^15), |2 b| < 8 = half of it),
         lo = 2 b exactly.  The kernel keeps hi hi + hi lo + lo hi: multiples of 2^14 below Ktot * 9.1 * 2^26 < 2^38 for Ktot <= 256 -- exact in fp32 in any order -- and drops lo lo = 4 b b', so the expected
         value is sum a a' + (a b' + b a') 2^-12 and NOT the float64 convolution, from which it differs by sum b b' 2^-24 (h2_lo_dropped).
  real   seeded Gaussians (rounded to bf16 for the bf16 cases), "scaled": activations times 1e3, weights times 1e-3.  Per output element
             bar = (c 2^-24 + r) (sum |x w| + |extras|)  [+ for a bf16 output its one final rounding: 2^-9 of the upper end of the value's
             binade, half a bf16 spacing (bf16_half_ulp) -- 2^-9 of the value itself only at the top of a binade, 2^-8 at its bottom]
         c = conv_chain(case), counted from the code: 32 per K step (K steps = R S C / 32, or ceil(R S C / 32) where C % 32 != 0 and the
         steps straddle taps; steps of padding-only taps the two-plane kernel skips are counted), the K-split tail's q parts, one per
         epilogue operand added (bias, accum, acc32, res_dz: 1; post: 3 + post_res).  r = 0 for operands used as stored (bf16, exact fp32
         MFMA), R_X3 and R_H2 exactly as wgrad_cases derives them.  The M2 half of stats: m2_bar, derived from the kernel's formula
         (the group's sum in fp32, mean = sum * (1 / cnt), M2 = sum of (v - mean)^2 over the group).
         No bar is measured on a kernel.  The GPU file prints the largest measured share of each bar.

Buffers (built by the GPU file): x, y, post_res, res_dz, bnr_y and acc32 are channel slices of wider buffers, pitch ld = C + 8 (ld_extra),
at offset 0 ("first") or ld - C ("last": the slice's last row ends the allocation; 8 elements keep every 16-byte alignment the header asks
for); input neighbours hold NaN, output neighbours and -- without accum -- the whole old y the 0xAA sentinel; the planes come from dml_h2_split
on the slice with ldp = ld, and from layout 1 for the weights.

The case table.  A row: id, kind (bf16 | f32 | x3 | planes), mode, (B, H, W, C, N) -- H x W the INPUT grid of the forward convolution, which is
the launch's input in mode 0 and its output in mode 1; C the K side, N the output side of the launch -- k or (R, S), stride, dil, pad, the
epilogue set, and EXPECT[id] = (kernel as tests/tools/conv_choice_dump.cpp prints it, grid, nblk_m, nblk_n, tail_q, statistics rows) for
the library's default switches (v1, bm256, ws) = (0, 1, 0); ws=True sets ws_min_tiles = 1 and w_tiled = 1 (the bf16 persistent kernel).
tests/test_conv_refs.py asks csrc/conv_choice.h for every row: a case that stops reaching its kernel fails there, without a GPU.
A two-plane descriptor with more than 32 taps (planes_7x7): the code runs the exact fp32 MFMA kernel where C % 32 != 0 or N <= 32, the
three-term split otherwise; the row here (C = 8) pins conv_igemm_kernel<f32,64,0,0>.

Out of scope, named: instantiations that need an environment switch read at load time (bf16 on the register-staged kernel with BN 64 / 128
aligned: DML_CONV_V1; forced 256-row tiles: DML_CONV_BM256=2; tests/test_gpu_conv_dma.py runs them in processes of their own), the K-split
tail of the 256-row tile (its smallest shape costs about 4e10 multiply-adds in float64), operands of 2^31 bytes.
"""
import numpy as np

from bn_cases import EPS32, F32, F64, bf16_round, h2_planes, pack_mask  # noqa: F401  (re-exported)
from wgrad_cases import R_H2, R_X3, h2_terms, x3_terms  # noqa: F401  (re-exported)

BK = 32
INT32_MAX = 2 ** 31 - 1
EUNSUPPORTED = -3
EXTRA_MAX = 64                      # bound on |extras| of the exact inputs (8 per operand, scaled by at most 2, summed)
LD_EXTRA = 8

EPIS = {"bias", "stats", "y_f32", "post", "post_res", "post_relu", "accum", "acc32", "res", "bnr", "bnr_relu", "bnr_inc"}


class Case:
    def __init__(self, cid, kind, mode, shape, k, stride=1, dil=1, pad=None, epi=(), ws=False, tail=False, scaled=False, special=None,
                 sub=None, pad_w=None, planes_only=False, rc=0):
        self.id, self.kind, self.mode, self.ws, self.tail, self.scaled, self.special = cid, kind, mode, ws, tail, scaled, special
        self.B, H, W, self.C, self.N = shape
        self.R, self.S = (k, k) if isinstance(k, int) else k
        self.stride, self.dil = stride, dil
        self.pad = dil * (self.R // 2) if pad is None else pad
        self.pad_x = (dil * (self.S // 2) if pad is None else pad) if pad_w is None else pad_w
        self.pad_w_set = pad_w is not None
        self.epi = frozenset(epi)
        assert self.epi <= EPIS, self.epi - EPIS
        self.sub, self.planes_only, self.rc = sub, planes_only, rc
        Hc = (H + 2 * self.pad - dil * (self.R - 1) - 1) // stride + 1
        Wc = (W + self.pad + self.pad_x - dil * (self.S - 1) - 1) // stride + 1 if pad_w is None else None
        if sub is not None:             # a parity class: stride-1 geometry on dY's grid (H x W), y has 2 H x 2 W pixels
            self.Hi, self.Wi, self.Ho, self.Wo = H, W, H, W
        elif mode == 0:
            self.Hi, self.Wi, self.Ho, self.Wo = H, W, Hc, Wc
        else:
            self.Hi, self.Wi, self.Ho, self.Wo = Hc, Wc, H, W
        self.M = self.B * self.Ho * self.Wo                    # rows of the launch
        self.Mx = self.B * self.Hi * self.Wi
        self.My = 4 * self.M if sub is not None else self.M    # rows of y and of the epilogue operands
        self.Ktot = self.R * self.S * self.C
        self.ldx, self.ldy = self.C + LD_EXTRA, self.N + LD_EXTRA
        self.dtype = "bf16" if kind == "bf16" else "f32"
        self.out_dtype = "f32" if (self.dtype == "f32" or "y_f32" in self.epi) else "bf16"
        self.vec = 8 if self.dtype == "bf16" else 4                 # channels per mask byte
        assert 9 * self.Ktot + EXTRA_MAX < 2 ** 24
        assert self.C <= self.ldx and self.N <= self.ldy

    def __repr__(self):
        return self.id

    @property
    def expect(self):
        return EXPECT[self.id]

    @property
    def kernel(self):
        return EXPECT[self.id][0]

    @property
    def stat_rows(self):
        return EXPECT[self.id][5]

    @property
    def tail_q(self):
        return EXPECT[self.id][4]

    def geometry(self):
        return (self.mode if self.sub is None else 1, self.B, self.Hi, self.Wi, self.C, self.Ho, self.Wo, self.N, self.R, self.S, self.stride,
                self.dil, self.pad, self.pad_x)

    def offsets(self, place):
        return (0, 0) if place == "first" else (self.ldx - self.C, self.ldy - self.N)

    def desc(self):
        """the descriptor as tests/test_conv_choice.py's table writes one (a pointer: 0 = null, 16 + its low four address bits)"""
        e = self.epi
        d = dict(x=16, w=16, y=16, B=self.B, Hi=self.Hi, Wi=self.Wi, C=self.C, ldx=self.ldx, Ho=self.Ho, Wo=self.Wo, N=self.N, ldy=self.ldy,
                 R=self.R, S=self.S, stride=self.stride, dil=self.dil, pad=self.pad, dtype=1 if self.kind == "bf16" else 0,
                 y_f32=int("y_f32" in e), accum=int("accum" in e), mode=self.mode,
                 f32_split={"bf16": 0, "f32": 0, "x3": 1, "planes": 2}[self.kind])
        if "bias" in e:
            d["bias"] = 16
        if "stats" in e:
            d["stats"] = 16
        if "post" in e:
            d.update(post_scale=16, post_shift=16, post_mean=16, post_relu=int("post_relu" in e))
            if "post_res" in e:
                d.update(post_res=16, post_ldres=self.ldy)
        if "acc32" in e:
            d.update(acc32=16, acc32_ld=self.ldy)
        if "res" in e:
            d.update(res_dz=16, res_mask=16, res_ld=self.ldy)
        if "bnr" in e:
            d.update(bnr_y=16, bnr_mean=16, bnr_invstd=16, bnr_partials=16, bnr_ldy=self.ldy, bnr_relu=int("bnr_relu" in e),
                     bnr_mask=16 if "bnr_relu" in e else 0, bnr_inc=int("bnr_inc" in e))
        if self.tail:
            d.update(tail_ws=16, tail_ws_elems=TAIL_WS_ELEMS, tail_counters=16, tail_counters_len=TAIL_COUNTERS)
        if self.ws:
            d.update(w_tiled=1, ws_min_tiles=1)
        if self.kind == "planes":
            d.update(x_planes=16, w_planes=16, x_unscale=16, w_unscale=16, x_plane_stride=self.Mx * self.ldx, w_plane_stride=self.N * self.Ktot)
            if self.planes_only:
                d["x_is_planes"] = 1
        if self.sub is not None:
            d.update(sub_grid=1, sub_y=self.sub[0], sub_x=self.sub[1])
        if self.pad_w_set:
            d.update(pad_w_set=1, pad_w=self.pad_x)
        return d


TAIL_WS_ELEMS = 8 * 8 * 128 * 128            # floats: 8 tail tiles of 128 x 128, up to 8 parts each
TAIL_COUNTERS = 128

WRAP_144 = (1, 97, 96, 32, 1024)
S2 = (2, 23, 19, 128, 128)
SMALL = (2, 9, 7, 64, 64)

CASES = [
    # --- two planes, forward ---------------------------------------------------------------------------------------------------------
    Case("pl_fwd_wrap48", "planes", 0, (1, 120, 121, 32, 256), 1, epi={"stats"}),          # 303 tiles of 48 rows on 256 workgroups, M % 48 = 24
    Case("pl_fwd_wrap144", "planes", 0, WRAP_144, 1, epi={"stats"}),                        # 65 x 4 tiles of 144 rows, one K step per tile
    Case("pl_fwd_wrap192", "planes", 0, (1, 222, 222, 64, 64), 1, epi={"stats"}),          # 257 tiles of 192 rows
    Case("pl_fwd_n320", "planes", 0, (2, 17, 21, 96, 320), 3, epi={"stats"}, scaled=True),  # half-empty last column block, C = 96
    Case("pl_fwd_n192", "planes", 0, (2, 15, 14, 64, 192), 3, epi={"bias"}),
    Case("pl_fwd_5x5", "planes", 0, (1, 9, 7, 32, 64), 5, epi={"stats"}),                   # 25 taps, a single partial tile
    Case("pl_fwd_post", "planes", 0, (2, 9, 7, 64, 256), 1, epi={"post", "post_res", "post_relu"}),
    Case("pl_fwd_pad_only", "planes", 0, (2, 5, 6, 64, 256), 3, dil=7),                     # 8 of 9 taps only ever see padding
    Case("pl_fwd_w1", "planes", 0, (3, 50, 1, 64, 256), 3, epi={"stats"}),                  # W = 1; batch boundaries inside the 48-row tiles
    Case("pl_fwd_h2_lo", "planes", 0, (2, 9, 7, 64, 64), 1, special="h2_lo"),
    # --- two planes, data gradient ---------------------------------------------------------------------------------------------------
    Case("pl_dg_wrap144", "planes", 1, (1, 97, 96, 64, 1024), 1),                           # 260 tiles, Ktot = 64: the two-stage minimum
    Case("pl_dg_3x3_n64", "planes", 1, (2, 15, 14, 64, 64), 3, scaled=True),
    Case("pl_dg_n64_accum", "planes", 1, (2, 15, 14, 64, 64), 3, epi={"accum"}),
    Case("pl_dg_n64_bnr", "planes", 1, (2, 15, 14, 64, 64), 3, epi={"bnr", "bnr_relu"}),
    Case("pl_dg_n64_bnr_res", "planes", 1, (2, 15, 14, 64, 64), 3, epi={"bnr", "bnr_relu", "res"}),
    Case("pl_dg_s2", "planes", 1, S2, 3, stride=2),                                         # odd image under stride 2, epi 0
    Case("pl_dg_s2_accum", "planes", 1, S2, 3, stride=2, epi={"accum"}),                    # epi 1
    Case("pl_dg_s2_bnr", "planes", 1, S2, 3, stride=2, epi={"bnr"}),                        # epi 2, no ReLU mask
    Case("pl_dg_s2_bnr_res", "planes", 1, S2, 3, stride=2, epi={"bnr", "bnr_relu", "res"}),  # epi 3
    Case("pl_dg_s2_bnr_inc", "planes", 1, S2, 3, stride=2, epi={"bnr", "bnr_relu", "accum", "bnr_inc"}),
    Case("pl_dg_n1024_res", "planes", 1, (2, 9, 7, 64, 1024), 1, epi={"res"}),
    Case("pl_dg_n1024_bnr", "planes", 1, (2, 9, 7, 64, 1024), 1, epi={"bnr", "bnr_relu"}),
    Case("pl_dg_n1024_bnr_acc", "planes", 1, (2, 9, 7, 64, 1024), 1, epi={"bnr", "bnr_relu", "accum"}),
    Case("pl_dg_k32_falls_to_x3", "planes", 1, (1, 20, 20, 32, 256), 1),                   # Ktot = 32: the three-term kernel
    Case("pl_dg_k32_planes_only", "planes", 1, (1, 20, 20, 32, 256), 1, planes_only=True, rc=EUNSUPPORTED),
    Case("planes_7x7", "planes", 0, (2, 33, 27, 8, 64), 7, stride=2),                      # 49 taps: the exact fp32 kernel (C % 32 != 0)
    # --- bf16: ring, persistent, register-staged -------------------------------------------------------------------------------------
    Case("ring_fwd_n64", "bf16", 0, (2, 11, 13, 64, 64), 3, epi={"stats"}, scaled=True),    # grid 3
    Case("ring_dg_n64", "bf16", 1, (2, 11, 13, 64, 64), 3, epi={"accum"}),
    Case("ring_fwd_n256", "bf16", 0, (2, 11, 13, 64, 256), 3, epi={"bias", "y_f32"}),       # grid 12: narrow, grid % 8 != 0
    Case("ring_dg_n256", "bf16", 1, (2, 11, 13, 64, 256), 3, epi={"bnr", "bnr_relu", "res"}),
    Case("ring_dg_n256_acc32", "bf16", 1, (2, 11, 13, 64, 256), 3, epi={"acc32"}),          # mode 2 on BN 64
    Case("ring_fwd_bn128", "bf16", 0, (1, 160, 161, 32, 128), 1, epi={"stats"}),            # grid 202, M % 128 = 32
    Case("ring_dg_bn128", "bf16", 1, (1, 160, 161, 32, 128), 1, epi={"bnr", "bnr_relu"}),
    Case("ring_dg_bn128_acc32", "bf16", 1, (1, 160, 161, 32, 128), 1, epi={"acc32"}),
    Case("ring_fwd_post", "bf16", 0, (2, 11, 13, 64, 256), 1, epi={"post", "post_res", "post_relu"}),
    Case("ring_fwd_256rows", "bf16", 0, (1, 57, 57, 512, 1024), 3, epi={"stats"}),          # 256-row tiles by the default rule, M % 256 = 177
    Case("ring_dg_256rows", "bf16", 1, (1, 57, 57, 512, 1024), 3, epi={"bnr", "bnr_relu"}),
    Case("ring_dg_256rows_acc32", "bf16", 1, (1, 57, 57, 512, 1024), 3, epi={"acc32"}),
    Case("ring_fwd_tail", "bf16", 0, (1, 64, 65, 128, 1024), 3, epi={"stats"}, tail=True),  # 264 tiles, tail_q = 6
    Case("ring_dg_tail", "bf16", 1, (1, 64, 65, 128, 1024), 3, tail=True),
    Case("ring_fwd_pad_only", "bf16", 0, (2, 5, 6, 64, 64), 3, dil=7),
    Case("ring_fwd_h1", "bf16", 0, (3, 1, 50, 64, 64), 3, epi={"stats"}),                   # H = 1; batch boundaries inside the 128-row tile
    Case("ws_fwd_wrap144", "bf16", 0, WRAP_144, 1, epi={"stats"}, ws=True),                # 260 tiles on 256 workgroups, 48-row groups
    Case("ws_fwd_wrap288", "bf16", 0, (1, 272, 272, 32, 128), 1, epi={"stats"}, ws=True),  # 257 tiles of 288 rows
    Case("ws_dg_wrap144", "bf16", 1, WRAP_144, 1, epi={"bnr", "bnr_relu"}, ws=True),
    Case("ws_dg_n128", "bf16", 1, (2, 11, 13, 64, 128), 3, epi={"accum"}, ws=True),
    Case("ws_dg_n256_acc32", "bf16", 1, (2, 11, 13, 64, 256), 3, epi={"acc32"}, ws=True),
    Case("ws_dg_n128_acc32", "bf16", 1, (2, 11, 13, 64, 128), 3, epi={"acc32"}, ws=True),
    Case("reg_bf16_n32", "bf16", 0, (2, 9, 7, 64, 32), 1, epi={"bias"}),
    Case("reg_bf16_n32_dg", "bf16", 1, (2, 9, 7, 64, 32), 1, epi={"accum"}),
    Case("reg_bf16_c40", "bf16", 0, (2, 9, 7, 40, 96), 3, epi={"stats"}, scaled=True),      # C % 32 != 0
    Case("reg_bf16_c40_dg", "bf16", 1, (2, 9, 7, 40, 96), 3),
    Case("reg_bf16_c40_n64", "bf16", 0, (2, 9, 7, 40, 64), 3, epi={"bias", "y_f32"}),
    Case("reg_bf16_c40_n64_dg", "bf16", 1, (2, 9, 7, 40, 64), 3, epi={"accum"}),
    Case("reg_bf16_c40_n24", "bf16", 0, (2, 9, 7, 40, 24), 3, epi={"stats"}),
    Case("reg_bf16_c40_n24_dg", "bf16", 1, (2, 9, 7, 40, 24), 3),
    # --- fp32: the exact MFMA -----------------------------------------------------------------------------------------------------------
    Case("f32_n128", "f32", 0, (2, 9, 7, 64, 128), 3, epi={"stats"}, scaled=True),
    Case("f32_n128_dg", "f32", 1, (2, 9, 7, 64, 128), 3, epi={"accum"}),
    Case("f32_n64", "f32", 0, SMALL, 3, epi={"post", "post_relu"}),
    Case("f32_n64_dg", "f32", 1, SMALL, 3),
    Case("f32_n32", "f32", 0, (2, 9, 7, 64, 32), 3, epi={"bias"}),
    Case("f32_n32_dg", "f32", 1, (2, 9, 7, 64, 32), 3),
    Case("f32_c12_n24", "f32", 0, (2, 9, 7, 12, 24), 3, epi={"stats"}),
    Case("f32_c12_n24_dg", "f32", 1, (2, 9, 7, 12, 24), 3, epi={"accum"}),
    Case("f32_stem", "f32", 0, (2, 33, 27, 8, 64), 7, stride=2, epi={"stats"}),
    Case("f32_stem_dg", "f32", 1, (2, 33, 27, 8, 64), 7, stride=2),
    Case("f32_c12_n136", "f32", 0, (2, 9, 7, 12, 136), 3, epi={"bias"}),
    Case("f32_c12_n136_dg", "f32", 1, (2, 9, 7, 12, 136), 3),
    Case("f32_pad_only", "f32", 0, (2, 5, 6, 64, 64), 3, dil=7),
    Case("f32_w1", "f32", 0, (3, 50, 1, 64, 64), 3, epi={"stats"}),
    # --- fp32: the three-term split ---------------------------------------------------------------------------------------------------
    Case("x3_n64", "x3", 0, SMALL, 3, epi={"stats"}, scaled=True),
    Case("x3_n64_dg", "x3", 1, SMALL, 3, epi={"accum"}),
    Case("x3_n320", "x3", 0, (2, 9, 7, 64, 320), 3, epi={"bias"}),
    Case("x3_n320_dg", "x3", 1, (2, 9, 7, 64, 320), 3),
    Case("x3_mid", "x3", 0, (2, 9, 7, 32, 64), 1, special="x3_mid"),
    Case("x3_pad_only", "x3", 0, (2, 5, 6, 64, 64), 3, dil=7),
    Case("x3_h1", "x3", 0, (3, 1, 50, 64, 64), 3),
    # --- M one row past and one row short of a multiple of every row tile: 48, 128, 144, 192, 256, 288 -----------------------------
    Case("m49_tile48", "planes", 0, (1, 7, 7, 32, 256), 1, epi={"stats"}),
    Case("m47_tile48", "planes", 0, (1, 1, 47, 32, 256), 1, epi={"stats"}),
    Case("m129_tile128", "bf16", 0, (1, 3, 43, 64, 64), 3, epi={"stats"}),
    Case("m127_tile128", "bf16", 1, (1, 1, 127, 64, 64), 3, epi={"bnr", "bnr_relu"}),
    Case("m145_tile144", "planes", 1, (1, 5, 29, 64, 256), 3, epi={"bnr", "bnr_relu"}),
    Case("m143_tile144", "planes", 1, (1, 11, 13, 64, 256), 3, epi={"accum"}),
    Case("m193_tile192", "planes", 0, (1, 1, 193, 64, 64), 3, epi={"stats"}),
    Case("m191_tile192", "planes", 1, (1, 1, 191, 64, 64), 3, epi={"bnr", "bnr_relu", "res"}),
    Case("m3329_tile256", "bf16", 0, (1, 1, 3329, 512, 1024), 3, epi={"stats"}),
    Case("m3327_tile256", "bf16", 0, (1, 1, 3327, 512, 1024), 3, epi={"bias"}),
    Case("m289_tile288", "bf16", 0, (1, 17, 17, 32, 128), 3, epi={"stats"}, ws=True),
    Case("m287_tile288", "bf16", 1, (1, 7, 41, 32, 128), 3, epi={"bnr", "bnr_relu"}, ws=True),
    # the epilogue's byte-load mask path: a wave tile of 64 channels that is not whole inside N
    Case("ring_dg_n96_bnr_res", "bf16", 1, (2, 11, 13, 64, 96), 3, epi={"bnr", "bnr_relu", "res"}),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the four parity classes of the data gradient of a 3 x 3 stride-2 pad-1 convolution, dY on a 12 x 10 grid, dX on 24 x 20
SUB_PARENT = Case("pl_dg_s2_even", "planes", 1, (2, 24, 20, 128, 128), 3, stride=2, epi={"accum"})


def parity_classes(parent=SUB_PARENT, epi=("accum",)):
    """[(case, rows of the filter, columns of the filter)] of a 3 x 3 stride-2 data gradient: class (cy, cx) sees the taps whose row / column
    has the parity of cy + pad / cx + pad, as a stride-1 launch with padding (cy + pad - first tap) / 2"""
    out = []
    for cy in (0, 1):
        for cx in (0, 1):
            rs = [r for r in range(parent.R) if (r - cy - parent.pad) % 2 == 0]
            ss = [s for s in range(parent.S) if (s - cx - parent.pad_x) % 2 == 0]
            c = Case("pl_dg_sub%d%d" % (cy, cx), "planes", 1, (parent.B, parent.Hi, parent.Wi, parent.C, parent.N), (len(rs), len(ss)),
                     pad=(cy + parent.pad - rs[0]) // 2, pad_w=(cx + parent.pad_x - ss[0]) // 2, sub=(cy, cx), epi=epi)
            out.append((c, rs, ss))
    return out


SUB_CASES = [c for c, _, _ in parity_classes()]

P_W48, P_W144, P_N64, P_NARROW = "conv_ws_kernel<1,4,%d,3,2,3,%d>", "conv_ws_kernel<1,4,%d,3,2,9,%d>", "conv_ws_kernel<4,1,%d,3,2,3,%d>", \
    "conv_ws_kernel<2,2,%d,3,2,9,%d>"
RING64, RING128, RING256 = "conv_igemm_dma_kernel<64,%d,3,3,128,64>", "conv_igemm_dma_kernel<128,%d,3,3,128,64>", \
    "conv_igemm_dma_kernel<128,%d,3,2,256,128>"
WS144, WS288 = "conv_ws_kernel<1,4,%d,3,1,9,0>", "conv_ws_kernel<2,2,%d,3,1,9,0>"
REG, X3K = "conv_igemm_kernel<%s,%d,%d,%d>", "conv_igemm_x3_kernel<%d,%d>"

# (kernel, grid, nblk_m, nblk_n, tail_q, statistics rows) -- asserted against csrc/conv_choice.h by tests/test_conv_refs.py
EXPECT = {
    "pl_fwd_wrap48": ("conv_ws_kernel<1,4,0,3,2,3,0>", 256, 303, 1, 1, 48),
    "pl_fwd_wrap144": ("conv_ws_kernel<1,4,0,3,2,9,0>", 256, 65, 4, 1, 144),
    "pl_fwd_wrap192": ("conv_ws_kernel<4,1,0,3,2,3,0>", 256, 257, 1, 1, 48),
    "pl_fwd_n320": ("conv_ws_kernel<2,2,0,3,2,9,0>", 9, 3, 3, 1, 144),
    "pl_fwd_n192": ("conv_ws_kernel<2,2,0,3,2,9,0>", 4, 2, 2, 1, 144),
    "pl_fwd_5x5": ("conv_ws_kernel<4,1,0,3,2,3,0>", 1, 1, 1, 1, 48),
    "pl_fwd_post": ("conv_ws_kernel<1,4,0,3,2,3,0>", 3, 3, 1, 1, 48),
    "pl_fwd_pad_only": ("conv_ws_kernel<1,4,0,3,2,3,0>", 2, 2, 1, 1, 48),
    "pl_fwd_w1": ("conv_ws_kernel<1,4,0,3,2,3,0>", 4, 4, 1, 1, 48),
    "pl_fwd_h2_lo": ("conv_ws_kernel<4,1,0,3,2,3,0>", 1, 1, 1, 1, 48),
    "pl_dg_wrap144": ("conv_ws_kernel<1,4,1,3,2,9,0>", 256, 65, 4, 1, 48),
    "pl_dg_3x3_n64": ("conv_ws_kernel<4,1,1,3,2,3,0>", 3, 3, 1, 1, 48),
    "pl_dg_n64_accum": ("conv_ws_kernel<4,1,1,3,2,3,1>", 3, 3, 1, 1, 48),
    "pl_dg_n64_bnr": ("conv_ws_kernel<4,1,1,3,2,3,2>", 3, 3, 1, 1, 48),
    "pl_dg_n64_bnr_res": ("conv_ws_kernel<4,1,1,3,2,3,3>", 3, 3, 1, 1, 48),
    "pl_dg_s2": ("conv_ws_kernel<2,2,1,3,2,9,0>", 4, 4, 1, 1, 48),
    "pl_dg_s2_accum": ("conv_ws_kernel<2,2,1,3,2,9,1>", 4, 4, 1, 1, 48),
    "pl_dg_s2_bnr": ("conv_ws_kernel<2,2,1,3,2,9,2>", 4, 4, 1, 1, 48),
    "pl_dg_s2_bnr_res": ("conv_ws_kernel<2,2,1,3,2,9,3>", 4, 4, 1, 1, 48),
    "pl_dg_s2_bnr_inc": ("conv_ws_kernel<2,2,1,3,2,9,3>", 4, 4, 1, 1, 48),
    "pl_dg_n1024_res": ("conv_ws_kernel<1,4,1,3,2,9,1>", 4, 1, 4, 1, 48),
    "pl_dg_n1024_bnr": ("conv_ws_kernel<1,4,1,3,2,9,2>", 4, 1, 4, 1, 48),
    "pl_dg_n1024_bnr_acc": ("conv_ws_kernel<1,4,1,3,2,9,3>", 4, 1, 4, 1, 48),
    "pl_dg_k32_falls_to_x3": ("conv_igemm_x3_kernel<128,1>", 8, 4, 2, 1, 64),
    "pl_dg_k32_planes_only": (None, 0, 0, 0, 1, 64),
    "planes_7x7": ("conv_igemm_kernel<f32,64,0,0>", 4, 4, 1, 1, 64),
    "ring_fwd_n64": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 3, 3, 1, 1, 64),
    "ring_dg_n64": ("conv_igemm_dma_kernel<64,1,3,3,128,64>", 3, 3, 1, 1, 64),
    "ring_fwd_n256": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 12, 3, 4, 1, 64),
    "ring_dg_n256": ("conv_igemm_dma_kernel<64,1,3,3,128,64>", 12, 3, 4, 1, 64),
    "ring_dg_n256_acc32": ("conv_igemm_dma_kernel<64,2,3,3,128,64>", 12, 3, 4, 1, 64),
    "ring_fwd_bn128": ("conv_igemm_dma_kernel<128,0,3,3,128,64>", 202, 202, 1, 1, 64),
    "ring_dg_bn128": ("conv_igemm_dma_kernel<128,1,3,3,128,64>", 202, 202, 1, 1, 64),
    "ring_dg_bn128_acc32": ("conv_igemm_dma_kernel<128,2,3,3,128,64>", 202, 202, 1, 1, 64),
    "ring_fwd_post": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 12, 3, 4, 1, 64),
    "ring_fwd_256rows": ("conv_igemm_dma_kernel<128,0,3,2,256,128>", 104, 13, 8, 1, 64),
    "ring_dg_256rows": ("conv_igemm_dma_kernel<128,1,3,2,256,128>", 104, 13, 8, 1, 64),
    "ring_dg_256rows_acc32": ("conv_igemm_dma_kernel<128,2,3,2,256,128>", 104, 13, 8, 1, 64),
    "ring_fwd_tail": ("conv_igemm_dma_kernel<128,0,3,3,128,64>", 304, 33, 8, 6, 64),
    "ring_dg_tail": ("conv_igemm_dma_kernel<128,1,3,3,128,64>", 304, 33, 8, 6, 64),
    "ring_fwd_pad_only": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 1, 1, 1, 1, 64),
    "ring_fwd_h1": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 2, 2, 1, 1, 64),
    "ws_fwd_wrap144": ("conv_ws_kernel<1,4,0,3,1,9,0>", 256, 65, 4, 1, 48),
    "ws_fwd_wrap288": ("conv_ws_kernel<2,2,0,3,1,9,0>", 256, 257, 1, 1, 48),
    "ws_dg_wrap144": ("conv_ws_kernel<1,4,1,3,1,9,0>", 256, 65, 4, 1, 48),
    "ws_dg_n128": ("conv_ws_kernel<2,2,1,3,1,9,0>", 1, 1, 1, 1, 48),
    "ws_dg_n256_acc32": ("conv_ws_kernel<1,4,2,3,1,9,0>", 2, 2, 1, 1, 48),
    "ws_dg_n128_acc32": ("conv_ws_kernel<2,2,2,3,1,9,0>", 1, 1, 1, 1, 48),
    "reg_bf16_n32": ("conv_igemm_kernel<bf16,32,1,0>", 1, 1, 1, 1, 64),
    "reg_bf16_n32_dg": ("conv_igemm_kernel<bf16,32,1,1>", 1, 1, 1, 1, 64),
    "reg_bf16_c40": ("conv_igemm_kernel<bf16,128,0,0>", 1, 1, 1, 1, 64),
    "reg_bf16_c40_dg": ("conv_igemm_kernel<bf16,128,0,1>", 1, 1, 1, 1, 64),
    "reg_bf16_c40_n64": ("conv_igemm_kernel<bf16,64,0,0>", 1, 1, 1, 1, 64),
    "reg_bf16_c40_n64_dg": ("conv_igemm_kernel<bf16,64,0,1>", 1, 1, 1, 1, 64),
    "reg_bf16_c40_n24": ("conv_igemm_kernel<bf16,32,0,0>", 1, 1, 1, 1, 64),
    "reg_bf16_c40_n24_dg": ("conv_igemm_kernel<bf16,32,0,1>", 1, 1, 1, 1, 64),
    "f32_n128": ("conv_igemm_kernel<f32,128,1,0>", 1, 1, 1, 1, 64),
    "f32_n128_dg": ("conv_igemm_kernel<f32,128,1,1>", 1, 1, 1, 1, 64),
    "f32_n64": ("conv_igemm_kernel<f32,64,1,0>", 1, 1, 1, 1, 64),
    "f32_n64_dg": ("conv_igemm_kernel<f32,64,1,1>", 1, 1, 1, 1, 64),
    "f32_n32": ("conv_igemm_kernel<f32,32,1,0>", 1, 1, 1, 1, 64),
    "f32_n32_dg": ("conv_igemm_kernel<f32,32,1,1>", 1, 1, 1, 1, 64),
    "f32_c12_n24": ("conv_igemm_kernel<f32,32,0,0>", 1, 1, 1, 1, 64),
    "f32_c12_n24_dg": ("conv_igemm_kernel<f32,32,0,1>", 1, 1, 1, 1, 64),
    "f32_stem": ("conv_igemm_kernel<f32,64,0,0>", 4, 4, 1, 1, 64),
    "f32_stem_dg": ("conv_igemm_kernel<f32,64,0,1>", 14, 14, 1, 1, 64),
    "f32_c12_n136": ("conv_igemm_kernel<f32,128,0,0>", 2, 1, 2, 1, 64),
    "f32_c12_n136_dg": ("conv_igemm_kernel<f32,128,0,1>", 2, 1, 2, 1, 64),
    "f32_pad_only": ("conv_igemm_kernel<f32,64,1,0>", 1, 1, 1, 1, 64),
    "f32_w1": ("conv_igemm_kernel<f32,64,1,0>", 2, 2, 1, 1, 64),
    "x3_n64": ("conv_igemm_x3_kernel<64,0>", 1, 1, 1, 1, 64),
    "x3_n64_dg": ("conv_igemm_x3_kernel<64,1>", 1, 1, 1, 1, 64),
    "x3_n320": ("conv_igemm_x3_kernel<128,0>", 3, 1, 3, 1, 64),
    "x3_n320_dg": ("conv_igemm_x3_kernel<128,1>", 3, 1, 3, 1, 64),
    "x3_mid": ("conv_igemm_x3_kernel<64,0>", 1, 1, 1, 1, 64),
    "x3_pad_only": ("conv_igemm_x3_kernel<64,0>", 1, 1, 1, 1, 64),
    "x3_h1": ("conv_igemm_x3_kernel<64,0>", 2, 2, 1, 1, 64),
    "pl_dg_s2_even": ("conv_ws_kernel<2,2,1,3,2,9,1>", 4, 4, 1, 1, 48),
    "pl_dg_sub00": ("conv_ws_kernel<2,2,1,3,2,9,1>", 1, 1, 1, 1, 48),
    "pl_dg_sub01": ("conv_ws_kernel<2,2,1,3,2,9,1>", 1, 1, 1, 1, 48),
    "pl_dg_sub10": ("conv_ws_kernel<2,2,1,3,2,9,1>", 1, 1, 1, 1, 48),
    "pl_dg_sub11": ("conv_ws_kernel<2,2,1,3,2,9,1>", 1, 1, 1, 1, 48),
    "m49_tile48": ("conv_ws_kernel<1,4,0,3,2,3,0>", 2, 2, 1, 1, 48),
    "m47_tile48": ("conv_ws_kernel<1,4,0,3,2,3,0>", 1, 1, 1, 1, 48),
    "m129_tile128": ("conv_igemm_dma_kernel<64,0,3,3,128,64>", 2, 2, 1, 1, 64),
    "m127_tile128": ("conv_igemm_dma_kernel<64,1,3,3,128,64>", 1, 1, 1, 1, 64),
    "m145_tile144": ("conv_ws_kernel<1,4,1,3,2,9,2>", 2, 2, 1, 1, 48),
    "m143_tile144": ("conv_ws_kernel<1,4,1,3,2,9,1>", 1, 1, 1, 1, 48),
    "m193_tile192": ("conv_ws_kernel<4,1,0,3,2,3,0>", 2, 2, 1, 1, 48),
    "m191_tile192": ("conv_ws_kernel<4,1,1,3,2,3,3>", 1, 1, 1, 1, 48),
    "m3329_tile256": ("conv_igemm_dma_kernel<128,0,3,2,256,128>", 112, 14, 8, 1, 64),
    "m3327_tile256": ("conv_igemm_dma_kernel<128,0,3,2,256,128>", 104, 13, 8, 1, 64),
    "m289_tile288": ("conv_ws_kernel<2,2,0,3,1,9,0>", 2, 2, 1, 1, 48),
    "m287_tile288": ("conv_ws_kernel<2,2,1,3,1,9,0>", 1, 1, 1, 1, 48),
    "ring_dg_n96_bnr_res": ("conv_igemm_dma_kernel<64,1,3,3,128,64>", 6, 3, 2, 1, 64),
}

# every forward and data-gradient instantiation reachable with the default switches
ALL_KERNELS = (
    {REG % ("bf16", bn, 0, m) for bn in (128, 64, 32) for m in (0, 1)} | {REG % ("bf16", 32, 1, m) for m in (0, 1)}
    | {REG % ("f32", bn, al, m) for bn in (128, 64, 32) for al in (0, 1) for m in (0, 1)}
    | {k % m for k in (RING64, RING128) for m in (0, 1, 2)} | {RING256 % 0, RING256 % 1, RING256 % 2}
    | {k % m for k in (WS144, WS288) for m in (0, 1, 2)}
    | {P_W48 % (0, 0), P_W144 % (0, 0), P_N64 % (0, 0), P_NARROW % (0, 0)}
    | {k % (1, e) for k in (P_W144, P_N64, P_NARROW) for e in range(4)}
    | {X3K % (bn, m) for bn in (128, 64) for m in (0, 1)})


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _seed(case, kind):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) * 2 + (kind == "real")) % (2 ** 31)


def inputs(case, kind):
    """dict of float32 / bool arrays the case's buffers hold exactly: x [B,Hi,Wi,C], w [N,R,S,C] and, per epilogue operand, bias [N],
    old [My,N] (the value y held), acc32, res (post_res / res_dz), res_on, bnr_y, bnr_on [My,N], bnr_mean, bnr_invstd, post_* [N]"""
    rs = np.random.RandomState(_seed(case, kind))
    xs, ws, on = (case.B, case.Hi, case.Wi, case.C), (case.N, case.R, case.S, case.C), (case.My, case.N)
    e, d = case.epi, {}
    exact = kind == "exact"

    def small(shape, lim=8):
        return rs.randint(-lim, lim + 1, shape).astype(F32) if exact else rs.standard_normal(shape).astype(F32)

    def pow2(shape):
        return rs.choice([0.5, 1.0, 2.0], shape).astype(F32) if exact else (rs.rand(*shape) + 0.5).astype(F32)
    if exact and case.special == "x3_mid":
        def two(shape):
            return (rs.choice([-3, -2, 2, 3], shape) + rs.choice([-1, 1], shape) * 2.0 ** -8).astype(F32)
        d["x"], d["w"] = two(xs), two(ws)
        d["x"][..., 24:] = 0
    elif exact and case.special == "h2_lo":
        def two(shape):
            a = rs.choice([-3, -2, 2, 3], shape)
            return (a + np.sign(a) * rs.choice([1, 2, 3], shape) * 2.0 ** -12).astype(F32)
        d["x"], d["w"] = two(xs), two(ws)
    elif exact:
        d["x"], d["w"] = rs.randint(-3, 4, xs).astype(F32), rs.randint(-3, 4, ws).astype(F32)
    else:
        d["x"] = rs.standard_normal(xs).astype(F32) * F32(1e3 if case.scaled else 1.0)
        d["w"] = rs.standard_normal(ws).astype(F32) * F32((1e-3 if case.scaled else 1.0) * (2.0 / case.Ktot) ** 0.5)
    if case.dtype == "bf16":
        d["x"], d["w"] = bf16_round(d["x"]), bf16_round(d["w"])
    store = bf16_round if case.dtype == "bf16" else (lambda a: a)
    if "bias" in e:
        d["bias"] = small((case.N,))
    if "accum" in e:
        d["old"] = small(on) if case.out_dtype == "f32" else bf16_round(small(on))
    if "acc32" in e:
        d["acc32"] = small(on)
    if "res" in e or "post_res" in e:
        d["res"] = store(small(on))
    if "res" in e:
        d["res_on"] = rs.rand(*on) < 0.6
    if "bnr" in e:
        d["bnr_y"] = store(small(on))
        d["bnr_on"] = (rs.rand(*on) < 0.6) if "bnr_relu" in e else np.ones(on, bool)
        d["bnr_mean"] = small((case.N,), 4) if exact else (rs.standard_normal(case.N) * 0.2).astype(F32)
        d["bnr_invstd"] = pow2((case.N,))
    if "post" in e:
        d["post_mean"] = small((case.N,), 4) if exact else (rs.standard_normal(case.N) * 0.2).astype(F32)
        d["post_scale"], d["post_shift"] = pow2((case.N,)), small((case.N,), 4)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def conv_fwd(x, w, stride, dil, pad, pad_x, Ho, Wo, dtype=F64):
    """y[b,yo,xo,n] = sum x[b, yo stride - pad + r dil, xo stride - pad_x + s dil, c] w[n,r,s,c]"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    N, R, S, _ = w.shape
    nh, nw = (Ho - 1) * stride + (R - 1) * dil + 1, (Wo - 1) * stride + (S - 1) * dil + 1
    xp = np.pad(x, ((0, 0), (pad, max(0, nh - x.shape[1] - pad)), (pad_x, max(0, nw - x.shape[2] - pad_x)), (0, 0)))
    out = np.zeros((x.shape[0], Ho, Wo, N), dtype)
    for r in range(R):
        for s in range(S):
            win = xp[:, r * dil:r * dil + (Ho - 1) * stride + 1:stride, s * dil:s * dil + (Wo - 1) * stride + 1:stride, :]
            assert win.shape[1:3] == (Ho, Wo)
            out += np.tensordot(win, w[:, r, s, :], axes=([3], [1]))
    return out


def conv_dgrad(dy, wt, stride, dil, pad, pad_x, Ho, Wo, dtype=F64):
    """dX[b,p,q,n] = sum over p = i stride - pad + r dil, q = j stride - pad_x + s dil of dY[b,i,j,c] wt[n,r,s,c]"""
    dy, wt = np.asarray(dy, dtype), np.asarray(wt, dtype)
    N, R, S, _ = wt.shape
    B, Hi, Wi, _ = dy.shape
    Hp, Wp = max(Ho + pad, (Hi - 1) * stride + (R - 1) * dil + 1), max(Wo + pad_x, (Wi - 1) * stride + (S - 1) * dil + 1)
    buf = np.zeros((B, Hp, Wp, N), dtype)
    for r in range(R):
        for s in range(S):
            buf[:, r * dil:r * dil + (Hi - 1) * stride + 1:stride, s * dil:s * dil + (Wi - 1) * stride + 1:stride, :] += \
                np.tensordot(dy, wt[:, r, s, :], axes=([3], [1]))
    return buf[:, pad:pad + Ho, pad_x:pad_x + Wo, :]


def conv_core(case, x, w, dtype=F64):
    """the convolution of the launch alone, [M, N]"""
    f = conv_fwd if (case.mode == 0 and case.sub is None) else conv_dgrad
    return f(x, w, case.stride, case.dil, case.pad, case.pad_x, case.Ho, case.Wo, dtype).reshape(case.M, case.N)


def out_rows(case):
    """row of y (and of every epilogue operand) each row of the launch writes"""
    m = np.arange(case.M)
    if case.sub is None:
        return m
    b, rem = np.divmod(m, case.Ho * case.Wo)
    y2, x2 = np.divmod(rem, case.Wo)
    return (b * 2 * case.Ho + 2 * y2 + case.sub[0]) * 2 * case.Wo + 2 * x2 + case.sub[1]


def h2_lo_dropped(case, inp):
    """what the two-plane kernel leaves out of an h2_lo case: sum of lo lo / (s t) = sum b b' 2^-24"""
    hx, lx, s = h2_terms(inp["x"])
    hw, lw, t = h2_terms(inp["w"])
    assert s == t == 2.0 ** 13
    return conv_core(case, lx.astype(F64) / s, lw.astype(F64) / t)


def groups(case, v, rows):
    """[M, N] -> [G, rows, N] and the valid-row mask [G, rows], zero filled"""
    G = -(-case.M // rows)
    out = np.zeros((G * rows, v.shape[1]), F64)
    out[:case.M] = v
    ok = np.arange(G * rows) < case.M
    return out.reshape(G, rows, -1), ok.reshape(G, rows)


def reference(case, inp, mag=False):
    """dict: y [M, N] float64 (the rows of the launch, before the one rounding of a bf16 store), stored (what the buffer holds),
    stats [G, N, 2], bnr [G, N, 2].  mag = True: the same walk over absolute values -- sum |x w| + |extras| per element of y"""
    e = case.epi
    A = (lambda a: np.abs(np.asarray(a, F64))) if mag else (lambda a: np.asarray(a, F64))
    rows = out_rows(case)
    conv = conv_core(case, A(inp["x"]), A(inp["w"]))
    if case.special == "h2_lo" and not mag:
        conv = conv - h2_lo_dropped(case, inp)
    out = {"conv": conv}
    y = conv.copy()
    if "stats" in e and not mag:
        g, ok = groups(case, conv, case.stat_rows)
        cnt = ok.sum(1)[:, None]
        s = g.sum(1)
        m2 = (np.where(ok[:, :, None], g - (s / cnt)[:, None, :], 0.0) ** 2).sum(1)
        out["stats"] = np.stack([s, m2], -1)
    if "bias" in e:
        y = y + A(inp["bias"])
    if "post" in e:
        y = (y - inp["post_mean"].astype(F64)) * inp["post_scale"].astype(F64) + inp["post_shift"].astype(F64) if not mag else \
            (y + A(inp["post_mean"])) * A(inp["post_scale"]) + A(inp["post_shift"])
        if "post_res" in e:
            y = y + A(inp["res"])[rows]
        if "post_relu" in e and not mag:
            y = np.maximum(y, 0.0)
    if "accum" in e:
        y = y + A(inp["old"])[rows]
    if "acc32" in e:
        y = y + A(inp["acc32"])[rows]
    if "res" in e:
        y = y + np.where(inp["res_on"][rows], A(inp["res"])[rows], 0.0)
    out["y"] = y
    if mag:
        return out
    out["stored"] = bf16_round(y.astype(F32)).astype(F64) if case.out_dtype == "bf16" else y
    if "bnr" in e:
        g = np.where(inp["bnr_on"][rows], conv if "bnr_inc" in e else out["stored"], 0.0)
        xhat = (inp["bnr_y"].astype(F64)[rows] - inp["bnr_mean"].astype(F64)) * inp["bnr_invstd"].astype(F64)
        gg, _ = groups(case, g, case.stat_rows)
        gx, _ = groups(case, g * xhat, case.stat_rows)
        out["bnr"] = np.stack([gg.sum(1), gx.sum(1)], -1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------------------------
def k_steps(case):
    return case.Ktot // BK if case.C % BK == 0 else -(-case.Ktot // BK)


def epi_terms(case):
    e = case.epi
    return sum(1 for k in ("bias", "accum", "acc32", "res", "post_res") if k in e) + (3 if "post" in e else 0)


def conv_chain(case):
    return BK * k_steps(case) + (case.tail_q if case.tail_q > 1 else 0) + epi_terms(case)


def conv_r(case):
    k = case.kernel
    return R_X3 if k.startswith("conv_igemm_x3") else (R_H2 if k.startswith("conv_ws_kernel") and ",3,2," in k else 0.0)


def y_bar(case, inp, ref=None):
    """the bar of every element of y [M, N]"""
    bar = (conv_chain(case) * EPS32 + conv_r(case)) * reference(case, inp, mag=True)["y"]
    if case.out_dtype == "bf16":
        bar = bar + bf16_half_ulp(np.abs((ref or reference(case, inp))["y"]) + bar)
    return bar


def bf16_half_ulp(v):
    """half the bf16 spacing of the binade of |v|: 2^-9 of the binade's upper end 2^(e + 1), i.e. between 2^-9 |v| and 2^-8 |v| (bf16 keeps 8
    significant bits: a value just above 2^e is rounded by up to 2^(e - 8), which no correct store can undercut)"""
    v = np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 8)


def conv_bar(case, inp):
    """the bar of the convolution alone (the accumulators the statistics are taken from)"""
    return ((BK * k_steps(case) + (case.tail_q if case.tail_q > 1 else 0)) * EPS32 + conv_r(case)) * reference(case, inp, mag=True)["conv"]


def stats_bars(case, inp, ref):
    """bars [G, N, 2] of the statistics partials, from the kernel's formula (conv_epilogue / ws_tile_stats): with v_i the fp32
    accumulators (each within e_i = conv_bar of the float64 convolution) of a group of cnt rows,
      sum   = the v_i added in fp32 in some order:                                |error| <= sum e_i + (cnt - 1) eps sum |v_i|
      mean  = sum * fl(1 / cnt): two more roundings:                              em = (|error of sum| + 2 eps |sum|) / cnt (first order)
      d_i   = fl(v_i - mean):                                                     t_i = e_i + em + eps (|v_i| + |mean|)
      M2    = the fl(d_i^2) added in fp32: |error| <= sum (2 |d_i| t_i + t_i^2) + (cnt + 1) eps sum (|d_i| + t_i)^2
    (M2 is taken about the COMPUTED mean; about the exact one it would differ by cnt (mean error)^2, which t_i^2 covers)"""
    e = conv_bar(case, inp)
    g, ok = groups(case, ref["conv"], case.stat_rows)
    eg, _ = groups(case, e, case.stat_rows)
    cnt = ok.sum(1)[:, None].astype(F64)
    av = np.abs(g).sum(1)
    s_bar = eg.sum(1) + (cnt - 1) * EPS32 * (av + eg.sum(1))
    mean = g.sum(1) / cnt
    em = (s_bar + 2 * EPS32 * np.abs(g.sum(1))) / cnt
    okk = ok[:, :, None]
    d = np.where(okk, np.abs(g - mean[:, None, :]), 0.0)
    t = np.where(okk, eg + em[:, None, :] + EPS32 * (np.abs(g) + np.abs(mean)[:, None, :]), 0.0)
    m2_bar = (2 * d * t + t * t).sum(1) + (cnt + 1) * EPS32 * ((d + t) ** 2).sum(1)
    return np.stack([s_bar, m2_bar], -1)


def bnr_bars(case, inp, ref):
    """bars [G, N, 2] of the BatchNorm-backward partials of a real case: g is the stored value (within y_bar of the float64 one; with
    bnr_inc the accumulator, within conv_bar), summed over the group's `rows` rows in fp32; the second sum multiplies by
    fl(fl(y - mean) * invstd): three more roundings per term"""
    e = conv_bar(case, inp) if "bnr_inc" in case.epi else y_bar(case, inp, ref)
    if case.out_dtype == "bf16":       # (the reference's g is the ROUNDED float64 value: half a spacing from y, as the kernel's is within y_bar of y)
        e = e + bf16_half_ulp(ref["y"])
    rows = out_rows(case)
    on = inp["bnr_on"][rows]
    gval = np.where(on, np.abs(ref["conv"] if "bnr_inc" in case.epi else ref["stored"]), 0.0)
    xhat = np.abs((inp["bnr_y"].astype(F64)[rows] - inp["bnr_mean"].astype(F64)) * inp["bnr_invstd"].astype(F64))
    eg, _ = groups(case, np.where(on, e, 0.0), case.stat_rows)
    gg, _ = groups(case, gval, case.stat_rows)
    ex, _ = groups(case, np.where(on, e, 0.0) * xhat, case.stat_rows)
    gx, _ = groups(case, gval * xhat, case.stat_rows)
    n = case.stat_rows
    return np.stack([eg.sum(1) + (n - 1) * EPS32 * (gg.sum(1) + eg.sum(1)), ex.sum(1) + (n + 3) * EPS32 * (gx.sum(1) + ex.sum(1))], -1)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' structure, emulated (tests/test_conv_refs.py: the bars are neither vacuous nor slack)
# ---------------------------------------------------------------------------------------------------------------------
def patches(case, x, dtype=F64, merge_batch=False):
    """[M, R S C]: the operand row of every output row, taps outermost (r, s, c), by pads and slices as the reference: the forward
    launches, and the data gradients as the stride-1 gather over the zero-inserted dY that they are (z[i stride, j stride] = dY[i, j],
    dX[p] = sum over r of z[p + pad - r dil] wt[r]; the parity classes are stride-1 launches as they stand).
    merge_batch: the images stacked without padding between them (a kernel that forgets the batch boundary); a data gradient's images
    at their pitch of Hi stride rows of z"""
    x = np.asarray(x, dtype)
    s, d = case.stride, case.dil
    cols = []
    if case.mode == 1 or case.sub is not None:
        Hz, Wz = case.Hi * s, case.Wi * s                      # (the last stride - 1 rows and columns of z are inserted zeros)
        z = np.zeros((case.B, Hz, Wz, case.C), dtype)
        z[:, ::s, ::s, :] = x
        T, L = max(0, d * (case.R - 1) - case.pad), max(0, d * (case.S - 1) - case.pad_x)
        bot, right = max(0, case.Ho + case.pad - Hz), max(0, case.Wo + case.pad_x - Wz)
        xp = np.pad(z, ((0, 0), (T, bot), (L, right), (0, 0)))
        if merge_batch:
            big = np.pad(z.reshape(1, case.B * Hz, Wz, case.C), ((0, 0), (T, bot + Hz), (L, right), (0, 0)))
            xp = np.stack([big[0, b * Hz:b * Hz + xp.shape[1]] for b in range(case.B)])
        for r in range(case.R):
            for t in range(case.S):
                y0, x0 = T + case.pad - r * d, L + case.pad_x - t * d
                cols.append(xp[:, y0:y0 + case.Ho, x0:x0 + case.Wo, :].reshape(case.M, case.C))
        return np.concatenate(cols, 1)
    nh, nw = (case.Ho - 1) * s + (case.R - 1) * d + 1, (case.Wo - 1) * s + (case.S - 1) * d + 1
    xp = np.pad(x, ((0, 0), (case.pad, max(0, nh - case.Hi - case.pad)), (case.pad_x, max(0, nw - case.Wi - case.pad_x)), (0, 0)))
    if merge_batch:
        flat = x.reshape(1, case.B * case.Hi, case.Wi, case.C)
        big = np.pad(flat, ((0, 0), (case.pad, nh), (case.pad_x, max(0, nw - case.Wi - case.pad_x)), (0, 0)))
        xp = np.stack([big[0, b * case.Hi:b * case.Hi + xp.shape[1]] for b in range(case.B)])
    for r in range(case.R):
        for t in range(case.S):
            cols.append(xp[:, r * d:r * d + (case.Ho - 1) * s + 1:s, t * d:t * d + (case.Wo - 1) * s + 1:s, :].reshape(case.M, case.C))
    return np.concatenate(cols, 1)


def operand_terms(case, a):
    """the terms a kernel multiplies for operand a (float32 array): [(term, scale)] with a = sum term / scale up to the split's error"""
    k = case.kernel
    if k.startswith("conv_igemm_x3"):
        return [(t.astype(F64), 1.0) for t in x3_terms(a)]
    if conv_r(case) == R_H2:
        hi, lo, s = h2_terms(a)
        return [(hi.astype(F64), s), (lo.astype(F64), s)]
    return [(np.asarray(a, F64), 1.0)]


def kept_products(case):
    """index pairs (term of x, term of w) the kernel keeps"""
    if case.kernel.startswith("conv_igemm_x3"):
        return [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
    if conv_r(case) == R_H2:
        return [(0, 0), (0, 1), (1, 0)]
    return [(0, 0)]


def emulate_f32(case, inp):
    """(accumulators, stored y) of a case in float32 in the kernel's structure: K steps of 32 in tap order, every kept product of the
    split terms, the K-split tail's parts summed on their own and added in part order, then the epilogue operands in fp32"""
    P = patches(case, inp["x"], F32)
    W = inp["w"].reshape(case.N, case.Ktot).astype(F32)
    xt = [(t.astype(F32), s) for t, s in operand_terms(case, P)]
    wt = [(t.astype(F32), s) for t, s in operand_terms(case, W)]
    ks = -(-case.Ktot // BK)
    q = case.tail_q if case.tail_q > 1 else 1
    parts = []
    for p in range(q):
        acc = np.zeros((case.M, case.N), F32)
        for j in range(p * ks // q, (p + 1) * ks // q):
            sl = slice(j * BK, min((j + 1) * BK, case.Ktot))
            for a, b in kept_products(case):
                acc += xt[a][0][:, sl] @ wt[b][0][:, sl].T
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    acc = (acc.astype(F64) / (xt[0][1] * wt[0][1])).astype(F32)
    y = acc
    e = case.epi
    if "bias" in e:
        y = y + inp["bias"]
    if "post" in e:
        y = (y - inp["post_mean"]) * inp["post_scale"] + inp["post_shift"]
        if "post_res" in e:
            y = y + inp["res"]
        if "post_relu" in e:
            y = np.maximum(y, F32(0))
    rows = out_rows(case)
    if "accum" in e:
        y = y + inp["old"][rows]
    if "acc32" in e:
        y = y + inp["acc32"][rows]
    if "res" in e:
        y = y + np.where(inp["res_on"][rows], inp["res"][rows], F32(0))
    assert y.dtype == F32
    return acc, (bf16_round(y) if case.out_dtype == "bf16" else y)
