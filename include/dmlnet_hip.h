/*
 * dmlnet_hip.h -- C ABI of libdmlnet_hip.so, the MI355X (gfx950) kernels under the DMLNet hot path.
 *
 * The reference (Jun-CEN/Open-World-Semantic-Segmentation) is 100 % Python and has no FFI: every
 * entry point below replaces a stock ATen/cuDNN op that the reference reaches through the call
 * site cited next to it (paths relative to /root/reference/DeepLabV3Plus-Pytorch unless noted).
 * The Python package `open-world-semantic-segmentation_amd/network` binds these with ctypes and
 * re-exposes the reference's own module API (network.deeplabv3plus_embedding_resnet101, ...).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated;
 *   - activations are NHWC, channel pitch ("ld", in elements) given explicitly so that producers
 *     can write straight into channel slices of a concat buffer (replaces torch.cat,
 *     network/utils.py:32,360);
 *   - conv weights are K-R-S-C ("OHWI"): w[n][r][s][c];
 *   - `dtype` selects the storage type of activations / compute weights: DML_F32 or DML_BF16;
 *     accumulation, batch-norm statistics, the distance head, the loss and the optimizer state
 *     are always fp32;
 *   - the caller owns every buffer (including workspaces); nothing here allocates, frees or
 *     synchronises; every launch goes to `stream` (a hipStream_t passed as void*);
 *   - return value: 0 on success, a negative DML_E* code for a rejected argument, or a positive
 *     hipError_t from the launch.  Nothing throws.
 */
#ifndef DMLNET_HIP_H
#define DMLNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DML_ABI_VERSION 6

enum { DML_F32 = 0, DML_BF16 = 1 };
enum { DML_EINVAL = -1, DML_EALIGN = -2, DML_EUNSUPPORTED = -3 };

int dml_abi_version(void);
/* Name of the code object the library was built for ("gfx950"). */
const char* dml_target_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA (nn.Conv2d call sites: network/backbone/resnet.py:24-32,139;
 * network/utils.py:11-23,311,322,337-352).
 * ---------------------------------------------------------------------------------------------- */
typedef struct DmlConvDesc {
    const void* x;        /* source activations [B,Hi,Wi,C] (fwd: conv input; dgrad: dY), pitch ldx    */
    const void* w;        /* fwd: w[N][R][S][C]; dgrad: transposed copy wt[N=Cin][R][S][C=Cout]         */
    void* y;              /* result [B,Ho,Wo,N], pitch ldy                                               */
    const float* bias;    /* optional [N] (only network/utils.py:23 has a bias)                          */
    float* stats;         /* optional BN partials [ceil(M/rows)][N][2], rows = dml_conv_stat_rows(): (sum, M2 about the */
                          /* group mean) taken from the fp32 accumulators (fused K9)         */
    int32_t B, Hi, Wi, C, ldx;
    int32_t Ho, Wo, N, ldy;
    int32_t R, S, stride, dil, pad;
    int32_t dtype;        /* DML_F32 | DML_BF16 for x, w, y                                              */
    int32_t y_f32;        /* 1: write y as float regardless of dtype                                     */
    int32_t accum;        /* 1: y += result                                                              */
    int32_t mode;         /* 0 = forward gather, 1 = data-gradient gather (transposed conv)              */
    /* (ABI 2: the pre_scale / pre_shift / pre_relu fields of ABI 1 -- the producer's BatchNorm + ReLU applied on the operand
     * load -- are gone: measured on the register-staged kernel in round 1 and on the loader-wave structure in round 4, the
     * transform costs the convolution more than the BatchNorm apply pass it would remove) */
    /* mode 1 only, optional (all NULL/0 otherwise): the result y is the output gradient dz of a BatchNorm
     * (+ReLU) whose pre-normalisation tensor is bnr_y [M][N] (pitch bnr_ldy) with the 1-bit ReLU mask of
     * dml_bn_apply; the epilogue then also writes that BN's backward partial sums, exactly what
     * dml_bn_bwd_reduce would produce from the stored dz: bnr_partials[ceil(M/rows)][N][2], rows = dml_conv_stat_rows() =
     * (sum g, sum g*(bnr_y - mean)*invstd), g = dz * [mask bit] -- pass it with nblocks = ceil(M/rows) to
     * dml_bn_bwd_finalize.  DML_BF16: N % 8 == 0, N > 32.  DML_F32: only launches the two-plane kernel takes (f32_split == 2 with
     * planes; dml_conv_stat_rows() == 48), bnr_y fp32, the mask one byte per four channels, N % 64 == 0; bnr_gmax (optional there):
     * 1024 zeroed floats whose maximum afterwards is max |g| (as `gmax` of dml_bn_bwd_reduce, for dml_h2_bound_bn_bwd). */
    const void* bnr_y;
    const uint8_t* bnr_mask;
    const float* bnr_mean;
    const float* bnr_invstd;
    float* bnr_partials;
    int32_t bnr_ldy, bnr_relu;
    /* mode 0 only, optional: inference epilogue -- y = act((conv - post_mean) * post_scale + post_shift [+ post_res]),
     * i.e. BatchNorm with running statistics (dml_bn_eval_coeffs gives scale / shift, post_mean = running_mean),
     * the bottleneck's residual add (resnet.py:110-113) and ReLU applied to the fp32 accumulators, so the
     * pre-normalisation tensor is never written.  post_res [M][N] has the storage dtype and pitch post_ldres. */
    const float* post_scale;
    const float* post_shift;
    const float* post_mean;
    const void* post_res;
    int32_t post_ldres, post_relu;
    /* optional (bf16, LDS-DMA kernel): balance a launch whose tile count leaves the last round of workgroups mostly
     * empty (576 tiles of 128 x 128 on 256 CUs x 3 slots: a quarter of the CUs carry three tiles, the rest two).  The
     * tiles beyond the last multiple of the CU count are split along K into q workgroups each, so that every CU gets
     * the same share; the parts park their fp32 accumulators in tail_ws ([tiles][q][128*128] floats) with write-through
     * (sc1) stores, wait for them to drain, and take a RELAXED ticket from tail_counters; the part that draws the last
     * ticket reads all parts back with sc1 loads, adds them in part order (deterministic) and runs the epilogue -- no
     * release / acquire fences (an agent-scope release would write back every dirty line of the XCD's L2).
     * tail_counters must be zero on entry and is zero again when the launch has completed.  tail_ws / tail_counters may
     * be shared by every conv of a plan ONLY if those launches are serialised on one stream (two concurrent launches
     * would mix their slabs and tickets); after an aborted launch the caller must zero tail_counters.  NULL = never
     * split. */
    float* tail_ws;
    int64_t tail_ws_elems;
    int32_t* tail_counters;
    int32_t tail_counters_len, tail_reserved;
    /* mode 1 only, optional (same conditions as bnr_*: bf16, or fp32 on the two-plane kernel; not with accum): y = conv + res_dz (.)
     * [res_mask bit], i.e. the gradient that reaches a bottleneck's input through its identity branch -- the block output's gradient
     * res_dz [M][N] (pitch res_ld) masked by the 1-bit ReLU mask of that output (dml_bn_apply's, one byte per 16-byte vector) --
     * is added in the epilogue of conv1's data gradient (resnet.py:96-113 backward), so that the BN-backward apply of
     * the block's bn3 need not write the masked copy (dres = NULL there) for this launch to read back. */
    const void* res_dz;
    const uint8_t* res_mask;
    int32_t res_ld, res_reserved;
    /* mode 1 only, optional (bf16, same conditions as bnr_*; not with accum / y_f32 / res_dz / bnr_*): y = bf16(conv + acc32).
     * A gradient with several producers (autograd's fp32 sum at network/utils.py:360 -- the five ASPP branches reading
     * `out` -- and at resnet.py:96-113 where a block input also feeds the downsample branch) is accumulated in an fp32
     * staging tensor acc32 [M][N] (pitch acc32_ld floats) by the earlier producers (y_f32 = 1, accum = 0 / 1) and the
     * LAST producer adds it to its accumulators and rounds the total once into the bf16 tensor y. */
    const float* acc32;
    int32_t acc32_ld;
    /* dtype DML_F32 only (2: see x_planes below): 1 = compute the products on the bf16 matrix cores through a three-term split of both operands
     * (x = hi + mid + lo, six bf16 MFMAs per block: fp32-level error, 2.7x fewer matrix cycles than v_mfma_f32_16x16x4_f32);
     * 0 = the exact fp32 MFMA, the reference's arithmetic (network/utils.py:84-118 computes in fp32).  Shapes the split kernel
     * does not take (C % 32 != 0, N <= 32) run exact either way.
     * Both split modes REQUIRE finite operands within the narrow format's range: with f32_split == 1 an Inf (or |x| > 3.39e38,
     * which rounds to a bf16 Inf) becomes hi = Inf, mid = Inf - Inf = NaN, so the output is NaN where exact fp32 would carry
     * the Inf; with f32_split == 2 the scale of a tensor that holds an Inf or NaN is 0 / NaN and the whole output is NaN.
     * Either way a non-finite input is visible in the output (never clipped or dropped), but not element for element as in
     * the exact mode.  Residuals below 2^-126 (fp32 subnormals) are flushed. */
    int32_t f32_split;
    /* 1 = `w` is the tile-major copy dml_prep_weights writes (DmlPrepDesc.w_tiled: [N / 64][K / 32][64][32], K = R * S * C): the
     * weight half of every LDS-DMA instruction is one contiguous KB (whole 128-byte lines) instead of sixteen 64-byte row
     * segments.  bf16, C % 32 == 0, N % 64 == 0, LDS-DMA kernels only: DML_EUNSUPPORTED otherwise (never a silent re-layout). */
    int32_t w_tiled;
    /* smallest tile count for which the wave-specialised kernel (one persistent workgroup per CU, dml_conv_stat_rows) takes an
     * eligible launch: 0 = the library's default (192 tiles = three quarters of the CUs), 1 = whenever the shape allows
     * (tests), INT32_MAX = never. */
    int32_t ws_min_tiles;
    /* dtype DML_F32, f32_split == 2: the products on the fp16 matrix cores through a TWO-term split of the power-of-two-scaled
     * operands -- x s = xh + xl, w t = wh + wl (fp16 hi / lo planes written by dml_h2_split), per block wl xh + wh xl + wh xh, fp32
     * accumulation, result unscaled by the exact 1 / (s t): relative error ~2^-21 per element, the reference's own fp32-vs-fp64
     * level on the parity fixtures (tests/tools/emu_split_terms.py) at three MFMAs per block instead of the six of
     * f32_split == 1.  x_planes / w_planes: [2][...] fp16, the hi plane then the lo plane `*_plane_stride` elements further, the
     * activation planes with the geometry (pitch ldx) of `x`, the weight planes tile-major ([N / 64][K / 32][64][32] per plane);
     * x_unscale / w_unscale: device scalars 1 / s and 1 / t (dml_h2_split).  Shapes the planes kernel does not take (C % 32,
     * N % 64, more than 32 taps, misaligned y, a data gradient with R S C < 64) run on x / w, which must therefore be valid as
     * well: the three-term split where that kernel takes the shape (C % 32 == 0, at most 32 taps, N > 32), the exact fp32 MFMA
     * otherwise (the 7 x 7 stem) -- UNLESS the caller keeps the activation as planes only and says so by passing
     * x == x_planes: such a launch returns DML_EUNSUPPORTED when the planes kernel cannot take it (never a fallback that would
     * read the planes as floats). */
    const void* x_planes;
    const void* w_planes;
    const float* x_unscale;
    const float* w_unscale;
    int64_t x_plane_stride, w_plane_stride;
    float* bnr_gmax;      /* see bnr_* above                                                             */
    /* mode 1, two-plane launches (f32_split == 2) only -- one PARITY CLASS of the data gradient of a stride-2 convolution, issued as
     * a stride-1 launch on the grid of dY (round 6): a pixel of dX only sees the filter taps of its own row / column parity, so the
     * data gradient of a 3x3 stride-2 convolution is four stride-1 correlations with 1, 2, 2 and 4 taps (nine instead of 36 tap
     * products per four pixels), that of a 1x1 stride-2 convolution one 1x1 launch on the even pixels.  sub_grid = 1: the rows of this
     * launch (b, y2, x2 on the Ho x Wo grid of the descriptor) are the pixels (b, 2 y2 + sub_y, 2 x2 + sub_x) of y, res_dz, bnr_y and
     * the masks, tensors of B x 2 Ho x 2 Wo pixels; bnr_partials receives ceil(B Ho Wo / 48) groups (the caller offsets the pointer
     * per class).  pad_w_set = 1: `pad_w` replaces `pad` along the width (a class's sub-filter is R x S = 1|2 x 1|2 taps with
     * padding R - 1 / S - 1).  Any other kernel family returns DML_EUNSUPPORTED for such a descriptor. */
    int32_t sub_grid, sub_y, sub_x;
    int32_t pad_w_set, pad_w;
    /* with bnr_* and an accumulating launch (accum = 1): the sums are taken over THIS launch's increment (the convolution result under
     * the mask, before the old value is added) instead of over the stored total -- the BatchNorm-backward sums are linear in the
     * gradient, so the producers of a gradient with several producers can each emit the sums of their own share into their own partial
     * groups (the 1x1 stride-2 data gradient as a parity-class launch only visits a quarter of the pixels: the first producer writes
     * the sums of its share over all pixels).  bnr_gmax still receives the maximum of the stored total. */
    int32_t bnr_inc;
} DmlConvDesc;

#define DML_STAT_ROWS 64   /* rows of the GEMM covered by one statistics partial */

int dml_conv_igemm(const DmlConvDesc* d, void* stream);
/* Rows of the GEMM covered by one partial of `stats` / `bnr_partials` for THIS launch: 48 where the wave-specialised kernel
 * (one persistent workgroup per CU on 144-row tiles: bf16, tile-major weights, N % 128 == 0, enough tiles to fill the chip)
 * takes it -- 144 for a two-plane (f32_split == 2) FORWARD launch on 144-row wave tiles, whose statistics are taken per wave tile
 * (round 6) -- DML_STAT_ROWS otherwise.  Size the partial buffers as ceil(M / rows) * N * 2 floats, pass `rows` to
 * dml_bn_finalize / dml_bn_moments and ceil(M / rows) as `nblocks` to dml_bn_bwd_finalize / dml_bn_bwd_sums. */
int dml_conv_stat_rows(const DmlConvDesc* desc);

/* fp32 tensor x[rows][ld] (C used columns) -> two fp16 planes of s * x, s the power of two that puts max|x| into [2^14, 2^15):
 * hi = fp16(s x), lo = fp16(s x - hi), both round-to-nearest-even, s x = hi + lo up to 2^-22 relative.  planes[0 .. ] = hi,
 * planes[plane_stride ..] = lo (fp16 elements); layout 0: row pitch ldp, element (r, c) at r * ldp + c; layout 1: tile-major
 * [rows / 64][C / 32][64][32] (rows % 64 == 0, C % 32 == 0: the weight operand of the LDS-DMA kernels).  `work`: >= 1025 floats of
 * scratch owned by this tensor; work[1024] receives 1 / s (DmlConvDesc.x_unscale / w_unscale).  Two launches (per-workgroup
 * maxima, then the split: no atomics, no memset, deterministic) -- or one, with amax_known = 1: the maximum over work[0 .. 1024)
 * then already is max |x| (any upper bound within a few binades works: fp16 keeps 11 bits down to 2^-14 of the scaled range),
 * collected by the tensor's producer (dml_bn_apply / dml_bn_bwd_apply, `amax` = work: order-independent atomic maxima spread over
 * those 1024 words, which the caller zeroed).
 * Non-finite values propagate (s becomes 0 or NaN). */
int dml_h2_split(const float* x, int64_t rows, int32_t C, int32_t ld, void* planes, int64_t plane_stride, int32_t ldp,
                 int32_t layout, float* work, int32_t amax_known, void* stream);

/* The same for `count` tensors in two launches; `table_device` is a DEVICE array (the tensors' own constraints as above, checked by the
 * caller: this entry point does not see the descriptors). */
typedef struct DmlH2Desc {
    const float* x;
    void* planes;
    float* work;
    int64_t rows, plane_stride;
    int32_t C, ld, ldp, layout;
} DmlH2Desc;
int dml_h2_split_table(const DmlH2Desc* table_device, int count, void* stream);

typedef struct DmlWgradDesc {
    const void* x;        /* conv input [B,Hi,Wi,C], pitch ldx                                           */
    const void* dy;       /* output gradient [B,Ho,Wo,N], pitch ldy                                      */
    float* dw;            /* fp32 weight gradient [N][R][S][Cm], accumulated (+=): atomics, or via `ws`  */
    int32_t B, Hi, Wi, C, ldx;
    int32_t Ho, Wo, N, ldy;
    int32_t R, S, stride, dil, pad;
    int32_t dtype;
    int32_t splitk;       /* number of slices of the pixel dimension (>=1); 0 = pick automatically      */
    int32_t Cm;           /* un-padded input channels of dw ([N][R][S][Cm]); 0 = C.  Cm < C needs `ws`        */
    float* ws;            /* optional workspace: slices store partials [splitk][N][R*S*C] with plain stores  */
    int64_t ws_elems;     /* and a second kernel folds them into dw (no fp32 atomics); capacity in floats     */
    int32_t f32_split;    /* dtype DML_F32 only: products through the three-term bf16 split (DmlConvDesc.f32_split) */
    int32_t reserved;
    /* f32_split == 2 (dtype DML_F32): both operands as two fp16 planes of the scaled tensors (dml_h2_split, layout 0, the pitches
     * of x / dy), three MFMAs per block on the fp16 matrix cores (DmlConvDesc.x_planes has the arithmetic); NULL planes or
     * misaligned shapes: the three-term split on x / dy -- except that x == x_planes (dy == dy_planes) declares the operand
     * planes-only: DML_EUNSUPPORTED instead of the fallback, as for DmlConvDesc. */
    const void* x_planes;
    const void* dy_planes;
    const float* x_unscale;
    const float* dy_unscale;
    int64_t x_plane_stride, dy_plane_stride;
} DmlWgradDesc;

int dml_conv_wgrad(const DmlWgradDesc* d, void* stream);

/* Weight gradients of several layers in ONE launch: the 48 x 48 layers have 4-9 output tiles each, so a launch of
 * its own needs ~28 pixel slabs per tile to fill 256 CUs and every slab is a 256 KB fp32 partial written and re-read
 * (64 + 64 MB per layer).  Grouped, the same workgroups cover several layers with a few slabs each.  `descs`: HOST
 * array of n <= 12 pointers to descriptors that pass dml_conv_wgrad_group_eligible (bf16, N % 256 == 0, >= 4 output
 * tiles, 31-bit addressable); their ws / ws_elems / splitk are ignored, `ws` (ws_elems floats) is partitioned here. */
int dml_conv_wgrad_group_eligible(const DmlWgradDesc* d);
int dml_conv_wgrad_group(const DmlWgradDesc* const* descs, int n, float* ws, int64_t ws_elems, void* stream);

/* master fp32 weight [N][RS][Cm] -> compute copy [N][RS][Cp] (zero padded, dtype) and, if wt != NULL,
 * the transposed copy wt[Cp][RS][N] used by the data gradient. */
int dml_prep_weight(const float* w_master, void* w, void* wt, int N, int RS, int Cm, int Cp, int dtype,
                    void* stream);
/* The same for every convolution of a model in one launch; `descs_device` is a DEVICE array. */
typedef struct DmlPrepDesc {
    const float* src;     /* master [N][RS][Cm] */
    void* w;              /* [N][RS][Cp] */
    void* wt;             /* [Cp][RS][N] or NULL */
    int32_t N, RS, Cm, Cp;
    /* tile-major copies for the LDS-DMA kernels (DmlConvDesc.w_tiled): the matrix [rows][K] (w: rows = N, K = RS * Cp; wt: rows =
     * Cp, K = RS * N) is stored as [rows / 64][K / 32][64][32], so that the 16 filter rows x 64 bytes one DMA instruction
     * fetches per K step are ONE contiguous KB.  Requires rows % 64 == 0 and K % 32 == 0 (w: Cp % 32 == 0; wt: N % 32 == 0). */
    int32_t w_tiled, wt_tiled;
} DmlPrepDesc;
int dml_prep_weights(const DmlPrepDesc* descs_device, int count, int dtype, void* stream);
/* dst[N][RS][Cm] += src[N][RS][Cp] (drops the padding channels of a padded weight gradient). */
int dml_unpad_wgrad(const float* src, float* dst, int N, int RS, int Cm, int Cp, void* stream);
/* bias gradient: db[n] += sum_m dy[m][n]  (network/utils.py:23) */
int dml_bias_grad(const void* dy, float* db, int64_t M, int N, int ldy, int dtype, void* stream);
/* the same as a fixed-order sum (bitwise reproducible): per-workgroup partial sums in ws (>= 1024 * N floats), then a fold.
 * dml_bias_grad itself combines its workgroups with fp32 atomics. */
int dml_bias_grad_ws(const void* dy, float* db, int64_t M, int N, int ldy, int dtype, float* ws, int64_t ws_elems, void* stream);

/* x[B,C,H,W] fp32 (the reference's input layout) -> NHWC with C padded to Cp, dtype. */
int dml_pack_input(const float* x_nchw, void* y_nhwc, int B, int C, int H, int W, int Cp, int dtype,
                   void* stream);
/* Space-to-depth form of a k x k stride-2 convolution with padding (k - 1) / 2 (odd) on few channels -- the stem, 7x7 s2 on the 3
 * image channels (backbone/resnet.py:139): x2[B][H/2][W/2][4 C] fp32 with channel (dy * 2 + dx) * C + c = x[b][c][2 y2 + dy][2 x2 + dx]
 * (H, W even), w2[N][k2][k2][4 C] with k2 = (k + 1) / 2 holding w[n][2 r2 + dy - 1][2 s2 + dx - 1][c] (zero outside 0 .. k - 1).  The
 * convolution is then a k2 x k2 STRIDE-1 one with padding ((k - 1) / 2 + 1) / 2 on x2 (DmlConvDesc: Ho = H / 2, Wo = W / 2 given
 * explicitly): the same products on K = 4 C k2^2 (192) instead of 8 k^2 (392) for the image padded to 8 channels.
 * dml_s2d_wgrad adds a weight gradient computed in that form (dw2[N][k2][k2][4 C]) to the parameter's dw[N][k][k][C]. */
int dml_pack_input_s2d(const float* x_nchw, float* x2, int B, int C, int H, int W, void* stream);
int dml_s2d_weights(const float* w, float* w2, int N, int k, int C, void* stream);
/* Sub-filter of a prepared fp32 weight copy [rows][taps_src][n]: dst[row][j][:] = src[row][t_j][:] for j < ntaps <= 4 (n % 4 == 0,
 * 16-byte aligned).  The data gradient of a stride-2 convolution (backbone/resnet.py:171-193 of the reference: layer2.0 / layer3.0)
 * runs as one stride-1 launch per pixel-parity class on the taps that class sees (DmlConvDesc.sub_grid); this builds the class's
 * operand from the transposed copy wt[C][R S][N] of dml_prep_weights. */
int dml_gather_taps(const float* src, float* dst, int rows, int taps_src, int n, int ntaps, int t0, int t1, int t2, int t3,
                    void* stream);
int dml_s2d_wgrad(const float* dw2, float* dw, int N, int k, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (112 instances; train: batch statistics, eval: running statistics).
 * ---------------------------------------------------------------------------------------------- */
/* Chan-merge the conv epilogue partials -> mean / biased var -> scale = gamma*invstd, shift = beta,
 * save_mean = mean (required; dml_bn_apply subtracts it before scaling so that low-variance channels do
 * not cancel); updates running stats with the unbiased variance and `momentum` exactly as
 * nn.BatchNorm2d does; saves invstd for the backward.  `partials` is scratch: the call may fold it in place
 * (large feature maps), so it is not valid input for a second call. */
/* stat_rows: rows of the GEMM covered by one partial = dml_conv_stat_rows() of the launch that wrote them (DML_STAT_ROWS for
 * dml_bn_stats). */
int dml_bn_finalize(float* partials, int64_t M, int N, int stat_rows, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);
/* Synchronised BatchNorm (statistics over all ranks' samples; anomaly/lib/nn/modules/batchnorm.py:56-139 of the
 * reference -- biased variance for the normalisation, unbiased over the global count for the running estimate).
 * The library stays collective-free: the caller all-gathers / all-reduces the small double buffers (RCCL).
 *   forward : dml_bn_moments(partials -> moments[N][2] = (mean, M2) of this rank's M rows)
 *             -> all_gather -> dml_bn_finalize_moments(moments[ranks][N][2], every rank holding M_each rows)
 *   backward: dml_bn_bwd_sums(partials -> sums[N][2] = (sum g, sum g*xhat); dgamma/dbeta += the LOCAL sums)
 *             -> all_reduce(sum) -> dml_bn_bwd_coef(sums, M_total) -> dml_bn_bwd_apply as usual. */
int dml_bn_moments(float* partials, int64_t M, int N, int stat_rows, double* moments, void* stream);
int dml_bn_finalize_moments(const double* moments, int ranks, int64_t M_each, int N, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, float momentum,
                            float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                            void* stream);
int dml_bn_bwd_sums(float* partials, int nblocks, int N, double* sums, float* dgamma, float* dbeta,
                    void* stream);
int dml_bn_bwd_coef(const double* sums, int64_t M_total, int N, const float* gamma, const float* save_mean,
                    const float* save_invstd, float* coef, void* stream);
/* Standalone statistics for tensors that were not produced by dml_conv_igemm (writes the same
 * partial format). */
int dml_bn_stats(const void* y, float* partials, int64_t M, int N, int ldy, int dtype, void* stream);
/* eval mode: scale = gamma/sqrt(running_var+eps), shift = beta; pass running_mean as `mean` to dml_bn_apply. */
int dml_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, int N,
                       void* stream);
/* the same for a whole network in one launch: `table` is a DEVICE array of `count` descriptors */
typedef struct DmlBnEvalDesc {
    const float* gamma; const float* beta; const float* running_var; float* scale; float* shift;
    int32_t N; float eps;
} DmlBnEvalDesc;
int dml_bn_eval_coeffs_table(const DmlBnEvalDesc* table, int count, void* stream);
/* z = act((y - mean)*scale + shift [+ res]) with optional inverted dropout (network/utils.py:354).
 * y, res, z have independent pitches.  `mask` (optional): one bit per element, z > 0, one BYTE per 16-byte vector of z --
 * DML_BF16: mask[m*(N/8) + c/8] bit c%8; DML_F32: mask[m*(N/4) + c/4] bit c%4 -- the backward passes then read 1 byte
 * instead of 16 bytes of z.  `amax` (optional): 1024 floats the caller zeroed; their maximum afterwards is max |z| (one
 * order-independent atomic maximum per workgroup, spread over the words: dml_h2_split, amax_known).
 * `planes` (optional, DML_F32): the output also as the two fp16 planes a conv of the f16x2 mode reads (dml_h2_split's arithmetic and
 * layout 0: hi at planes[m * ldp + c], lo `plane_stride` elements further), scaled by 1 / unscale[0], a power of two the caller
 * fixed BEFORE this launch from a bound on |z| (dml_h2_bound_bn) -- no dml_h2_split pass over z then; z may be NULL when nothing
 * reads the fp32 tensor.  `res_unscale` (optional, DML_F32; ABI 4): the residual operand exists as fp16 planes only -- `res` then
 * points at its hi plane (pitch ldres, lo plane `res_plane_stride` elements further) and the value added is (hi + lo) *
 * res_unscale[0], exactly what the convolutions reading those planes see. */
int dml_bn_apply(const void* y, const void* res, void* z, const float* scale, const float* shift,
                 const float* mean, uint8_t* mask, int64_t M, int N, int ldy, int ldres, int ldz, int relu,
                 int dtype, float drop_p, uint64_t drop_seed, float* amax, void* planes, int64_t plane_stride,
                 int32_t ldp, const float* unscale, int64_t res_plane_stride, const float* res_unscale, void* stream);
/* backward, pass 1: per-channel sums of g = dz*[z>0]*gscale and g*xhat -> partials[blocks][N][2]
 * ([z>0] from `mask` when given, else from z).
 * returns the number of partial rows through *nblocks (host int).  `gmax` (optional): 1024 zeroed floats, their maximum
 * afterwards is max |g| (as `amax` of dml_bn_apply; input of dml_h2_bound_bn_bwd). */
int dml_bn_bwd_reduce(const void* dz, const void* y, const void* z, const uint8_t* mask, const float* save_mean,
                      const float* save_invstd, float* partials, int64_t M, int N, int lddz, int ldy,
                      int ldz, int relu, float gscale, int dtype, int* nblocks, float* gmax, void* stream);
/* backward, pass 1b: fold partials, write dgamma/dbeta (+=) and the per-channel coefficients
 * coef[4][N] with dy = coef0*g + coef1*(y - coef3) + coef2  (coef3 = batch mean).
 * M = 0 selects a layer that normalised with FIXED statistics (BatchNorm2d.eval() inside a training step, the
 * reference's main_self_distillation.py:432-435): save_mean / save_invstd are then the running statistics, the two
 * correction terms are zero (coef1 = coef2 = 0); dgamma / dbeta still receive the sums (+=), as autograd of an eval() BatchNorm gives.
 * With more than 2048 partial rows they are first folded in place (two coalesced stages): `partials` is clobbered. */
int dml_bn_bwd_finalize(float* partials, int nblocks, int64_t M, int N, const float* gamma,
                        const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta,
                        float* coef, void* stream);
/* backward, pass 2: dy = coef0*g + coef1*(y - coef3) + coef2; optionally dres (+)= g for the identity branch.  `amax`
 * (optional): max |dy|, as in dml_bn_apply.  `planes` / `plane_stride` / `ldp` / `unscale` (optional, DML_F32): dy as fp16 planes,
 * as in dml_bn_apply (scale from dml_h2_bound_bn_bwd); dy may then be NULL. */
int dml_bn_bwd_apply(const void* dz, const void* y, const void* z, const uint8_t* mask, const float* coef, void* dy,
                     void* dres, int64_t M, int N, int lddz, int ldy, int ldz, int lddy, int lddres,
                     int relu, float gscale, int dres_accum, int dtype, float* amax, void* planes, int64_t plane_stride,
                     int32_t ldp, const float* unscale, void* stream);
/* The stem (network/backbone/resnet.py:139-143: conv1 -> bn1 -> ReLU -> MaxPool2d(3, 2, 1)) without its full-resolution tensors.
 * Forward: dml_bn_apply (ReLU) + dml_maxpool3x3s2_fwd in one pass over y[B][H][W] (pitch ldy, fp32, C % 8 == 0): per pooled
 * element the window taps in the order r, then s, z = (y - mean) * scale + shift, ReLU, the maximum with dml_maxpool3x3s2_fwd's
 * rule (first wins on ties, NaN propagates) -- `p` and `argmax` are bit-equal to the two-call sequence's.  Outputs, each optional
 * (one of p / planes is required): p[B][Ho][Wo][C] fp32; argmax (one byte per element, 0 .. 8); `mask`, the ReLU mask of the
 * UNPOOLED tensor in dml_bn_apply's fp32 layout (one byte per four channels, [B H W][C / 4]); the two fp16 planes of p (pitch C,
 * lo `plane_stride` elements behind hi) scaled by 1 / unscale[0] -- the BatchNorm's bound (dml_h2_bound_bn) holds for the pooled
 * tensor too, a maximum of bounded values; `amax`, 1024 zeroed words raised to max |p| as dml_bn_apply raises them, for a
 * dml_h2_split of p with amax_known = 1 (the scale, and with it the planes, that the split computes from p on its own). */
int dml_bn_relu_maxpool3x3s2_fwd(const void* y, const float* scale, const float* shift, const float* mean, void* p,
                                 uint8_t* argmax, uint8_t* mask, void* planes, int64_t plane_stride, const float* unscale,
                                 float* amax, int B, int H, int W, int C, int ldy, void* stream);
/* Backward: dml_maxpool3x3s2_bwd + dml_bn_bwd_reduce / dml_bn_bwd_apply (ReLU from `mask`, gscale 1) without the d(z) tensor
 * between them.  Both form g of an input pixel from dp = d(p)[B][Ho][Wo][C] and the argmax bytes -- its (at most four) windows added
 * in dml_maxpool3x3s2_bwd's order, then the pixel's mask bits -- so g, and with equal `coef` dy, are bit-equal to the three-call
 * sequence's.  fp32, C % 4 == 0.  The reduce walks the pixels in dml_bn_bwd_reduce's geometry and order: *nblocks and the partial
 * rows (for dml_bn_bwd_finalize[_bound]; `gmax` as there) are bit-equal to what that call writes from the d(z) tensor; the apply writes dy[B H W] (pitch lddy) and / or its planes as dml_bn_bwd_apply does. */
int dml_stem_bn_bwd_reduce(const void* dp, const uint8_t* argmax, const uint8_t* mask, const void* y, const float* save_mean,
                           const float* save_invstd, float* partials, int B, int H, int W, int C, int ldy, int* nblocks,
                           float* gmax, void* stream);
int dml_stem_bn_bwd_apply(const void* dp, const uint8_t* argmax, const uint8_t* mask, const void* y, const float* coef, void* dy,
                          int B, int H, int W, int C, int ldy, int lddy, void* planes, int64_t plane_stride, int32_t ldp,
                          const float* unscale, void* stream);
/* The BatchNorm backward of the unit in FRONT of a 1x1 convolution with few output channels (the decoder's 256 -> 16 embedding
 * conv, network/utils.py:24-27), without that conv's data gradient as a tensor: dz[m][c] = sum_{k < K} de[m][k] w[k][c], formed per
 * row in registers with fp32 FMAs in the order k = 0, 1, ... (de[M][Kp] with pitch ldde, Kp in {8, 16, 24, 32} columns of which the
 * first K count; w[K][N] with pitch ldw: the convolution's own weight).  Otherwise dml_bn_bwd_reduce / dml_bn_bwd_apply for fp32
 * tensors with the ReLU taken from `mask` and gscale 1. */
int dml_head_bn_bwd_reduce(const void* de, const float* w, const void* y, const uint8_t* mask, const float* save_mean,
                           const float* save_invstd, float* partials, int64_t M, int N, int K, int Kp, int ldde, int ldw, int ldy,
                           int relu, int* nblocks, float* gmax, void* stream);
int dml_head_bn_bwd_apply(const void* de, const float* w, const void* y, const uint8_t* mask, const float* coef, void* dy,
                          int64_t M, int N, int K, int Kp, int ldde, int ldw, int ldy, int lddy, int relu, void* planes,
                          int64_t plane_stride, int32_t ldp, const float* unscale, void* stream);
/* Scale of a batch-statistics BatchNorm output's fp16 planes from a BOUND on its magnitude, available before the tensor is
 * written: every normalised element obeys |y - mean| * invstd <= sqrt(count) (count = elements per channel over all ranks that
 * share the statistics), so |z| <= max_c (|gamma_c| sqrt(count) + |beta_c|) * mult + max |res| (`mult`: 1, or the dropout's
 * 1 / (1 - p); `res_amax`: NULL, or the 1024 amax words of the residual tensor) and, in the backward, |dy| <= max_c (|coef0_c| max|g|
 * + |coef1_c| sqrt(count) / invstd_c + |coef2_c|) (`g_amax`: the words dml_bn_bwd_reduce raised).  work[1024] receives 1 / s, s the
 * power of two that puts the bound into [2^14, 2^15) -- the `unscale` of the apply kernels and DmlConvDesc.x_unscale.  A bound 2^k
 * above the true maximum costs the planes k of the ~12 binades over which an element keeps its full 2^-22 relative precision. */
int dml_h2_bound_bn(const float* gamma, const float* beta, int N, int64_t count, float mult, const float* res_amax,
                    float* work, void* stream);
int dml_h2_bound_bn_bwd(const float* coef, const float* save_invstd, int N, int64_t count, const float* g_amax,
                        float* work, void* stream);
/* The two pairs above as ONE launch each (round 6: 145 dependent one-block launches per train step removed).  Every block of the
 * finalize kernel raises state[0] to the largest bound term of its own channels and takes a ticket in state[1]; the block that
 * arrives last writes work[1024] and leaves both words zero for the next call.  `state`: two zero-initialised 32-bit words owned by
 * this BatchNorm (not shared between launches that may run concurrently).  Results equal the two-call sequence's.  Replaces
 * nn.BatchNorm2d's statistics step in backbone/resnet.py:97-108 of the reference like the calls it fuses. */
int dml_bn_finalize_bound(float* partials, int64_t M, int N, int stat_rows, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps,
                          float* scale, float* shift, float* save_mean, float* save_invstd,
                          int64_t count, float mult, const float* res_amax, float* work, uint32_t* state, void* stream);
int dml_bn_bwd_finalize_bound(float* partials, int nblocks, int64_t M, int N, const float* gamma,
                              const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta,
                              float* coef, int64_t count, const float* g_amax, float* work, uint32_t* state, void* stream);
/* dml_h2_bound_bn for `count` residual-free BatchNorms in one launch (`table_device`: DEVICE array; root_count = sqrt(elements per
 * channel) * 1.0001, as the single call computes it). */
typedef struct DmlH2BoundDesc {
    const float* gamma;
    const float* beta;
    float* work;
    int32_t N;
    float root_count, mult;
    int32_t reserved;
} DmlH2BoundDesc;
int dml_h2_bound_bn_table(const DmlH2BoundDesc* table_device, int count, void* stream);
/* ONE scale for a tensor that several batch-statistics BatchNorms write channel slices of (directly, or through a bilinear resize,
 * which keeps the bound): work[1024] = 1 / s from the LARGEST of the `count` entries' bounds (their own `work` fields are ignored).
 * The decoder's concat buffer of network/utils.py:28-32 (low-level projection + upsampled ASPP projection) then exists as fp16 planes
 * only: no dml_h2_split pass (an amax pass + a split pass over 755 MB at 16 x 768 x 768). */
int dml_h2_bound_bn_multi(const DmlH2BoundDesc* table_device, int count, float* work, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling (network/backbone/resnet.py:143; network/utils.py:320,326-329).
 * ---------------------------------------------------------------------------------------------- */
int dml_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* argmax, int B, int H, int W, int C, int dtype,
                         void* stream);
int dml_maxpool3x3s2_bwd(const void* dy, const uint8_t* argmax, void* dx, int B, int H, int W, int C,
                         int dtype, void* stream);
/* y[b][c] = mean over HW of x[b,:,:,c]  (AdaptiveAvgPool2d(1)); y has dtype. */
int dml_global_avgpool_fwd(const void* x, void* y, int B, int HW, int C, int ldx, int dtype, void* stream);
/* z[b,h,w,c] = v[b][c] (bilinear upsample of a 1x1 map is a broadcast) */
int dml_broadcast_hw(const void* v, void* z, int B, int HW, int C, int ldz, int dtype, void* stream);
/* dv[b][c] = sum over HW of dz[b,:,:,c] */
int dml_reduce_hw(const void* dz, void* dv, int B, int HW, int C, int lddz, int dtype, void* stream);
/* out[b][c] = scale * sum over HW of x[b,:,:,c], x in `dtype`, out ALWAYS fp32.  The ASPP image-pooling branch
 * (network/utils.py:318-329) runs a BatchNorm over only B samples per channel: its input (scale = 1/HW) and its output
 * gradient (scale = 1) are B x C values whose sample-to-sample DIFFERENCES decide 1/sigma and the backward's
 * cancellation, so the bf16 plans keep them unrounded. */
int dml_reduce_hw_f32(const void* x, float* out, int B, int HW, int C, int ldx, int dtype, float scale, void* stream);
/* dx[b,:,:,c] += dv[b][c] / HW */
int dml_avgpool_bwd_add(const void* dv, void* dx, int B, int HW, int C, int lddx, int dtype, void* stream);
/* dx[b,:,:,c] = dv[b][c] / HW.  In bf16 the plan lets this INITIALISE the gradient buffer and the data gradients of the
 * other ASPP branches accumulate on top: added last, a per-pixel term of 1/HW of a pooled gradient is below half an ulp
 * of the running sum at every pixel and would vanish entirely, although it is coherent over the image. */
int dml_avgpool_bwd_set(const void* dv, void* dx, int B, int HW, int C, int lddx, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=False (F.interpolate call sites network/utils.py:30,88,329).
 * in_f32 / out_f32 select float storage for that side, otherwise `dtype`.
 * ---------------------------------------------------------------------------------------------- */
int dml_bilinear_fwd(const void* x, void* y, int B, int h, int w, int H, int W, int C, int ldx, int ldy,
                     int dtype, int in_f32, int out_f32, void* stream);
/* dml_bilinear_fwd of an fp32 tensor with the result as the two fp16 planes of the scaled value (hi at `planes`, lo `plane_stride`
 * elements further, pitch ldp, scale = 1 / unscale[0]: dml_h2_split's arithmetic on the value dml_bilinear_fwd would store). */
int dml_bilinear_fwd_planes(const float* x, void* planes, int64_t plane_stride, int ldp, const float* unscale, int B, int h, int w, int H,
                            int W, int C, int ldx, void* stream);
int dml_bilinear_bwd(const void* dy, void* dx, int B, int h, int w, int H, int W, int C, int lddy,
                     int lddx, int dtype, int in_f32, int out_f32, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel -> prototype squared-distance head (network/utils.py:92-118; anomaly/models/models.py:636-657)
 * and what the drivers compute from it on the host (test_embedding.py:339-350,428-445;
 * anomaly/eval_ood_traditional.py:301-305).
 * ---------------------------------------------------------------------------------------------- */
/* x: embedding at full resolution, NCHW fp32 (what F.interpolate returns at utils.py:88).
 * logits[b,k,h,w] = -sum_c (x[b,c,h,w]-protos[k][c])^2 (NCHW), features_out = x in NHWC.
 * Any of logits / feats / argmax / dissum may be NULL.  192 B per pixel at K=C=16.
 *   feats    a copy of x, bit for bit (-0.0 and NaN payloads included).
 *   argmax   [B,H,W] uint8: the FIRST k with the largest logit (strict > against a running best that starts at -inf, k = 0).  A NaN
 *            logit therefore never wins, and a pixel with no logit above -inf (all NaN or -inf: a NaN or inf feature) reports 0.
 *   dissum   [B,H,W] = -sum_k logits[b,k,h,w], the kernel's own fp32 logits summed in k order.
 *   inf / NaN features propagate: every logit and the dissum of that pixel are -inf / +inf or NaN; other pixels are not touched.
 * Supported: 1 <= C <= 32, 1 <= K <= 33 (DML_EUNSUPPORTED otherwise); x or protos NULL, B / H / W <= 0: DML_EINVAL.  Nothing is
 * launched when a code is returned.
 * Alignment (assumed, not checked): with H*W % 4 == 0 a lane owns four consecutive pixels and x, logits and dissum are accessed as
 * 16-byte vectors -- they must be 16-byte aligned; with C % 4 == 0 a pixel's features are stored as 16-byte vectors -- feats must be
 * 16-byte aligned.  Otherwise 4-byte alignment is enough.  argmax has no alignment requirement. */
int dml_proto_dist_fwd(const float* x_nchw, const float* protos, float* logits, float* feats,
                       uint8_t* argmax, float* dissum, int B, int C, int K, int H, int W, void* stream);
/* Fused: bilinear x(H/h) upsample of the low-resolution embedding e[B,h,w,C] (NHWC fp32) + the
 * distance head, writing logits NCHW and features_out NHWC at [H,W].
 *   feats = F.interpolate(e, (H,W), bilinear, align_corners = False) in fp32 (any ratio, shrinking included); logits, argmax (first
 *   maximum, NaN never wins) and dissum as dml_proto_dist_fwd defines them, on those features.  Any of the four outputs may be NULL.
 *   A non-finite value of e makes the output pixels that interpolate it non-finite; which pixels next to those also become NaN
 *   (a zero weight times inf) is not part of the contract.
 * Supported C, K and the codes: as dml_proto_dist_fwd, with h / w <= 0 refused as well.
 * Alignment (assumed, not checked): with W % 4 == 0 logits and dissum are written as 16-byte vectors and must be 16-byte aligned; with
 * C % 4 == 0 e is read and feats is written as 16-byte vectors and both must be 16-byte aligned. */
int dml_upsample_dist_fwd(const float* e, const float* protos, float* logits, float* feats,
                          uint8_t* argmax, float* dissum, int B, int h, int w, int C, int K, int H,
                          int W, void* stream);
/* Merged prediction of the incremental multi-head model (test_self_distillation.py:292-297) from the heads' low-resolution
 * embeddings, in one pass and without full-resolution logits or features: 8 bytes written per pixel.
 *   heads: HOST array of n descriptors (copied into the launch; the `e` inside are device pointers): e = embedding
 *          [B,h,w,ld] NHWC fp32 -- what dml_upsample_dist_fwd takes --, C = channels carried (C <= ld; columns C..ld-1 are
 *          never read), K = prototypes, novel_id = the class this head contributes (unused for head 0).
 *   Per output pixel and head: f = bilinear sample of e at (H,W), align_corners = False, dml_upsample_dist_fwd's source
 *   coordinates and weights; a_i = first maximal k of d_k = -sum_c (f_c - P[k][c])^2 over k < K, with P = 3 I_K cut to C
 *   columns (Engine.prototypes; row C of a K = C + 1 head is zero).  Because d_k = 6 f_k - 9 - sum_c f_c^2 the kernel compares
 *   the f_k (1.5 for k = C) and never rounds a distance: exact ties of f are exact ties of d, lowest k wins.
 *   preds[B,H,W] (int64) = a_0, then for i = 1 .. n-1 in order: a_i == heads[i].novel_id -> preds = novel_id (a later head
 *   overrides an earlier one; any other a_i changes nothing).  head_argmax: optional [n,B,H,W] uint8 = a_i; NULL skips it.
 *   Any H, W >= 1 for any h, w >= 1.  preds is stored as 16-byte pairs from its first 16-byte boundary on, single values
 *   before it and after the last whole pair; embedding rows are read as 16-byte vectors when C % 4 == 0, ld % 4 == 0 and e
 *   is 16-byte aligned, as scalars otherwise.
 * DML_EINVAL: heads or preds NULL, n < 1, B / h / w / H / W <= 0, or a head with e NULL, C <= 0, K <= 0 or ld < C.
 * DML_EUNSUPPORTED: n > DML_PREDICT_MAX_HEADS, or a head with C > 32, K > 33 or K > C + 1 (prototype k lives in channel k:
 *   beyond k = C it has no channel to be compared in).  DML_EALIGN: preds not 8-byte aligned.
 * Nothing is written when a code is returned. */
#define DML_PREDICT_MAX_HEADS 4
typedef struct DmlPredictHead {
    const float* e;
    int32_t C, K, ld, novel_id;
} DmlPredictHead;
int dml_incremental_predict(const DmlPredictHead* heads, int n, int64_t* preds, uint8_t* head_argmax, int B, int h, int w,
                            int H, int W, void* stream);
/* df[b,h,w,c] = -2 * sum_k glogits[b,k,h,w] * (feats[b,h,w,c]-protos[k][c]) (+ gfeats[b,h,w,c]); gfeats may be NULL.
 * Evaluated as -2 (gs f - gm) with gs = sum_k g_k and gm_c = sum_k g_k protos[k][c]: a pixel whose g_k are all zero gets
 * df = gfeats (or 0).  1 <= C <= 32, 1 <= K <= 33 (DML_EUNSUPPORTED otherwise); glogits, feats, protos or df NULL, B / H / W <= 0:
 * DML_EINVAL, before any launch.  Alignment (assumed, not checked): glogits 16-byte aligned when H*W % 4 == 0; feats, gfeats and df
 * 16-byte aligned when C % 4 == 0. */
int dml_proto_dist_bwd(const float* glogits, const float* gfeats, const float* feats,
                       const float* protos, float* df, int B, int C, int K, int H, int W, void* stream);

/* Backward of DML loss + distance head + final x4 upsample in one pass, for a loss whose only input is this head's
 * logits: de[B,h,w,C] (dtype) = bilinear^T( d loss / d features ), d loss / d logits exactly as dml_loss_bwd defines it
 * (sums / gout / alpha / n_images / ignore_index as there) with the logits recomputed from feats[B,H,W,C].
 * C = K = 16, H = 4h, W = 4w; anything else returns DML_EUNSUPPORTED (use dml_loss_bwd + dml_proto_dist_bwd +
 * dml_bilinear_bwd).  72 B per full-resolution pixel instead of 394. */
int dml_head_bwd_fused(const float* feats, const int64_t* labels, const double* sums, const float* gout,
                       const float* protos, void* de, int B, int h, int w, int C, int K, int H, int W,
                       int64_t ignore_index, float alpha, float n_images, int dtype, void* stream);

/* preds = argmax_k logits (ties -> lowest k), msp = 1 - max softmax  (test_embedding.py:339-341) */
int dml_argmax_msp(const float* logits, int64_t* preds, float* msp, int B, int K, int H, int W,
                   void* stream);
/* s = -sum_k logit_k, clipped (inclusive: s>=clip -> clip, else s>clip -> clip), then per-image
 * min-max normalised.  work: 2*B floats. */
int dml_dissum_score(const float* logits, float* score, float* work, int B, int K, int H, int W,
                     float clip, int inclusive, void* stream);
/* preds[p] = new_label where -|f_p - proto|^2 > thresh and > max_k logits[k][p] */
int dml_novel_relabel(const float* feats, const float* logits, const float* proto, int64_t* preds,
                      int B, int C, int K, int H, int W, float thresh, int64_t new_label, void* stream);
/* The three calls above in one pass over logits[B,K,H,W] and feats[B,H,W,C], for N <= 8 few-shot prototypes
 * (test_embedding.py:339-350,365,445 and the 2- / 3-class rules kept at :510-511,:520-522 of the reference):
 *   preds = first maximal k (as dml_argmax_msp); msp = 1 - max softmax; score = dml_dissum_score's value (same clip
 *   rule, +0.0 for a zero sum, per-image min / max left in work[2 b], work[2 b + 1], then normalised by a second launch);
 *   d_j = -sum_c (f_c - protos[j][c])^2; with j* the index whose d is strictly above every other d_j (a tie for the top:
 *   none), preds = new_labels[j*] iff d_j* > thresh and (vs_known == 0 or d_j* > max_k logit_k).
 * N = 1, vs_known = 1 is dml_novel_relabel's rule; vs_known = 0 compares the novel distances only with each other.
 * msp and score may be NULL (score != NULL needs work: 2 B floats).  N = 0 skips the relabel and never reads feats /
 * protos / new_labels (they may be NULL).  protos [N,C] and new_labels [N] are device arrays.
 * DML_EINVAL: a required pointer is NULL, or B, C, K, H, W <= 0, or N < 0.  DML_EUNSUPPORTED: C > 32, K > 33, N > 8,
 * B > 65535 or B H W > 2^40.  16-byte loads (4 pixels per lane) when H W % 4 == 0 and the tensors are 16-byte aligned,
 * one pixel per lane otherwise; C = K = 16 keeps logits and features in registers. */
int dml_open_world_post(const float* logits, const float* feats, const float* protos, const int64_t* new_labels,
                        int64_t* preds, float* msp, float* score, float* work, int B, int C, int K, int H, int W,
                        int N, float thresh, int vs_known, float clip, int inclusive, void* stream);
/* The relabel rule of dml_open_world_post alone, in place on given preds (a second instantiation of the same kernel:
 * only relabelled pixels are written; the logits are read only when vs_known != 0).  Same checks and codes. */
int dml_novel_relabel_multi(const float* feats, const float* logits, const float* protos, const int64_t* new_labels,
                            int64_t* preds, int B, int C, int K, int H, int W, int N, float thresh, int vs_known,
                            void* stream);

/* kNN cosine-similarity anomaly score (anomaly/eval_ood_traditional.py:511-530 of the reference, `--ood knn`, neighbor_size = 9
 * there) of feats[B,C,H,W] fp32 (NCHW, contiguous: the multi-scale mean of the upsampled embedding) in one launch:
 *   n(b,y,x) = f(b,:,y,x) / max(|f(b,:,y,x)|_2, 1e-8)      (ATen's cosine_similarity: each norm clamped on its own)
 *   score[b,y,x] = sum_{i=1..R} sum_{j=1..R} n(b,y,x) . n(b,y+i,x+j) + n(b,y,x) . n(b,y-i,x-j),   R = neighbor_size - 1
 * -- the down-right and the up-left quadrant only, 2 R^2 neighbours, none on the pixel's own row or column; a neighbour outside
 * the image contributes exactly 0 (the reference's shifted copy is zero there), so images smaller than the neighbourhood are
 * fine; a pixel whose own vector is zero scores exactly 0; neighbor_size = 1 gives an all-zero map.  Computed as
 * sum_c n_c(p) * (row sums, then column sums of n_c over the quadrants): 4 R additions per pixel and channel.  No workspace, no
 * atomics, every sum in a fixed order over the plain values: bitwise reproducible, image b of a batch equals the image alone, and
 * C = 1 gives exact integers.  Inputs |f| <= 1e18 (the squares stay finite).  16-byte loads and stores when W % 4 == 0 and both
 * pointers are 16-byte aligned, one float per lane otherwise.  The reference's resize of the map to segSize is the identity
 * (feats already has that size) and its plot is not reproduced.
 * DML_EINVAL: a NULL pointer, B, C, H, W <= 0 or neighbor_size < 1.  DML_EUNSUPPORTED: C > 32, neighbor_size > 17, B > 65535 or
 * B H W > 2^40.  Nothing is launched when a code is returned. */
int dml_knn_cosine_score(const float* feats, float* score, int B, int C, int H, int W, int neighbor_size, void* stream);

/* The paper's "EDS + MMSP" anomaly score of logits[B,K,H,W] fp32 (NCHW, contiguous) over the classes k_first <= k < K
 * (k_first = 1: --exclude_back without a copy): the min-max normalised, clipped distance sum and the min-max normalised
 * maximum softmax probability mixed through a sigmoid gate -- anomaly/eval_ood_traditional.py:302-305, :434-435 and
 * :447-448 of the reference (Coefficient_map(dis_sum, 0.2), lamda = 50; overwritten there by a leftover `conf = dis_sum`
 * at :450), and, with prob_logit = 1, clip = 1000, threshold = 0.3, the recipe test_embedding.py:366-369 keeps commented.
 * Per image b, every minimum and maximum over that image alone:
 *   s(p) = -(sum_k L_k(p)) + 0.0, set to clip where >= clip       m(p) = 1 / sum_k exp(L_k(p) - max_k L_k(p))   (prob_logit = 0)
 *   d(p) = (s(p) - min s) / (max s - min s)                            = max_k L_k(p)                            (prob_logit = 1)
 *   q(p) = (m(p) - min m) / (max m - min m)
 *   c(p) = 1 / (1 + exp(slope * (d(p) - threshold)))              conf(p) = c(p) d(p) + (1 - c(p)) q(p)
 * A constant s or m map normalises to 0/0 = NaN and conf is NaN on every pixel of that image, as numpy evaluates the
 * reference's statements (K - k_first = 1 without prob_logit is such a case).  An exp that overflows gives c = +0 and
 * conf = q.  work: 4 B + 2 B H W floats -- min s, max s, min m, max m per image, then the raw s and m maps.
 * Three launches ordered by the stream: the ranges' initialisation; pass 1 reads every logit from memory once (K - k_first
 * <= 16 keeps them in registers, more re-reads them from cache for the softmax denominator), writes s and m and reduces both
 * ranges per wave, per workgroup and with at most one atomic pair per map per workgroup (an atomic that could not change the
 * stored value is skipped); pass 2 reads the two maps and writes conf.
 * 16-byte loads and stores (4 pixels per lane) when H W % 4 == 0 and the pointers are 16-byte aligned, one float per lane
 * otherwise.  Atomic min / max do not depend on the order: bitwise reproducible, image b of a batch equals the image alone.
 * DML_EINVAL: a NULL pointer, B, K, H, W <= 0, k_first < 0 or k_first >= K.  DML_EUNSUPPORTED: K - k_first > 32, B > 65535
 * or B H W > 2^40.  Nothing is launched when a code is returned. */
int dml_dissum_msp_score(const float* logits, float* conf, float* work, int B, int K, int H, int W, int k_first,
                         float clip, float threshold, float slope, int prob_logit, void* stream);

/* Dense CRF with one spatial Gaussian pairwise term on logits[B,K,H,W] fp32 (NCHW, contiguous) over the classes
 * k_first <= k < K, C = K - k_first (k_first = 1: --exclude_back without a copy): anomaly/eval_ood_traditional.py:492-510 of
 * the reference (`--ood crf-gauss`: pydensecrf's unary_from_softmax, addPairwiseGaussian(sxy = 3, compat = 3), inference(100),
 * np.max over the classes).  Per image, y the row and x the column:
 *   U_c = -log(min(max(softmax_c(L), clip), 1))
 *   kx(d) = exp(-d^2 / (2 sx^2)) for |d| <= Rx = ceil(6 sx), else 0; ky, Ry alike with sy.  The tail cut at 6 sigma is 1.5e-8
 *   of the centre tap.  Sums run over the pixels inside the image (nothing is padded) and include the pixel itself (d = 0).
 *   nx(x) = 1 / sqrt(sum_x' kx(x - x')), ny(y) alike: densecrf's symmetric normalisation 1 / sqrt(sum_y',x' ky kx), factorised
 *   M_c(y,x) = ny(y) nx(x) sum_y' ky(y - y') ny(y') sum_x' kx(x - x') nx(x') Q_c(y',x')
 *   Q^0 = softmax_c(-U),  Q^{t+1} = softmax_c(-U + compat M(Q^t))              (PottsCompatibility(compat), inference(iters))
 *   conf(y,x) = max_c Q^iters_c(y,x) (higher = in-distribution); map(y,x) = argmax_c, the lowest index on a tie, counted from
 *   k_first.  map may be NULL.  iters = 0 gives the maximum of the re-normalised clipped softmax; compat = 0 gives the same
 *   bits after any number of steps.
 * work: dml_crf_gauss_workspace_bytes(B, C, H, W) = 4 (3 B C H W + H + W + 256) bytes -- U, Q and the row-filtered T, the two
 * tap tables (128 floats each), nx[W], ny[H]; nothing beyond it is written.  A negative DML_E* code for a shape
 * dml_crf_gauss rejects.
 * 1 + 2 iters launches, ordered by the stream alone (no cooperative grid, flag or atomic): the init launch (U, Q^0, tables);
 * per step a row launch (Q -> T through an LDS row tile with a halo of Rx) and a column launch (T with a halo of Ry through
 * LDS, a pixel's C messages in registers, softmax fused; the last one writes conf and map instead of Q).  Traffic per step,
 * in units of B C H W 4 bytes: Q read + T written + T read + U read + Q written = 5 (the column tile's halo rows, 2 Ry per
 * 32 rows at C <= 16 and per 16 rows above, are re-read from cache).  16-byte accesses in the row launch when W % 4 == 0
 * and work is 16-byte aligned, one float per lane otherwise and in the column launch.  Every sum has a fixed order: bitwise
 * reproducible, image b of a batch equals the image alone.
 * Two properties of the reference are deliberately not reproduced: (1) it calls DenseCRF2D(h, w, ch) although the
 * constructor takes (width, height, nlabels), so on a non-square frame it filters over scrambled neighbourhoods -- here y is
 * the row and x the column; (2) it takes ch from `scores`, not from `tmp_scores`, so with --exclude_back it stops at
 * setUnaryEnergy -- here k_first = 1 works.  pydensecrf's permutohedral lattice approximates the Gaussian filter that is
 * computed exactly here; the two do not agree digit for digit.
 * DML_EINVAL: logits, conf or work NULL, B, K, H, W <= 0, k_first < 0 or >= K, iters < 0, sx, sy or clip not > 0, clip >= 1.
 * DML_EUNSUPPORTED: K - k_first > 32, sx or sy > 8 (Rx, Ry <= 48), B > 65535 or B H W > 2^40.  Nothing is launched when a code
 * is returned. */
int64_t dml_crf_gauss_workspace_bytes(int B, int C, int H, int W);
int dml_crf_gauss(const float* logits, float* conf, int64_t* map, void* work, int B, int K, int H, int W, int k_first,
                  float sx, float sy, float compat, int iters, float clip, void* stream);

/* Reconstruction-consistency score (anomaly/eval_ood_rec.py:90-150 of the reference, `--ood rec`), in two calls.
 *
 * dml_rec_cosine: f1[s], f2[s], s < n (1..DML_REC_MAX_SCALES; host arrays of device pointers), are the decoder's pyramid concats
 * of the n resized copies of a frame and of its reconstruction, [B, h[s], w[s], C] channels last with a pixel pitch of ld[s] >= C
 * elements of `dtype` (h, w, ld: host arrays).  With R_s the bilinear resize to (Hq, Wq) of F.interpolate(mode='bilinear',
 * align_corners=False) (dml_bilinear_fwd's source-index arithmetic; a scale may be larger or smaller than the output):
 *   a_k = (1/n) sum_s R_s f_k[s]                u_k = a_k / max(|a_k|, 1e-12)                               (F.normalize, dim = C)
 *   cos[b,y,x] = sum_c (u_1 / max(|u_1|, 1e-8)) (u_2 / max(|u_2|, 1e-8))                                   (F.cosine_similarity)
 * A pixel where a_1 or a_2 is all zero gives exactly 0, never NaN.  cos: [B, Hq, Wq] fp32.
 * One launch, no workspace, nothing of size C Hq Wq: a workgroup owns 16 output pixels of one row, a thread 4 channels of each
 * 1024-channel chunk; the scales are summed per pixel and channel in fp32 registers (a source column, blended over the two source
 * rows, is loaded once per strip), and only the sums a_1.a_2, |a_1|^2, |a_2|^2 are kept, per thread in LDS, folded in a fixed order at
 * the end.  No atomics: bitwise reproducible.  Loads of 4 channels (16 bytes of fp32, 8 bytes of bf16) when every ld[s] % 4 == 0
 * and every pointer is aligned to that load, with the C % 4 last channels one by one; otherwise one channel per load.  Any C >= 1.
 * DML_EINVAL: a NULL pointer (the arrays, their first n entries, cos), n outside 1..DML_REC_MAX_SCALES, B, C, Hq, Wq, h[s], w[s] <= 0,
 * ld[s] < C, dtype neither DML_F32 nor DML_BF16.  DML_EUNSUPPORTED: B h[s] w[s] ld[s] (the kernel's element offsets are
 * 32-bit) or B Hq ceil(Wq / 16) >= 2^31.
 *
 * dml_rec_confidence: scores [B, K, H, W] fp32 (the multi-scale mean of the frame's scores), cos [B, Hq, Wq] -> conf [B, H, W]:
 *   msp = max_c scores[:, c], k_first <= c < K (prob_logit = 1: the reference's statement on its un-softmaxed scores)
 *       = max_c softmax_c(scores[:, k_first:])  (prob_logit = 0)
 *   conf = msp > threshold ? msp : (bilinear resize of cos to (H, W))[y, x]
 * One launch, one thread per pixel: the scores are read once, cos through its four taps.  k_first = 1 is --exclude_back without a
 * copy.  DML_EINVAL: a NULL pointer, B, K, H, W, Hq, Wq <= 0, k_first < 0 or >= K, K - k_first > 32.  DML_EUNSUPPORTED: B H W or
 * B Hq Wq > 2^40.  Nothing is launched when a code is returned. */
#define DML_REC_MAX_SCALES 8
int dml_rec_cosine(const void* const* f1, const void* const* f2, const int* h, const int* w, const int* ld, int n, int B, int C,
                   int dtype, float* cos, int Hq, int Wq, void* stream);
int dml_rec_confidence(const float* scores, const float* cos, float* conf, int B, int K, int H, int W, int Hq, int Wq, int k_first,
                       float threshold, int prob_logit, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DML loss = CE(-dist^2)/n + alpha * VAR/n (anomaly/models/models.py:42-78; live part of
 * utils/loss.py:34-42 is alpha = 0).
 * sums (device, double[4]) = { sum nll over valid px, #valid px, VAR, #correct }.
 * ---------------------------------------------------------------------------------------------- */
int dml_loss_fwd(const float* logits, const int64_t* labels, double* sums, float* block_partials,
                 int B, int K, int H, int W, int64_t ignore_index, void* stream);
/* loss = (sums[0]/sums[1] + alpha*sums[2]) / n_images  (written to *loss, device float).
 * n_images <= 0 (here and in dml_loss_bwd): the image count is read from sums[4] on the device -- the data-parallel
 * caller all-reduces {sums[0..3], local batch} in one 5-double message and never brings the count to the host. */
int dml_loss_finalize(const double* sums, float* loss, float alpha, float n_images, void* stream);
/* glogits = gout * d loss / d logits; gout is a device scalar. */
int dml_loss_bwd(const float* logits, const int64_t* labels, const double* sums, const float* gout,
                 float* glogits, int B, int K, int H, int W, int64_t ignore_index, float alpha,
                 float n_images, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Focal loss (utils/loss.py:7-23 of the reference) of logits[B,K,H,W] fp32 (NCHW, contiguous) and labels[B,H,W] int64.
 * A pixel is valid when its label != ignore_index; a valid label lies in [0, K) (the caller's duty, as for dml_loss_fwd).
 * On a valid pixel
 *   ce = logsumexp_k L_k - L_y      pt = exp(-ce)      u = 1 - pt      fl = alpha u^gamma ce
 *   m  = alpha (u^gamma + gamma pt ce u^(gamma-1))     d fl / d L_k = m (softmax_k - [k = y])
 * and fl = 0, gradient 0 on an ignored one.  Where u = 0 (pt rounds to 1): fl = 0, m = alpha for gamma = 0 and m = 0 for
 * gamma > 0 -- the analytic limit; the reference's autograd gives NaN there for 0 < gamma < 1.  u^0 = 1 for every u.
 * u is taken as -expm1(-ce), and the log-sum-exp keeps its largest term out of the sum (ce = max - L_y + log1p(rest)).
 * size_average != 0: loss = sum fl / (B H W) -- the divisor counts the ignored pixels too (the reference's .mean() of a
 * reduction='none' map) -- else loss = sum fl.  A batch with nothing valid has loss 0 and a zero gradient.
 * DML_EINVAL (all three; nothing is launched): a NULL pointer other than gout, B, H or W <= 0, K < 1, gamma < 0, alpha or
 * gamma not finite.
 * 16-byte loads and stores (4 pixels per lane) when H W % 4 == 0 and logits, labels (and glogits) are 16-byte aligned, one
 * float per lane otherwise; a pixel sees the same operations in the same order on either path (bitwise equal results).
 * 64-bit offsets, grid-stride loops, any K >= 1.  No atomics: bitwise reproducible.
 *
 * dml_focal_loss_fwd: one pass over the logits.  sums (device, double[4]) = { sum fl over valid px, #valid px,
 * #pixels = B H W, #correct (argmax == label) }: fp32 per lane, per-wave and per-workgroup partials in block_partials
 * (3 x 2048 floats, device), then one workgroup folds them in double in a fixed order.
 * ---------------------------------------------------------------------------------------------- */
int dml_focal_loss_fwd(const float* logits, const int64_t* labels, double* sums, float* block_partials,
                       int B, int K, int H, int W, int64_t ignore_index, float alpha, float gamma, void* stream);
/* *loss (device float) = size_average ? sums[0] / sums[2] : sums[0].  A data-parallel caller all-reduces the four doubles
 * first: the global pixel count travels in sums[2]. */
int dml_focal_loss_finalize(const double* sums, float* loss, int size_average, void* stream);
/* glogits[B,K,H,W] = gout * d loss / d logits; gout is a device scalar, NULL = 1.  The divisor is read from sums[2] on the
 * device.  K <= 16: a pixel's logits stay in registers between the log-sum-exp and the gradient (read from memory once);
 * more classes are read a second time. */
int dml_focal_loss_bwd(const float* logits, const int64_t* labels, const double* sums, const float* gout,
                       float* glogits, int B, int K, int H, int W, int64_t ignore_index, float alpha, float gamma,
                       int size_average, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature-distillation term (utils/loss.py:104-117 of the reference, main_distillation.py:427-434) of teacher features
 * t[B,H,W,Ct] and student features s[B,H,W,Cs], both fp32, channels last, dense, 1 <= Ct <= Cs <= 32, and labels[B,H,W] int64.
 * pad(t) is t with zero channels appended up to Cs (the reference appends one).  A pixel is masked in when its label != novel_id
 * -- a label equal to ignore_index is therefore masked in, as in the reference after its fill.  Per image i
 *   S_i = sum over masked-in pixels and all Cs channels of (s - pad(t))^2      cnt_i = #masked-in pixels
 *   dis = (1 / n) sum_{i: cnt_i > 0} S_i / cnt_i       d dis / d s[i,p,c] = 2 / (n cnt_i) (s - pad(t)) on a masked-in pixel, else 0
 * An image with cnt_i = 0 contributes 0 and has a zero gradient; the reference divides by zero there and returns NaN.
 * DML_EINVAL (nothing is launched): a NULL pointer other than t_logits, gout (and labels_out when t_logits is NULL), B, H or
 * W <= 0, Ct < 1, Ct > Cs, Cs > 32.  DML_EUNSUPPORTED (nothing is launched): B > 2048, or H W Cs >= 2^31 (offsets inside one
 * image are 32-bit, the image's base offset is 64-bit).
 * An image's student tensor is taken flat in groups of four floats, one lane each, with the group's (up to four, consecutive)
 * teacher floats and the one or two labels it touches: 16-byte loads and stores of s (and gs) when H W Cs % 4 == 0 and they are
 * 16-byte aligned, one float at a time otherwise; a group sees the same operations in the same order on either path (bitwise
 * equal results).  t, labels and t_logits need their natural alignment only.  Grid-stride loops.  No atomics: bitwise
 * reproducible.
 *
 * dml_distill_fwd: one pass.  With t_logits ([B,Ct,H,W], NCHW; the teacher's logits) not NULL it also writes
 *   labels_out[p] = labels_in[p] == ignore_index ? first maximal k of t_logits[:, p] : labels_in[p]
 * (the tie rule of dml_argmax_msp) and takes the mask from labels_out; labels_out may equal labels_in.  With t_logits == NULL the
 * labels are only read, ignore_index is unused and labels_out may be NULL.
 * Launch shape, min(.., 2048 / B) workgroups of 256 lanes per image: without t_logits a workgroup strides over the image's
 * ceil(H W Cs / 4) groups; with them over its tiles of 256 pixels -- a lane fills one pixel's label (label and logits coalesced
 * over the tile) and leaves it in LDS, then the tile's 64 Cs groups go over the lanes.
 * sums (device, double[2 B + 2]): sums[2 i] = S_i, sums[2 i + 1] = cnt_i, sums[2 B] = sum_{i: cnt_i > 0} S_i / cnt_i,
 * sums[2 B + 1] = B.  fp32 per lane, per-wave and per-workgroup partials in block_partials (2 x 2048 floats, device: a sum and
 * the bits of an integer count for each workgroup), then one workgroup folds them in double in a fixed order.
 * ---------------------------------------------------------------------------------------------- */
int dml_distill_fwd(const float* t_logits, const float* t, const float* s, const int64_t* labels_in, int64_t* labels_out,
                    double* sums, float* block_partials, int B, int Ct, int Cs, int H, int W, int64_t ignore_index,
                    int64_t novel_id, void* stream);
/* *dis (device float) = sums[2 B] / n.  n = n_images, or for n_images <= 0 (here and in dml_distill_bwd) sums[2 B + 1] read on the
 * device -- the convention of dml_loss_finalize: a data-parallel caller all-reduces the last two doubles and never brings the
 * count to the host. */
int dml_distill_finalize(const double* sums, int B, float n_images, float* dis, void* stream);
/* gs[B,H,W,Cs] = gout * d dis / d s: gout 2 / (n cnt_b) (s - pad(t)) on the masked-in pixels of an image with cnt_b > 0 and exactly
 * 0 elsewhere; every element is written.  labels: the ones the forward took its mask from (labels_out after a fill).  cnt_b is
 * read from sums[2 b + 1]; gout is a device scalar, NULL = 1. */
int dml_distill_bwd(const float* t, const float* s, const int64_t* labels, const double* sums, const float* gout, float* gs,
                    int B, int Ct, int Cs, int H, int W, int64_t novel_id, float n_images, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inter-class and centre terms of the metric loss (utils/loss.py:43-79 of the reference, behind its early return) of logits
 * L[B,K,H,W] (NCHW; minus the squared distances), features F[B,H,W,C] (channels last, dense) and labels[B,H,W] int64, all fp32,
 * 1 <= K <= 32, 1 <= C <= 32.  N = H W counts every pixel of an image, the ignored ones too (the reference's total_size, the
 * divisor of dml_loss_fwd's VAR).  A pixel is valid when its label != ignore_index; a valid label lies in [0, K) (the caller's
 * duty; a label outside is skipped like an ignored one, never used as an index).  For image i and class c with n_ic >= 1 pixels
 *   mu_ic    = (1 / n_ic) sum_{p: y_p = c} F[i,p,:]
 *   Inter_i  = (1 / N) sum_{valid p} sum_{k != y_p} L[i,k,p]
 *   Center_i = (1 / N) sum_{valid p} |F[i,p,:] - mu_{i,y_p}|^2
 *   term     = (beta sum_i Inter_i + gamma sum_i Center_i) / n                          n = images of the (global) batch
 *   d term / d L[i,k,p] = beta / (n N) on a valid pixel for k != y_p, else 0
 *   d term / d F[i,p,:] = 2 gamma / (n N) (F[i,p,:] - mu_{i,y_p}) on a valid pixel, else 0   (the part through mu cancels)
 * An image without a valid pixel contributes 0; a class of one pixel contributes 0 to Center.  The features are taken flat over
 * H W: the reference indexes features_in[i] ([H,W,C]) with flat pixel indices along its first dimension, which fails as soon as a
 * class has a pixel index >= H; the geometry it intended is the one computed here.
 * Center is summed from the deviations F - mu in a second read of the features, never as sum |F|^2 - n |mu|^2.
 * No atomics, in global memory or LDS: bitwise reproducible.  fp32 per lane, then double, in a fixed order.
 * DML_EINVAL (nothing is launched): a NULL pointer other than the optional ones named below, B, H or W <= 0, K < 1, C < 1, beta
 * or gamma not finite.  DML_EUNSUPPORTED (nothing is launched): K > 32, C > 32, B > 2048, H W C >= 2^31 (offsets inside an image
 * are 32-bit, the image's base offset is 64-bit).
 *
 * dml_metric_fwd.  logits NULL: Inter_i = 0 and the logits are not read; feats NULL: Center_i = 0, means and counts are not
 * written (and may be NULL) and C is only range-checked; not both NULL.
 *   means[B,K,C] fp32 = mu (0 for a class absent from the image), counts[B,K] int32 = n_ic: kept for the backward.
 *   sums (device, double[2 B + 3]): sums[2 i] = Inter_i, sums[2 i + 1] = Center_i, sums[2 B] = sum_i Inter_i,
 *   sums[2 B + 1] = sum_i Center_i, sums[2 B + 2] = B.
 *   work (device, 16-byte aligned): 2048 (2 + K (C + 1)) doubles.
 * Launches, each min(.., 2048 / B) workgroups of 256 lanes per image:
 *   1 (with feats) class sums: a wave takes 64 / CP pixels x CP channel lanes per step, CP = C rounded up to a power of two; a lane
 *     owns one column of a wave-private LDS table [K][64] (plus [K][64 / CP] counts; 4 K (64 + 64 / CP) 4 bytes per workgroup)
 *     and adds its float into the row of its pixel's label in program order; dword loads, 4 C bytes per pixel contiguous over
 *     the wave.  The workgroup folds its columns in double into work: K (C + 1) doubles per workgroup.
 *   2 (with feats) a wave per (class, channel) folds the workgroups' partials in double: means, counts.
 *   3 the image's means in LDS; the features flat in groups of four floats per lane (the mapping of dml_distill_fwd), fp32 sum of
 *     (F - mu)^2 per lane; then the logits, four consecutive pixels per lane, plane by plane, fp32 sum of the planes k != y.
 *     16-byte loads of F when H W C % 4 == 0 and F is 16-byte aligned, of L when H W % 4 == 0 and L is 16-byte aligned, one float
 *     at a time otherwise; the same lane takes the same elements in the same order on either path (bitwise equal results).
 *     Two doubles per workgroup into work.
 *   4 one workgroup folds those in double: a wave per image, then one wave over the images.
 * ---------------------------------------------------------------------------------------------- */
int dml_metric_fwd(const float* logits, const float* feats, const int64_t* labels, float* means, int32_t* counts, double* sums,
                   double* work, int B, int K, int C, int H, int W, int64_t ignore_index, void* stream);
/* *term (device float) = (beta sums[2 B] + gamma sums[2 B + 1]) / n.  n = n_images, or for n_images <= 0 (here and in
 * dml_metric_bwd) sums[2 B + 2] read on the device -- the convention of dml_loss_finalize and dml_distill_finalize: a data-parallel
 * caller all-reduces the last three doubles and never brings the count to the host. */
int dml_metric_finalize(const double* sums, int B, float beta, float gamma, float n_images, float* term, void* stream);
/* gfeats[B,H,W,C] (not NULL: feats and means required) = gout 2 gamma / (n N) (F - mu_y) on a valid pixel and exactly 0
 * elsewhere; every element is written.  glogits[B,K,H,W] (not NULL) += gout beta / (n N) on a valid pixel for k != y_p, in place:
 * one read-modify-write pass over the buffer dml_loss_bwd has written, from the labels alone; the own-class element of a valid
 * pixel is rewritten with its own value and a group of four pixels without a valid one is not touched.  Either may be NULL, not
 * both.  The two weights are rounded to fp32 once.  gout is a device scalar, NULL = 1.  16-byte accesses under the conditions
 * of the forward (gfeats and glogits 16-byte aligned as well). */
int dml_metric_bwd(const float* feats, const int64_t* labels, const float* means, const double* sums, const float* gout,
                   float* glogits, float* gfeats, int B, int K, int C, int H, int W, int64_t ignore_index, float beta, float gamma,
                   float n_images, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SGD with momentum and weight decay, torch semantics (main_embedding.py:385-388):
 *   g = gscale*g + wd*p ; v = mu*v + g ; p -= lr*v
 * ---------------------------------------------------------------------------------------------- */
int dml_sgd_step(float* p, const float* g, float* v, int64_t n, float lr, float momentum,
                 float weight_decay, float gscale, void* stream);

/* fill / scale helpers used by the host runtime */
int dml_fill_f32(float* p, int64_t n, float value, void* stream);
/* dst[i] = (dst_dtype) src[i] -- the bf16 plans keep the ASPP image-pooling branch (network/utils.py:318-329: a
 * BatchNorm over B x 256 x 1 x 1, i.e. over only B samples) in fp32 storage: with two near-equal samples a bf16-rounded
 * pre-normalisation value makes that layer's gradient blow up by up to 1/sqrt(eps). */
int dml_convert_dtype(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input pipeline on the device (the step before the path): the Cityscapes train
 * transform of main_embedding.py:148-157 -- random crop, colour jitter (brightness / contrast /
 * saturation in a random order), horizontal flip, ToTensor, Normalize (utils/ext_transforms.py:222-230,
 * 282-293, 313-322, 357-393, 469-504) -- on a batch of uint8 NHWC frames resident in HBM.  The random
 * draws stay on the host (utils/ext_transforms.py of this package mirrors the reference's order of
 * `random` calls); the kernels take one DmlAugSample per image.  Pixel arithmetic is Pillow's, bit for
 * bit: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; blend(a, b, f) = (uint8)(a + f*(b - a)) in
 * float32 without fused multiply-add, truncating, clipped to [0,255] when f is outside [0,1]; the
 * contrast pivot is int(mean(L over the crop, after the ops that precede it) + 0.5).
 * ---------------------------------------------------------------------------------------------- */
typedef struct DmlAugSample {
    int32_t i, j;       /* crop origin (row, column) in the source frame */
    int32_t flip;       /* horizontal flip (applied after the jitter, ext_transforms.py:229) */
    int32_t n_ops;      /* 0..3 jitter ops */
    int32_t op[3];      /* 0 brightness, 1 contrast, 2 saturation, in application order */
    float factor[3];
} DmlAugSample;
/* lsum[b] (device uint32, zeroed by the call) = sum of L over sample b's crop as seen by its contrast
 * op (after the ops that precede it); untouched semantics for samples without a contrast op. */
int dml_aug_contrast_sum(const uint8_t* img, const DmlAugSample* samples, uint32_t* lsum, int B, int H,
                         int W, int th, int tw, void* stream);
/* out_img[B,3,th,tw] fp32 = ((jittered, flipped crop)/255 - mean)/std; out_lbl[B,th,tw] int64 = the
 * same crop / flip of lbl[B,H,W] (uint8).  lsum from dml_aug_contrast_sum on the same stream. */
int dml_aug_apply(const uint8_t* img, const uint8_t* lbl, const DmlAugSample* samples,
                  const uint32_t* lsum, float* out_img, int64_t* out_lbl, int B, int H, int W, int th,
                  int tw, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                  void* stream);
/* Same, with the dataset's label encoding folded in (datasets/cityscapes.py:132-154 of the reference:
 * Cityscapes.encode_target = raw id -> train id -> unknown classes to 255, higher ids shifted down; pointwise, so it
 * commutes with crop / flip): out_lbl = lut[raw], out_lbl_true = lut_true[raw] (optional second output, the reference's
 * `target_true`).  lut / lut_true: device uint8[256]. */
int dml_aug_apply_encoded(const uint8_t* img, const uint8_t* lbl, const DmlAugSample* samples,
                          const uint32_t* lsum, float* out_img, int64_t* out_lbl, int B, int H, int W,
                          int th, int tw, float mean0, float mean1, float mean2, float std0, float std1,
                          float std2, const uint8_t* lut, const uint8_t* lut_true, int64_t* out_lbl_true,
                          void* stream);
/* The same table applied to a whole uint8 label tensor (validation path: no crop / jitter). */
int dml_label_encode(const uint8_t* raw, int64_t n, const uint8_t* lut, const uint8_t* lut_true,
                     int64_t* out, int64_t* out_true, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation input of the anomaly sub-project (anomaly/dataset.py:249-300 of the reference, ValDataset):
 * one decoded uint8 HWC RGB frame -> every scale of the multi-scale test, each equal bit for bit to
 * img_transform(imresize(img, (W_s, H_s), 'bilinear')).  The resampler is Pillow's 8-bit one
 * (libImaging/Resample.c): per-axis coefficients rounded to fixed point with 22 fraction bits (built on
 * the host in double), a horizontal pass over the source rows the vertical pass reads, rounded to uint8
 * (int32 accumulator from 2^21, (acc >> 22) clamped to [0,255]), then a vertical pass over that uint8
 * intermediate rounded the same way.  Normalisation in fp32 with true divisions: (v/255 - mean_c)/std_c.
 * ---------------------------------------------------------------------------------------------- */
#define DML_RESIZE_MAX_SCALES 8
typedef struct DmlResizeScale {
    float* out;                 /* [3, Hs, Ws] fp32 (the [1, 3, Hs, Ws] NCHW tensor of one scale)             */
    const int32_t* hbounds;     /* [Ws][2] (first source column, tap count) of each output column (device)     */
    const int32_t* hcoef;       /* [Ws][kh] fixed-point weights of those columns (device)                      */
    const int32_t* vbounds;     /* [Hs][2] (first source row, tap count) of each output row (device)           */
    const int32_t* vcoef;       /* [Hs][kv] (device)                                                          */
    int32_t Hs, Ws, kh, kv;
    int32_t band_rows;          /* output rows of one workgroup (a band of 64 columns)                         */
    int32_t lds_rows;           /* upper bound of the source rows any band of this scale reads (<= 256)        */
} DmlResizeScale;
/* All S (1..DML_RESIZE_MAX_SCALES) scales of frame img[h][w][3] (device uint8) in one launch.  `scales`
 * is a HOST array read during the call (its pointers are device pointers); the tables must have been
 * built for this (h, w).  DML_EUNSUPPORTED when a band needs more than 256 source rows. */
int dml_pil_resize_normalize(const uint8_t* img, int h, int w, const DmlResizeScale* scales, int S,
                             float mean0, float mean1, float mean2, float std0, float std1, float std2,
                             void* stream);
/* segm_transform of the same dataset: out[i] = (int64) segm[i] - 1 (an 'L' annotation; 0 becomes -1). */
int dml_segm_to_label(const uint8_t* segm, int64_t n, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scale / resize / pad / crop stage of the input pipeline (utils/ext_transforms.py:68-146, 328-428 of the
 * reference: ExtRandomScale, ExtScale, ExtResize, ExtCenterCrop, ExtRandomCrop with padding / pad_if_needed), on
 * a batch of uint8 NHWC frames of one size, a different scale per sample, one launch.  Per sample the kernel sees
 * a VIRTUAL image -- the frame resized to (Hs, Ws) -- and a th x tw output window whose origin in that image may
 * be negative and whose extent may pass its far edge; a pixel outside the virtual image is 0, in the image and in
 * the label (F.pad's default fill; Image.crop beyond the image).  Image: the 8-bit BILINEAR resampler described
 * above, restricted to the window.  Label: Pillow's NEAREST resize (Geometry.c, ImagingScaleAffine: the source
 * index is int(xo) of a double that starts at 0.5 * in / out and grows by in / out per output pixel), as a gather
 * through host-built index tables.  The window feeds dml_aug_contrast_sum / dml_aug_apply(_encoded) with
 * i = j = 0 and frame size (th, tw).
 * All tables of a batch live in ONE device int32 buffer `tables` (table_len elements); a sample names its own by
 * element offsets.  A window column / row outside the virtual image has tap count 0 (and label index -1); an axis
 * whose size does not change carries the identity (one tap of weight 2^22), which the arithmetic passes through
 * unchanged.  Rows above the virtual image carry the first inside row's first source row, rows below it the last
 * inside row's end, so that a band's source rows are [vbounds[first][0], vbounds[last][0] + vbounds[last][1]).
 * ---------------------------------------------------------------------------------------------- */
typedef struct DmlScaleWindow {
    int32_t hbounds;   /* [tw][2] (first source column, tap count) of each window column                   */
    int32_t hcoef;     /* [tw][kh] fixed-point weights (22 fraction bits)                                  */
    int32_t vbounds;   /* [th][2] (first source row, tap count) of each window row                         */
    int32_t vcoef;     /* [th][kv]                                                                          */
    int32_t lrow;      /* [th] source row of the label's window row, -1 outside                            */
    int32_t lcol;      /* [tw] source column of the label's window column, -1 outside                      */
    int32_t kh, kv;    /* widths of hcoef / vcoef                                                           */
} DmlScaleWindow;
/* img [B,H,W,3], lbl [B,H,W] (optional, with out_lbl) -> out_img [B,th,tw,3], out_lbl [B,th,tw], all uint8.
 * `samples`: DEVICE array of B.  band_rows: window rows per workgroup (a band of 64 columns); lds_rows: upper
 * bound of the source rows any band of any sample reads (<= 256, else DML_EUNSUPPORTED).  The caller validates
 * the tables against the frame before the upload; the kernel clamps every index it reads from them all the same
 * (an out-of-frame entry contributes nothing). */
int dml_aug_scale_window(const uint8_t* img, const uint8_t* lbl, const DmlScaleWindow* samples,
                         const int32_t* tables, int64_t table_len, uint8_t* out_img, uint8_t* out_lbl, int B,
                         int H, int W, int th, int tw, int band_rows, int lds_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pyramid-pooling decoder of the anomaly model (anomaly/models/models.py:586-687,
 * eval_ood_traditional.py:198-210 of the reference), inference only.
 * ---------------------------------------------------------------------------------------------- */
/* nn.AdaptiveAvgPool2d(S) on NHWC x[B,H,W,C] (pitch ldx) -> y[B,S,S,C] (dense): bin i = [floor(i*H/S), ceil((i+1)*H/S)).
 * ws: caller-owned fp32 workspace of dml_adaptive_avgpool_ws_elems(...) elements (two deterministic stages). */
int64_t dml_adaptive_avgpool_ws_elems(int B, int H, int W, int C, int S);
int dml_adaptive_avgpool_fwd(const void* x, void* y, float* ws, int B, int H, int W, int C, int ldx, int S,
                             int dtype, void* stream);
/* out[m][k] = -sum_c (emb[m][c] - protos[k][c])^2 for k < K on an NHWC fp32 embedding with Kp (<= 32) channels
 * (pad channels zero in emb and protos[K][Kp]); out channels K..Kp-1 = +0.0.  models.py:633-657: the distance is
 * taken at 1/8 resolution, BEFORE the upsample.  Rows of emb have pitch lde and rows of out pitch ldo (both >= Kp): columns Kp..lde-1
 * are never read and columns Kp..ldo-1 never written.  Scalar accesses: 4-byte alignment is enough.
 * DML_EINVAL: a NULL pointer, M <= 0, K <= 0, K > 33, Kp < 1, Kp > 32, K > Kp + 1, lde < Kp or ldo < Kp; DML_EUNSUPPORTED: K == Kp + 1
 * (one output channel per prototype inside the padded width). */
int dml_proto_dist_nhwc(const float* emb, const float* protos, float* out, int64_t M, int K, int Kp, int lde,
                        int ldo, void* stream);
/* dst[B,C,H,W] (+)= alpha * bilinear(src[B,h,w,ld] channels 0..C-1), align_corners = False -- F.interpolate to
 * segSize (models.py:659-668) with the multi-scale mean `scores = scores + scores_tmp / n` folded in. */
int dml_upsample_nhwc_to_nchw(const float* src, float* dst, int B, int h, int w, int ld, int C, int H, int W,
                              float alpha, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming segmentation metrics on the device (the step after the path):
 * hist[n*t + p] += 1 for every pixel with 0 <= t < n (and 0 <= p < n), the np.bincount of
 * metrics/stream_metrics.py:49-55.  hist is a device int64[n*n] that the call accumulates into;
 * n <= 64.  The scores of :57-83 are computed from the n x n matrix on the host.
 * ---------------------------------------------------------------------------------------------- */
int dml_confusion_update(const int64_t* label_true, const int64_t* label_pred, int64_t* hist,
                         int64_t count, int n_classes, void* stream);

/* Open-set prediction and its threshold sweep (anomaly/eval_ood_traditional.py:155-156,227-229,537-549,599-607 and
 * test_embedding.py:385-386 of the reference: `pred[conf < thre] = unknown`, scored per threshold), all T thresholds in one read of
 * conf, pred and label (device arrays of n elements).  thresholds (HOST float[T], 1 <= T <= 12, strictly increasing, no NaN) and
 * out_labels (HOST int64[n_out], 0 <= n_out <= 8, may be NULL when n_out = 0) are read before the call returns.  Per pixel p:
 *   l = label[p], and l = unknown_id if l is one of out_labels;  q = pred[p]
 *   j = #{i : conf[p] >= t_i}, compared in float32: a NaN confidence gives j = 0 (unknown at every threshold), +inf gives j = T, and
 *       a confidence equal to a threshold keeps its prediction
 *   if 0 <= l < n_classes and 0 <= q < n_classes: cube[l][q][j] += 1, else the pixel is skipped (dml_confusion_update's rule: 255
 *       and -1 drop out)
 *   if open_pred: open_pred[p] = conf[p] >= t_{write_idx} ? q : unknown_id, for every pixel, skipped ones included
 * cube is a device int64[n_classes][n_classes][T + 1] that the call accumulates into (integer atomics: exact, order-free, bitwise
 * reproducible).  The confusion matrix of threshold i (rows = label, columns = open-set prediction) follows on the host:
 *   M_i[l][q] = sum_{j > i} cube[l][q][j]                                               for q != unknown_id
 *   M_i[l][u] = sum_{j > i} cube[l][u][j] + sum_q sum_{j <= i} cube[l][q][j]            for u = unknown_id
 * cube may be NULL when open_pred is given (the prediction alone; label is then not read and may be NULL too).
 * 2 <= n_classes <= 33 (32 model classes and unknown: the largest cube, 33 * 33 * 13 uint32 counters, fits a workgroup's LDS),
 * 0 <= unknown_id < n_classes, write_idx in [0, T) whenever open_pred is given.  DML_EINVAL for any violation, for n < 0, for a NULL
 * conf, pred or thresholds, for a NULL label with a cube, and when cube and open_pred are both NULL.  Natural alignment is enough
 * (4 bytes for conf, 8 for the int64 arrays; DML_EALIGN otherwise).  n == 0 returns 0 and writes nothing; DML_EUNSUPPORTED
 * from about 2^41 pixels on (a workgroup's 32-bit counters).  No workspace, no host synchronisation. */
int dml_open_set_sweep(const float* conf, const int64_t* pred, const int64_t* label, int64_t n, const float* thresholds, int T,
                       const int64_t* out_labels, int n_out, int n_classes, int unknown_id, int64_t* cube, int64_t* open_pred,
                       int write_idx, void* stream);

/* The per-class ECDF certainty score (the recipe the reference keeps commented at DeepLabV3Plus-Pytorch/main_embedding.py:106-113,
 * 172-226,249-260 and test_embedding.py:155-163,361-364): fit, over calibration frames and per class, the empirical CDF E_cl of the
 * distance sums of the pixels labelled and predicted cl; score conf(p) = sum_cl softmax_cl(p) * Certainty(E_cl(s(p))).  An ECDF is kept
 * as a histogram over NB equal bins of [0, clip].  Definitions the three entry points share, each a float32 operation that
 * numpy.float32 restates bit for bit (the library is built without fast-math, and nothing below can be contracted):
 *   classes  k_first <= k < K, Kn = K - k_first (k_first = 1: --exclude_back without a copy)
 *   s(p)     = -(((L_kfirst(p) + L_kfirst+1(p)) + ...) + L_K-1(p)) + 0.0: ascending k from 0.0f, one rounding per addition
 *   inv_w    = (float)NB / clip, one division
 *   bin(s)   = NB - 1 where s >= clip; 0 where s <= 0; otherwise min((int)(s * inv_w), NB - 1), one product, truncated.
 *              A NaN s has no bin; +inf falls in NB - 1 and -inf in 0.
 *   pred(p)  = the first k in the range whose L_k(p) is maximal (dml_argmax_msp's rule), counted from k_first
 *
 * dml_ecdf_collect: logits[B,K,H,W] fp32 (NCHW, contiguous), labels[B,H,W] int64, hist device int64[Kn][NB].  For every pixel with
 * k_first <= label < K, label - k_first == pred and s not NaN: hist[label - k_first][bin(s)] += 1.  Every other pixel (255, -1, a class
 * below k_first, a wrong prediction) is skipped.  The call accumulates onto what hist holds: one call per calibration frame builds the
 * sample.  A workgroup counts in uint32 LDS cells sized by the actual Kn * NB and adds its non-zero cells with 64-bit integer atomics:
 * exact, order-free, bitwise reproducible; no workspace, no host synchronisation.  16-byte loads (4 pixels per lane) when
 * H W % 4 == 0 and logits and labels are 16-byte aligned, one pixel per lane otherwise; Kn <= 16 keeps a lane's planes in registers.
 * DML_EINVAL: a NULL pointer, B, K, H, W <= 0, k_first < 0 or >= K, clip <= 0 or not finite, NB < 1.  DML_EUNSUPPORTED: Kn > 32,
 * NB > 2048, Kn * NB > 32768 (128 KiB of LDS: 13 x 2048, 19 x 1024 and 32 x 1024 fit), B > 65535, B H W > 2^40, or an image so large
 * that a workgroup's 32-bit cells could overflow (from about 2^41 / B pixels on).  DML_EALIGN: logits off 4 bytes, labels or hist off 8.
 *
 * dml_ecdf_table: hist as above, table device float[NB][Kp] (bin-major: one pixel's Kn certainties are one contiguous row), Kp a
 * multiple of 4 and >= Kn, thresholds device float[Kn] (mode 1; may be NULL otherwise).  Per class cl, n_cl = sum_b hist[cl][b] and
 *   E_cl[b] = (float)((double)(hist[cl][0] + ... + hist[cl][b]) / (double)n_cl)        (the inclusive prefix sum)
 *   mode 0 (hard, main_embedding.py:107-109):    table[b][cl] = E_cl[b] > cut ? 1 : E_cl[b]
 *   mode 1 (sigmoid, test_embedding.py:156-161): table[b][cl] = 1 / (1 + expf(-slope * (E_cl[b] - E_cl[bin(thresholds[cl])])))
 *                                                 (a NaN threshold gives NaN)
 *   mode 2:                                       table[b][cl] = E_cl[b]
 * A class with n_cl = 0 has E_cl = 1 everywhere and, in every mode, the certainty 1: with no evidence its softmax weight passes
 * through.  Columns Kn..Kp-1 are written as 0.  One launch, Kp workgroups.
 * DML_EINVAL: a NULL hist or table, Kn < 1, NB < 1, clip <= 0 or not finite, Kp % 4 != 0, Kp < Kn, mode outside 0..2, mode 1 without
 * thresholds.  DML_EUNSUPPORTED: Kn > 32 or NB > 2048.  DML_EALIGN: hist off 8 bytes, thresholds off 4, table off 16.
 *
 * dml_ecdf_score: conf[B,H,W] fp32, conf(p) = (sum_k e_k(p) table[bin(s(p))][k - k_first]) / (sum_k e_k(p)) with
 * e_k(p) = expf(L_k(p) - max_k L_k(p)), both sums in ascending k: the softmax in the two-read form of dml_dissum_msp_score.  A NaN
 * s gives a NaN conf, and so does an infinite maximum (exp(inf - inf), as in float64).  The logits are read from memory once (Kn <= 20 keeps them in registers, more re-reads them from cache); a
 * table row is read as Kp / 4 16-byte vectors through the caches.  16-byte loads and stores of the maps when H W % 4 == 0 and logits
 * and conf are 16-byte aligned, one pixel per lane otherwise.  No atomics, no workspace: bitwise reproducible, and image b of a batch
 * equals the image alone.
 * DML_EINVAL: a NULL pointer, B, K, H, W <= 0, k_first < 0 or >= K, Kp % 4 != 0, Kp < Kn, clip <= 0 or not finite, NB < 1.
 * DML_EUNSUPPORTED: Kn > 32, NB > 2048, B > 65535 or B H W > 2^40.  DML_EALIGN: logits or conf off 4 bytes, table off 16 (its rows
 * are vectors).  Nothing is launched when any of the three returns a code. */
int dml_ecdf_collect(const float* logits, const int64_t* labels, int64_t* hist, int B, int K, int H, int W, int k_first, float clip,
                     int NB, void* stream);
int dml_ecdf_table(const int64_t* hist, float* table, const float* thresholds, int Kn, int Kp, int NB, float clip, int mode,
                   float cut, float slope, void* stream);
int dml_ecdf_score(const float* logits, const float* table, float* conf, int B, int K, int H, int W, int k_first, int Kp, float clip,
                   int NB, void* stream);

/* Few-shot prototype extraction (the recipe at test_embedding.py:413-425 of the reference: mean of features_out over
 * the pixels of one class): sums[c] (device double[C], zeroed by the call) = sum of feats[p][c] over pixels with
 * labels[p] == class_id, count (device uint64) = their number.  C <= 32. */
int dml_class_feature_sum(const float* feats, const int64_t* labels, int64_t n_px, int C, int64_t class_id,
                          double* sums, unsigned long long* count, void* stream);
/* The same for M <= 8 classes in one read of feats and labels: sums[m][c] (device double[M*C], zeroed by the call) and
 * counts[m] (device uint64[M]) for class_ids[m] (device int64[M]).  The ids must be distinct: the library cannot see
 * device memory, so the caller checks that (utils.extract_prototypes raises DML_EINVAL's error for duplicates).
 * Accumulation as in dml_class_feature_sum (fp32 within a thread, at most ceil(n_px / 262144) terms; double across
 * threads).  DML_EINVAL for a NULL pointer, n_px <= 0, C outside 1..32 or M outside 1..8. */
int dml_class_feature_sums(const float* feats, const int64_t* labels, int64_t n_px, int C, const int64_t* class_ids,
                           int M, double* sums, unsigned long long* counts, void* stream);

/* Pixel-level OOD measures (anomaly/anom_utils.py:25-78 as called by eval_ood_traditional.py:128-148):
 * scores = -conf; positives = pixels whose label is one of out_labels (host array, n_out <= 8), negatives = the
 * rest; pixels with mask[i] == 0 are left out (mask optional).  result (device double[5]) = { AUROC, AUPR,
 * FPR at recall_level, #positives, #negatives }; the three measures are NaN when either class is empty (the
 * reference prints a notice and skips the image).  work: >= dml_ood_workspace_bytes(n) bytes, 256-byte aligned.
 * Device-side radix sort + rank statistics; nothing is copied to the host. */
int64_t dml_ood_workspace_bytes(int64_t n);
int dml_ood_measures(const float* conf, const int64_t* seg_label, const uint8_t* mask, int64_t n,
                     const int64_t* out_labels, int n_out, double recall_level, void* work,
                     int64_t work_bytes, double* result, void* stream);

/* The same three measures over all pixels of a DATASET at once (pooled), where dml_ood_measures sorts one frame and the drivers
 * average per-frame figures: frames weigh by their anomaly area, a frame without an anomaly counts as negatives, one threshold serves
 * the whole set.  A sort needs every key resident; what streams is a histogram of the confidence over NB equal bins of [lo, hi].
 * state: device int64[2 * NB + 5] = hist[2][NB] (row 0: positives, the pixels whose label is one of out_labels; row 1: negatives), then
 * n_nan, n_below, n_above, n_masked, n_frames.  Plain additive memory: zero it to start, and two states over disjoint frames add
 * element-wise (which is how ranks combine them).
 *
 * dml_pooled_ood_update: one read of conf (fp32), seg_label (int64, compared as int64: ids below 0 and above 2^31 are fine) and the
 * optional mask (uint8, 0 = skip) of n pixels; out_labels is a HOST array of 1 <= n_out <= 8 ids, read before the call returns.  Per
 * pixel, in this order: mask 0 -> n_masked += 1 and nothing else; conf NaN -> n_nan += 1 and nothing else; otherwise n_below += 1 where
 * conf < lo, n_above += 1 where conf > hi (strictly outside, the infinities included: the user's sign that the range is wrong) and
 * hist[row][bin(conf)] += 1 with the bin bitwise defined in float32, one rounding per operation, nothing contracted:
 *   inv_w = (float)NB / (hi - lo)
 *   bin   = NB - 1 where conf >= hi; 0 where conf <= lo; otherwise min((int)((conf - lo) * inv_w), NB - 1), truncated
 * so -0.0 bins as 0.0, +inf falls in NB - 1 and -inf in 0.  n_frames += 1 per call with n > 0.  A workgroup counts in 2 NB + 4 uint32 LDS
 * cells and adds its non-zero cells with 64-bit integer atomics: exact, order-free, bitwise reproducible; no workspace, no host
 * synchronisation.  DML_EINVAL: a NULL conf, seg_label, out_labels or state, n < 0, NB outside 1..8192, n_out outside 1..8, lo, hi or
 * hi - lo (in float32) not finite, hi <= lo.  DML_EALIGN: conf off 4 bytes, seg_label or state off 8.  n == 0 returns 0 and touches
 * nothing.  DML_EUNSUPPORTED from about 2^40 pixels in one call on (a workgroup's 32-bit cells; the grid is capped at 256 workgroups).
 *
 * dml_pooled_ood_finalize: one workgroup; result (device double[8]) = { AUROC, AUPR, FPR at recall_level, P, N, tie mass, cut-off bin,
 * 0 }: the measures of anom_utils.get_measures on the quantised scores -bin.  With P_b, N_b the two rows, tp_b = P_0 + ... + P_b and
 * fp_b likewise (a pixel is flagged when its bin <= b):
 *   AUROC = (sum_b P_b (2 (N - fp_b) + N_b)) / (2 P N)      the numerator an exact 128-bit integer, rounded once
 *   AUPR  = sum_{b: P_b > 0} (P_b / P) (tp_b / (tp_b + fp_b))   float64, in a fixed ascending order (each of 256 lanes sums its
 *           ceil(NB / 256) consecutive bins in ascending b, then the 256 partial sums are added in ascending order): reproducible
 *   FPR   = fp / N of the candidate whose recall tp / P is nearest recall_level (the higher recall on a tie); candidates are the bins
 *           with P_b > 0: the highest of them with its own (tp_b = P, fp_b), every other with its tp_b and the negatives of the bins
 *           strictly below the next higher such bin (anom_utils.py:58-66); the cut-off bin is the candidate's bin
 *   tie mass T = (sum_b P_b N_b) / (P N): binning is monotone, so only pairs inside one bin can change order, and the unquantised
 *           pooled AUROC lies in [AUROC - T / 2, AUROC + T / 2]
 * P == 0 or N == 0: AUROC, AUPR, FPR and T are NaN, the cut-off bin -1, P and N as they are.  Exact up to 2^40 pixels.
 * DML_EINVAL: a NULL pointer, NB outside 1..8192, a NaN recall_level.  DML_EALIGN: state or result off 8 bytes. */
int dml_pooled_ood_update(const float* conf, const int64_t* seg_label, const uint8_t* mask, int64_t n, const int64_t* out_labels,
                          int n_out, float lo, float hi, int NB, int64_t* state, void* stream);
int dml_pooled_ood_finalize(const int64_t* state, int NB, double recall_level, double* result, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Native replay of a static launch list.  The reference dispatches one Python call per layer per step
 * (nn.Module.forward / autograd, network/utils.py:84-118, backbone/resnet.py:95-115); the drop-in's plan is a fixed
 * list of this library's own entry points, and dml_plan_run walks a packed copy of it in one call -- same launches,
 * same order, same streams, no interpreter in between.  HOST-side only: `ops` is a host array.
 *   fn      index from dml_plan_fn_id("dml_...") (any entry point above whose last parameter is the stream)
 *   args    one 64-bit word per parameter in declaration order, stream excluded: pointers and integers as they are
 *           (sign-extended), float in the low 32 bits, double as its 64 bits; host pointers to descriptors
 *           (DmlConvDesc / DmlWgradDesc) must stay valid for the call
 *   indirect bit k set: args[k] is the HOST address of an int32 read when the op is issued (the *nblocks that
 *           dml_bn_bwd_reduce wrote a few ops earlier)
 *   stream  0 = `stream`, 1 = `side_stream` (weight gradients); wait = 1: the side stream first waits for everything
 *           enqueued on `stream` so far (one of `events`, a ring of hipEvent_t, is recorded there)
 * Ops [first, last) are issued; on failure the index goes to *failed_op and the op's code is returned.
 * ---------------------------------------------------------------------------------------------- */
#define DML_PLAN_MAX_ARGS 24
typedef struct DmlPlanOp {
    int32_t fn, nargs;
    int32_t stream, wait;
    uint32_t indirect, reserved;
    uint64_t args[DML_PLAN_MAX_ARGS];
} DmlPlanOp;
int dml_plan_fn_id(const char* name);
int dml_plan_fn_nargs(int fn);
int dml_plan_run(const DmlPlanOp* ops, int first, int last, void* stream, void* side_stream, void* const* events,
                 int n_events, int* failed_op);
/* dml_plan_run with MARKS: after op marks[k] (ascending op indices; those outside [first, last) are ignored) mark_events[2 k] is
 * recorded on `stream` and, with a side stream, mark_events[2 k + 1] on `side_stream` (hipEvent_t handles).  Replaces the reference's
 * per-step nn.DataParallel reduce (main_embedding.py:425,438-439) together with dmlnet/parallel.py: the reducer's communication stream
 * waits on these events, so the host enqueues the whole backward in one call. */
int dml_plan_run_marks(const DmlPlanOp* ops, int first, int last, void* stream, void* side_stream, void* const* events,
                       int n_events, const int32_t* marks, int n_marks, void* const* mark_events, int* failed_op);

#ifdef __cplusplus
}
#endif
#endif /* DMLNET_HIP_H */
