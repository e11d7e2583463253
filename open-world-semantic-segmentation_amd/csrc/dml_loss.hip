// DML loss on the distance head's logits[B,K,H,W] (NCHW), for gfx950: cross entropy plus alpha times the mean distance to the own
// class' prototype, one fused forward pass and one backward pass that materialises d loss / d logits (head.hip's
// head_bwd_fused_c16_kernel is the train step's form of the latter).
//
// Replaces utils/loss.py:34-42 / anomaly/models/models.py:42-78 (per-image per-class Python loop with host round trips).
#include "common.h"

namespace {

// block partial = (sum nll, #valid, sum -logit_y over valid, #correct)
template <int PX>
__global__ __launch_bounds__(256) void loss_fwd_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ labels,
                                                       float* __restrict__ partials, int B, int K, int64_t HW,
                                                       int64_t ignore_index) {
    __shared__ float sh[4][4];
    float s_nll = 0.f, s_cnt = 0.f, s_var = 0.f, s_ok = 0.f;
    const int64_t gpi = HW / PX, total = (int64_t)B * gpi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / gpi, pix = (i - b * gpi) * PX;
        int64_t lab[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) lab[p] = labels[b * HW + pix + p];
        const float* src = logits + b * K * HW + pix;
        float mx[PX], own[PX], den[PX];
        int bi[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { mx[p] = -INFINITY; own[p] = 0.f; den[p] = 0.f; bi[p] = 0; }
        for (int k = 0; k < K; ++k) {
            float v[PX];
            load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                // online log-sum-exp: one pass over the K planes.  An equal value counts 1, not expf(v - mx): the same for finite
                // ties (expf(0) is 1) and right for -inf while mx is still -inf.  +inf is outside the contract: one +inf plane gives an
                // inf loss and two of them a finite denominator, where float64's inf - inf is NaN
                if (v[p] > mx[p]) { den[p] = den[p] * expf(mx[p] - v[p]) + 1.f; mx[p] = v[p]; bi[p] = k; }
                else den[p] += v[p] == mx[p] ? 1.f : expf(v[p] - mx[p]);      // -inf while mx is -inf: exp(-inf + inf) is NaN
                if ((int64_t)k == lab[p]) own[p] = v[p];
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if (lab[p] == ignore_index) continue;
            s_nll += (mx[p] - own[p]) + logf(den[p]);
            s_cnt += 1.f;
            s_var += -own[p];
            s_ok += (bi[p] == (int)lab[p]) ? 1.f : 0.f;
        }
    }
    // common.h's block_fold, written out: through the helper the compiler reorders this kernel's pixel loop
    s_nll = wave_sum(s_nll); s_cnt = wave_sum(s_cnt); s_var = wave_sum(s_var); s_ok = wave_sum(s_ok);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        sh[wv][0] = s_nll; sh[wv][1] = s_cnt; sh[wv][2] = s_var; sh[wv][3] = s_ok;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        partials[(int64_t)blockIdx.x * 4 + q] = sh[0][q] + sh[1][q] + sh[2][q] + sh[3][q];
    }
}
__global__ __launch_bounds__(256) void loss_sum_kernel(const float* __restrict__ partials, int nblocks,
                                                       double* sums, double inv_hw) {
    double acc[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)partials[(int64_t)i * 4 + q];
    block_fold(acc, [&](int q, double v) {
        if (q == 2) v *= inv_hw;       // VAR = sum_i (1/HW_i) sum_valid(-logit_y), HW_i identical in a batch
        sums[q] = v;
    });
}
__global__ void loss_finalize_kernel(const double* sums, float* loss, float alpha, float n_images) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double ce = sums[0] / sums[1];          // NaN when nothing is valid, as torch
        const double n = n_images > 0.f ? (double)n_images : sums[4];      // data parallel: global image count on the device
        *loss = (float)((ce + (double)alpha * sums[2]) / n);
    }
}
template <int PX>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ labels,
                                                       const double* __restrict__ sums,
                                                       const float* __restrict__ gout,
                                                       float* __restrict__ glogits, int B, int K, int64_t HW,
                                                       int64_t ignore_index, float alpha, float n_images_arg) {
    const float go = gout ? *gout : 1.f;
    const float n_images = n_images_arg > 0.f ? n_images_arg : (float)sums[4];
    const float w_ce = go / ((float)sums[1] * n_images);
    const float w_var = go * alpha / ((float)HW * n_images);
    const int64_t gpi = HW / PX, total = (int64_t)B * gpi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / gpi, pix = (i - b * gpi) * PX;
        int64_t lab[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) lab[p] = labels[b * HW + pix + p];
        const float* src = logits + b * K * HW + pix;
        float* dst = glogits + b * K * HW + pix;
        float mx[PX], den[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { mx[p] = -INFINITY; den[p] = 0.f; }
        for (int k = 0; k < K; ++k) {
            float v[PX];
            load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                if (v[p] > mx[p]) { den[p] = den[p] * expf(mx[p] - v[p]) + 1.f; mx[p] = v[p]; }
                else den[p] += v[p] == mx[p] ? 1.f : expf(v[p] - mx[p]);      // -inf while mx is -inf: exp(-inf + inf) is NaN
            }
        }
        float inv[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) inv[p] = lab[p] == ignore_index ? 0.f : w_ce / den[p];
        for (int k = 0; k < K; ++k) {
            float v[PX], g[PX];
            load_px<PX>(src + (int64_t)k * HW, v);                              // L2-resident re-read
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                g[p] = expf(v[p] - mx[p]) * inv[p];
                if ((int64_t)k == lab[p] && lab[p] != ignore_index) g[p] -= w_ce + w_var;
            }
            store_px<PX>(dst + (int64_t)k * HW, g);
        }
    }
}

}  // namespace

extern "C" int dml_loss_fwd(const float* logits, const int64_t* labels, double* sums, float* block_partials,
                            int B, int K, int H, int W, int64_t ignore_index, void* stream) {
    if (!logits || !labels || !sums || !block_partials || B <= 0 || K <= 0) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool v4 = (HW % 4) == 0;
    const int grid = grid_for(B * HW / (v4 ? 4 : 1), 256, MAX_BLOCKS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (v4)
        hipLaunchKernelGGL(loss_fwd_kernel<4>, dim3(grid), dim3(256), 0, st, logits, labels, block_partials, B, K, HW,
                           ignore_index);
    else
        hipLaunchKernelGGL(loss_fwd_kernel<1>, dim3(grid), dim3(256), 0, st, logits, labels, block_partials, B, K, HW,
                           ignore_index);
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, st, block_partials, grid, sums, 1.0 / (double)HW);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_loss_finalize(const double* sums, float* loss, float alpha, float n_images, void* stream) {
    if (!sums || !loss) return DML_EINVAL;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sums, loss,
                       alpha, n_images);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_loss_bwd(const float* logits, const int64_t* labels, const double* sums, const float* gout,
                            float* glogits, int B, int K, int H, int W, int64_t ignore_index, float alpha,
                            float n_images, void* stream) {
    if (!logits || !labels || !sums || !glogits) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (HW % 4 == 0)
        hipLaunchKernelGGL(loss_bwd_kernel<4>, dim3(grid_for(B * HW / 4, 256, 256 * 32)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), logits, labels, sums, gout, glogits, B, K, HW,
                           ignore_index, alpha, n_images);
    else
        hipLaunchKernelGGL(loss_bwd_kernel<1>, dim3(grid_for(B * HW, 256, 256 * 32)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), logits, labels, sums, gout, glogits, B, K, HW,
                           ignore_index, alpha, n_images);
    DML_LAUNCH_CHECK();
    return 0;
}
