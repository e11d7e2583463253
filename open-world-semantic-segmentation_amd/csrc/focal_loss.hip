// Focal loss of the reference's utils/loss.py:7-23 on logits[B,K,H,W] fp32 (NCHW): one fused forward pass, one fused backward
// pass that materialises d loss / d logits.  Definition, limits and normalisation: include/dmlnet_hip.h, DESIGN.md 7g.
#include "common.h"

#include <math.h>

namespace {

constexpr int FOCAL_KREG = 16;        // up to this many classes a pixel's logits are loaded up front and, in the backward, kept

typedef long long focal_ll2 __attribute__((ext_vector_type(2)));

template <int PX> __device__ __forceinline__ void focal_load_labels(const int64_t* p, int64_t (&lab)[PX]) {
    if constexpr (PX == 4) {
        const focal_ll2 a = reinterpret_cast<const focal_ll2*>(p)[0], b = reinterpret_cast<const focal_ll2*>(p)[1];
        lab[0] = a.x; lab[1] = a.y; lab[2] = b.x; lab[3] = b.y;
    } else {
        lab[0] = *p;
    }
}

// Online log-sum-exp that keeps the largest term out of the sum: sum_k exp(L_k) = exp(mx) * (1 + rest).  A pixel whose own
// class dominates then has ce = log1p(rest) with rest tiny, where log(1 + rest) would have rounded to 0.
// An equal value counts 1, not expf(v - mx): the same for finite ties and right for -inf while mx is still -inf; +inf logits are
// outside the contract (two of them give a finite sum where float64's inf - inf is NaN).
__device__ __forceinline__ void focal_lse_step(float v, float& mx, float& rest) {
#pragma clang fp contract(off)
    if (v > mx) { rest = (rest + 1.f) * expf(mx - v); mx = v; }       // the first class: (0 + 1) * exp(-inf) = 0
    else rest += v == mx ? 1.f : expf(v - mx);                        // -inf while mx is -inf: exp(-inf + inf) is NaN
}
__device__ __forceinline__ float focal_ce(float mx, float own, float rest) {
#pragma clang fp contract(off)
    return (mx - own) + log1pf(rest);                                 // >= 0: mx >= own and rest >= 0
}

// fl = alpha u^gamma ce and m = alpha (u^gamma + gamma pt ce u^(gamma-1)) = alpha u^gamma (1 + gamma pt ce / u), u = 1 - pt taken
// as -expm1(-ce) (no cancellation).  ce / u lies in [1, max(1, ce)] for every ce > 0, so nothing here overflows for a gamma
// below 1, where u^(gamma-1) alone would.  u = 0 (ce = 0): fl = 0 and m = alpha for gamma = 0, 0 for gamma > 0 -- the analytic
// limit (ce ~ u), where the reference's autograd has inf * 0.  u^0 = 1 for every u, as torch.pow.
__device__ __forceinline__ float focal_value(float ce, float alpha, float gamma) {
#pragma clang fp contract(off)
    if (gamma == 0.f) return alpha * ce;
    const float u = -expm1f(-ce);
    if (!(u > 0.f)) return 0.f;
    return alpha * powf(u, gamma) * ce;
}
__device__ __forceinline__ float focal_slope(float ce, float alpha, float gamma) {
#pragma clang fp contract(off)
    if (gamma == 0.f) return alpha;
    const float u = -expm1f(-ce);
    if (!(u > 0.f)) return 0.f;
    const float pt = expf(-ce);
    return alpha * powf(u, gamma) * (1.f + gamma * pt * (ce / u));
}

// block partial = (sum fl over valid, #valid, #correct).  REG: the K <= FOCAL_KREG loads of a pixel are all issued before the
// first is used (measured: 0.236 -> 0.214 ms at 16 x 16 x 768 x 768); unrolling the loop of the wider form by four cost
// occupancy and 3-7 % at 19 classes, so it stays rolled.  The arithmetic and its order are the same in both forms.
template <int PX, bool REG>
__global__ __launch_bounds__(256) void focal_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        float* __restrict__ partials, int B, int K, int64_t HW,
                                                        int64_t ignore_index, float alpha, float gamma) {
    float s_fl = 0.f, s_cnt = 0.f, s_ok = 0.f;
    const int64_t gpi = HW / PX, total = (int64_t)B * gpi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / gpi, pix = (i - b * gpi) * PX;
        int64_t lab[PX];
        focal_load_labels<PX>(labels + b * HW + pix, lab);
        const float* src = logits + b * K * HW + pix;
        float mx[PX], own[PX], rest[PX];
        int bi[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { mx[p] = -INFINITY; own[p] = 0.f; rest[p] = 0.f; bi[p] = 0; }
        auto step = [&](const float (&v)[PX], int k) {
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                if (v[p] > mx[p]) bi[p] = k;
                focal_lse_step(v[p], mx[p], rest[p]);
                if ((int64_t)k == lab[p]) own[p] = v[p];
            }
        };
        if constexpr (REG) {
            float reg[FOCAL_KREG][PX];
#pragma unroll
            for (int k = 0; k < FOCAL_KREG; ++k)
                if (k < K) load_px<PX>(src + (int64_t)k * HW, reg[k]);
#pragma unroll
            for (int k = 0; k < FOCAL_KREG; ++k)
                if (k < K) step(reg[k], k);
        } else {
            for (int k = 0; k < K; ++k) {
                float v[PX];
                load_px<PX>(src + (int64_t)k * HW, v);
                step(v, k);
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if (lab[p] == ignore_index) continue;
            s_fl += focal_value(focal_ce(mx[p], own[p], rest[p]), alpha, gamma);
            s_cnt += 1.f;
            s_ok += (bi[p] == (int)lab[p]) ? 1.f : 0.f;
        }
    }
    const float s[3] = {s_fl, s_cnt, s_ok};
    block_fold(s, [&](int q, float v) { partials[(int64_t)blockIdx.x * 3 + q] = v; });
}

// the double fold of the workgroups' partials, in a fixed order; sums = { sum fl, #valid, #pixels, #correct }
__global__ __launch_bounds__(256) void focal_sum_kernel(const float* __restrict__ partials, int nblocks, double* sums,
                                                        double pixels) {
    double acc[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x)
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += (double)partials[(int64_t)i * 3 + q];
    block_fold(acc, [&](int q, double v) { sums[q == 2 ? 3 : q] = v; });
    if (threadIdx.x == 3) sums[2] = pixels;
}

__global__ void focal_finalize_kernel(const double* sums, float* loss, int size_average) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *loss = (float)(size_average ? sums[0] / sums[2] : sums[0]);          // the divisor counts the ignored pixels: never 0
}

// REG: the K <= FOCAL_KREG logits of a pixel stay in registers between the log-sum-exp and the gradient (read once); otherwise
// the gradient loop reads them again.  Either way each pixel sees the same operations in the same order.
template <int PX, bool REG>
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        const double* __restrict__ sums, const float* __restrict__ gout,
                                                        float* __restrict__ glogits, int B, int K, int64_t HW,
                                                        int64_t ignore_index, float alpha, float gamma, int size_average) {
    const float go = gout ? *gout : 1.f;
    const float w = size_average ? (float)((double)go / sums[2]) : go;
    const int64_t gpi = HW / PX, total = (int64_t)B * gpi;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / gpi, pix = (i - b * gpi) * PX;
        int64_t lab[PX];
        focal_load_labels<PX>(labels + b * HW + pix, lab);
        const float* src = logits + b * K * HW + pix;
        float* dst = glogits + b * K * HW + pix;
        float mx[PX], own[PX], rest[PX], wm[PX], coef[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { mx[p] = -INFINITY; own[p] = 0.f; rest[p] = 0.f; }
        float reg[REG ? FOCAL_KREG : 1][PX];
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < FOCAL_KREG; ++k)
                if (k < K) load_px<PX>(src + (int64_t)k * HW, reg[k]);
#pragma unroll
            for (int k = 0; k < FOCAL_KREG; ++k)
                if (k < K) {
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        focal_lse_step(reg[k][p], mx[p], rest[p]);
                        if ((int64_t)k == lab[p]) own[p] = reg[k][p];
                    }
                }
        } else {
            for (int k = 0; k < K; ++k) {
                float v[PX];
                load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    focal_lse_step(v[p], mx[p], rest[p]);
                    if ((int64_t)k == lab[p]) own[p] = v[p];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
#pragma clang fp contract(off)
            wm[p] = w * focal_slope(focal_ce(mx[p], own[p], rest[p]), alpha, gamma);
            coef[p] = wm[p] / (1.f + rest[p]);
        }
        auto grad = [&](const float (&v)[PX], int k) {
#pragma clang fp contract(off)
            float g[PX];
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                g[p] = expf(v[p] - mx[p]) * coef[p];
                if ((int64_t)k == lab[p]) g[p] -= wm[p];
                if (lab[p] == ignore_index) g[p] = 0.f;
            }
            store_px<PX>(dst + (int64_t)k * HW, g);
        };
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < FOCAL_KREG; ++k)
                if (k < K) grad(reg[k], k);
        } else {
            for (int k = 0; k < K; ++k) {
                float v[PX];
                load_px<PX>(src + (int64_t)k * HW, v);                       // cache-resident re-read
                grad(v, k);
            }
        }
    }
}

bool focal_params_ok(float alpha, float gamma) { return isfinite(alpha) && isfinite(gamma) && gamma >= 0.f; }

}  // namespace

extern "C" int dml_focal_loss_fwd(const float* logits, const int64_t* labels, double* sums, float* block_partials, int B,
                                  int K, int H, int W, int64_t ignore_index, float alpha, float gamma, void* stream) {
    if (!logits || !labels || !sums || !block_partials || B <= 0 || K < 1 || H <= 0 || W <= 0 || !focal_params_ok(alpha, gamma))
        return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool v4 = (HW % 4) == 0 && aligned16(logits, labels);
    const int grid = grid_for(B * HW / (v4 ? 4 : 1), 256, MAX_BLOCKS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool reg = K <= FOCAL_KREG;
#define FOCAL_FWD(PX, REG)                                                                                              \
    hipLaunchKernelGGL((focal_fwd_kernel<PX, REG>), dim3(grid), dim3(256), 0, st, logits, labels, block_partials, B, K, HW, \
                       ignore_index, alpha, gamma)
    if (v4 && reg) FOCAL_FWD(4, true);
    else if (v4) FOCAL_FWD(4, false);
    else if (reg) FOCAL_FWD(1, true);
    else FOCAL_FWD(1, false);
#undef FOCAL_FWD
    hipLaunchKernelGGL(focal_sum_kernel, dim3(1), dim3(256), 0, st, block_partials, grid, sums, (double)B * (double)HW);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_focal_loss_finalize(const double* sums, float* loss, int size_average, void* stream) {
    if (!sums || !loss) return DML_EINVAL;
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sums, loss,
                       size_average);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_focal_loss_bwd(const float* logits, const int64_t* labels, const double* sums, const float* gout,
                                  float* glogits, int B, int K, int H, int W, int64_t ignore_index, float alpha, float gamma,
                                  int size_average, void* stream) {
    if (!logits || !labels || !sums || !glogits || B <= 0 || K < 1 || H <= 0 || W <= 0 || !focal_params_ok(alpha, gamma))
        return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool v4 = (HW % 4) == 0 && aligned16(logits, labels, glogits);
    const bool reg = K <= FOCAL_KREG;
    const int grid = grid_for(B * HW / (v4 ? 4 : 1), 256, MAX_BLOCKS);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define FOCAL_BWD(PX, REG)                                                                                              \
    hipLaunchKernelGGL((focal_bwd_kernel<PX, REG>), dim3(grid), dim3(256), 0, st, logits, labels, sums, gout, glogits, B, K, \
                       HW, ignore_index, alpha, gamma, size_average)
    if (v4 && reg) FOCAL_BWD(4, true);
    else if (v4) FOCAL_BWD(4, false);
    else if (reg) FOCAL_BWD(1, true);
    else FOCAL_BWD(1, false);
#undef FOCAL_BWD
    DML_LAUNCH_CHECK();
    return 0;
}
