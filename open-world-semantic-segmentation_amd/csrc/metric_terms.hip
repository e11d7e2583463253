// Inter-class and centre terms of the metric loss (the reference's utils/loss.py:43-79, behind its early return) on logits
// L[B,K,H,W] (NCHW), features F[B,H,W,C] (channels last) and labels[B,H,W]: per image and class the mean feature (a segmented
// reduction), the sum of the other classes' logits, the squared deviations from the own class mean, and the gradients of both.
// Definition, limits and normalisation: include/dmlnet_hip.h, DESIGN.md 7k.
//
// Forward, up to four launches (the first two and the centre loop only with features, the inter loop only with logits):
//   metric_class_sums_kernel  grid (bpi, B): a wave takes 64 / CP pixels x CP channel lanes per step (CP = C rounded up to a power
//       of two), the waves and workgroups of an image striding over its pixels.  Lane (slot, c) owns column `lane` of a
//       wave-private LDS table [K][64] and adds its float into the row of its pixel's label; the lane of channel 0 counts the
//       pixel in [K][64 / CP].  A column has one owner, so there is no atomic and the order of a column's additions is the
//       lane's program order.  Four steps are loaded before the first is added.  The workgroup then folds its 4 x 64 / CP
//       columns per (class, channel) in double, in a fixed order, into partials[workgroup][K (C + 1)].
//       The lanes keep one channel for the whole launch, so these are dword loads, 4 CP bytes per pixel contiguous over the wave
//       (256 B per load instruction for C = 16 and 32); the other launches move 16 bytes per lane.
//   metric_means_kernel       grid (ceil(K C / 4), B): a wave per (class, channel) folds the workgroups' partials in double.
//   metric_terms_kernel       grid (bpi, B): the image's means in LDS; the features a second time, flat in groups of four floats
//       per lane (the mapping of csrc/distill_loss.hip), d = F - mean of the own class, sum d^2; then the logits, four
//       consecutive pixels per lane, plane by plane, summing the planes that are not the pixel's own class.
//   metric_fold_kernel        one workgroup: the double fold of the workgroups' (centre, inter) partials, per image, then over
//       the images.
// Backward: metric_gfeats_kernel (the groups again, w (F - mean)) and metric_glogits_kernel (four pixels per lane, plane by plane,
// read - add - write).  The 16-byte and the one-float forms of a load or store take the same group on the same lane and do the same
// operations in the same order: the same bits.
#include "common.h"

#include <math.h>

namespace {

// MAX_BLOCKS: most workgroups of a forward launch; work holds 2 + K (C + 1) doubles for each.  MAXC: classes and channels at most.

__device__ __forceinline__ bool metric_valid(int64_t lab, int64_t ignore_index, int K) {
    return lab != ignore_index && (uint64_t)lab < (uint64_t)K;      // never an index outside a [K] table
}

// ---- per workgroup: sum of the features and number of pixels of every class
template <int CP>
__global__ __launch_bounds__(256) void metric_class_sums_kernel(const float* __restrict__ feats, const int64_t* __restrict__ labels,
                                                                double* __restrict__ partials, int K, int C, int64_t HW,
                                                                int64_t ignore_index) {
    extern __shared__ float metric_lds[];                  // 4 waves x [K][64] floats, then 4 waves x [K][PPW] counts
    constexpr int PPW = 64 / CP;                           // pixels of a wave's step
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, slot = lane / CP, c = lane % CP;
    float* tab = metric_lds + wv * K * 64;
    uint32_t* cnts = reinterpret_cast<uint32_t*>(metric_lds + 4 * K * 64);
    uint32_t* cnt = cnts + wv * K * PPW;
    for (int k = 0; k < K; ++k) {
        tab[k * 64 + lane] = 0.f;
        if (c == 0) cnt[k * PPW + slot] = 0u;
    }
    const bool active = c < C;
    const int64_t b = blockIdx.y;
    const float* fimg = feats + b * HW * C;
    const int64_t* limg = labels + b * HW;
    const uint64_t px = (uint64_t)HW, stride = (uint64_t)gridDim.x * 4u * PPW;
    for (uint64_t p0 = ((uint64_t)blockIdx.x * 4u + wv) * PPW + slot; p0 < px; p0 += 4u * stride) {
        int64_t lab[4];
        float f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t p = p0 + u * stride;
            const bool in = p < px;
            lab[u] = in ? limg[p] : (int64_t)-1;            // -1: not a class whatever ignore_index is
            f[u] = in && active ? fimg[p * (uint32_t)C + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!metric_valid(lab[u], ignore_index, K)) continue;
            const int k = (int)lab[u];
            if (active) tab[k * 64 + lane] += f[u];
            if (c == 0) cnt[k * PPW + slot] += 1u;
        }
    }
    __syncthreads();
    double* out = partials + ((int64_t)b * gridDim.x + blockIdx.x) * (K * (C + 1));
    for (int e = threadIdx.x; e < K * C; e += 256) {
        const int k = e / C, cc = e - k * C;
        double s = 0;
        for (int w = 0; w < 4; ++w)
            for (int sl = 0; sl < PPW; ++sl) s += (double)metric_lds[(w * K + k) * 64 + sl * CP + cc];
        out[e] = s;
    }
    for (int k = threadIdx.x; k < K; k += 256) {
        uint32_t n = 0;
        for (int w = 0; w < 4; ++w)
            for (int sl = 0; sl < PPW; ++sl) n += cnts[(w * K + k) * PPW + sl];
        out[K * C + k] = (double)n;
    }
}

// ---- a wave per (class, channel): the workgroups' partials in double, mean = sum / count (0 for an absent class)
__global__ __launch_bounds__(256) void metric_means_kernel(const double* __restrict__ partials, int bpi, int K, int C,
                                                           float* __restrict__ means, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= K * C) return;                                // the whole wave
    const int64_t b = blockIdx.y;
    const int k = e / C, E = K * (C + 1);
    const double* base = partials + b * bpi * E;
    double s = 0, n = 0;
    for (int j = lane; j < bpi; j += 64) {
        s += base[(int64_t)j * E + e];
        n += base[(int64_t)j * E + K * C + k];
    }
    s = wave_sum_d(s);
    n = wave_sum_d(n);
    if (lane == 0) {
        means[b * K * C + e] = n > 0 ? (float)(s / n) : 0.f;
        if (e == k * C) counts[b * K + k] = (int32_t)n;
    }
}

// One group of four features: d[k] = F - mean of the own class, m[k] = the element is there and its pixel is valid.
// mu: the image's means [K][C] in LDS.
template <bool VEC>
__device__ __forceinline__ void metric_group(const float* fimg, const int64_t* limg, const float* mu, uint32_t g, uint32_t n_img,
                                             int K, int C, const FastDiv& divC, int64_t ignore_index, float (&d)[4], bool (&m)[4]) {
#pragma clang fp contract(off)
    const uint32_t e0 = 4u * g, left = n_img - e0;
    uint32_t pix = fdiv(e0, divC);
    int c = (int)(e0 - pix * (uint32_t)C);
    float v[4];
    load4_tail<VEC>(fimg + e0, left, v);
    int row = 0;
    bool in = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool there = VEC || (uint32_t)k < left;
        if (there && (k == 0 || c == 0)) {
            const int64_t lab = limg[pix];
            in = metric_valid(lab, ignore_index, K);
            row = in ? (int)lab * C : 0;
        }
        m[k] = there && in;
        d[k] = m[k] ? v[k] - mu[row + c] : 0.f;
        if (++c == C) { c = 0; ++pix; }
    }
}

// ---- per workgroup: (sum of squared deviations, sum of the other classes' logits) over its share of the image
template <bool VECF, bool VECL>
__global__ __launch_bounds__(256) void metric_terms_kernel(const float* __restrict__ logits, const float* __restrict__ feats,
                                                           const int64_t* __restrict__ labels, const float* __restrict__ means,
                                                           double* __restrict__ partials, int K, int C, int64_t HW, FastDiv divC,
                                                           int64_t ignore_index) {
#pragma clang fp contract(off)
    __shared__ float mu[MAXC * MAXC];
    const int64_t b = blockIdx.y;
    const int64_t* limg = labels + b * HW;
    float center = 0.f, inter = 0.f;
    if (feats != nullptr) {
        for (int i = threadIdx.x; i < K * C; i += 256) mu[i] = means[b * K * C + i];
        __syncthreads();
        const float* fimg = feats + b * HW * C;
        const uint32_t n_img = (uint32_t)(HW * C), groups = (n_img + 3u) / 4u;
        for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256u) {
            float d[4];
            bool m[4];
            metric_group<VECF>(fimg, limg, mu, (uint32_t)g, n_img, K, C, divC, ignore_index, d, m);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (m[k]) center = center + d[k] * d[k];
        }
    }
    if (logits != nullptr) {
        const float* limg_l = logits + b * K * HW;
        const uint32_t px = (uint32_t)HW, quads = (px + 3u) / 4u;
        for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * 256u) {
            const uint32_t p = 4u * (uint32_t)q, left = px - p;
            int lab[4];
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t y = (uint32_t)j < left ? limg[p + j] : (int64_t)-1;
                lab[j] = metric_valid(y, ignore_index, K) ? (int)y : -1;
            }
            if (lab[0] < 0 && lab[1] < 0 && lab[2] < 0 && lab[3] < 0) continue;      // no valid pixel: its logits are not read
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                float v[4];
                load4_tail<VECL>(limg_l + (int64_t)k * HW + p, left, v);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k != lab[j]) s[j] = s[j] + v[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (lab[j] >= 0) inter = inter + s[j];
        }
    }
    const float s[2] = {center, inter};
    block_fold(s, [&](int q, float v) { partials[((int64_t)b * gridDim.x + blockIdx.x) * 2 + q] = (double)v; });
}

// ---- the double fold of the (centre, inter) partials in a fixed order: a wave per image, then one wave over the images
__global__ __launch_bounds__(256) void metric_fold_kernel(const double* __restrict__ partials, int B, int bpi, double inv_hw,
                                                          double* __restrict__ sums) {
    __shared__ double img[2 * MAX_BLOCKS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = wv; i < B; i += 4) {
        double ce = 0, in = 0;
        for (int j = lane; j < bpi; j += 64) {
            ce += partials[((int64_t)i * bpi + j) * 2];
            in += partials[((int64_t)i * bpi + j) * 2 + 1];
        }
        ce = wave_sum_d(ce);
        in = wave_sum_d(in);
        if (lane == 0) {
            img[2 * i] = sums[2 * i] = in * inv_hw;
            img[2 * i + 1] = sums[2 * i + 1] = ce * inv_hw;
        }
    }
    __syncthreads();
    if (wv == 0) {
        double ce = 0, in = 0;
        for (int i = lane; i < B; i += 64) { in += img[2 * i]; ce += img[2 * i + 1]; }
        ce = wave_sum_d(ce);
        in = wave_sum_d(in);
        if (lane == 0) { sums[2 * B] = in; sums[2 * B + 1] = ce; sums[2 * B + 2] = (double)B; }
    }
}

__global__ void metric_finalize_kernel(const double* sums, int B, float beta, float gamma, float n_images, float* term) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double n = n_images > 0.f ? (double)n_images : sums[2 * B + 2];
        *term = (float)(((double)beta * sums[2 * B] + (double)gamma * sums[2 * B + 1]) / n);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void metric_gfeats_kernel(const float* __restrict__ feats, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ means, const double* __restrict__ sums,
                                                            const float* __restrict__ gout, float* __restrict__ gfeats, int B, int K,
                                                            int C, int64_t HW, FastDiv divC, int64_t ignore_index, float gamma,
                                                            float n_images) {
#pragma clang fp contract(off)
    __shared__ float mu[MAXC * MAXC];
    const int64_t b = blockIdx.y;
    for (int i = threadIdx.x; i < K * C; i += 256) mu[i] = means[b * K * C + i];
    __syncthreads();
    const double n = n_images > 0.f ? (double)n_images : sums[2 * B + 2];
    const double go = gout ? (double)*gout : 1.0;
    const float w = (float)(go * 2.0 * (double)gamma / (n * (double)HW));
    const float* fimg = feats + b * HW * C;
    const int64_t* limg = labels + b * HW;
    float* gimg = gfeats + b * HW * C;
    const uint32_t n_img = (uint32_t)(HW * C), groups = (n_img + 3u) / 4u;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256u) {
        float d[4], r[4];
        bool m[4];
        metric_group<VEC>(fimg, limg, mu, (uint32_t)g, n_img, K, C, divC, ignore_index, d, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = m[k] ? w * d[k] : 0.f;
        store4_tail<VEC>(gimg + 4u * (uint32_t)g, n_img - 4u * (uint32_t)g, r);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void metric_glogits_kernel(const int64_t* __restrict__ labels, const double* __restrict__ sums,
                                                             const float* __restrict__ gout, float* __restrict__ glogits, int B,
                                                             int K, int64_t HW, int64_t ignore_index, float beta, float n_images) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const double n = n_images > 0.f ? (double)n_images : sums[2 * B + 2];
    const double go = gout ? (double)*gout : 1.0;
    const float w = (float)(go * (double)beta / (n * (double)HW));
    const int64_t* limg = labels + b * HW;
    float* gimg = glogits + b * K * HW;
    const uint32_t px = (uint32_t)HW, quads = (px + 3u) / 4u;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * 256u) {
        const uint32_t p = 4u * (uint32_t)q, left = px - p;
        int lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t y = (uint32_t)j < left ? limg[p + j] : (int64_t)-1;
            lab[j] = metric_valid(y, ignore_index, K) ? (int)y : -1;
        }
        if (lab[0] < 0 && lab[1] < 0 && lab[2] < 0 && lab[3] < 0) continue;      // nothing to add: the four pixels stay untouched
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            float v[4];
            load4_tail<VEC>(gimg + (int64_t)k * HW + p, left, v);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (lab[j] >= 0 && lab[j] != k) v[j] = v[j] + w;
            store4_tail<VEC>(gimg + (int64_t)k * HW + p, left, v);
        }
    }
}

int metric_shape_check(int B, int K, int C, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || K < 1 || C < 1) return DML_EINVAL;
    if (K > MAXC || C > MAXC || B > MAX_BLOCKS || (int64_t)H * W * C >= ((int64_t)1 << 31)) return DML_EUNSUPPORTED;
    return 0;
}
int metric_cp(int C) {
    int cp = 1;
    while (cp < C) cp *= 2;
    return cp;
}
int metric_bpi_sums(int B, int64_t HW, int C) { return grid_for(HW, 4 * (64 / metric_cp(C)), MAX_BLOCKS / B); }
int metric_bpi_flat(int B, int64_t HW, int C) { return grid_for((HW * C + 3) / 4, 256, MAX_BLOCKS / B); }
int metric_bpi_quads(int B, int64_t HW) { return grid_for((HW + 3) / 4, 256, MAX_BLOCKS / B); }
bool metric_vec(int64_t n_img, const void* a, const void* b) { return n_img % 4 == 0 && aligned16(a, b); }

}  // namespace

extern "C" int dml_metric_fwd(const float* logits, const float* feats, const int64_t* labels, float* means, int32_t* counts,
                              double* sums, double* work, int B, int K, int C, int H, int W, int64_t ignore_index, void* stream) {
    if (!labels || !sums || !work || (!logits && !feats) || (feats && (!means || !counts))) return DML_EINVAL;
    if (const int rc = metric_shape_check(B, K, C, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* term_partials = work;
    double* class_partials = work + 2 * MAX_BLOCKS;
    if (feats) {
        const int bpi = metric_bpi_sums(B, HW, C), cp = metric_cp(C);
        const size_t lds = (size_t)4 * K * (64 + 64 / cp) * sizeof(float);
#define METRIC_SUMS(CP)                                                                                                        \
    hipLaunchKernelGGL((metric_class_sums_kernel<CP>), dim3(bpi, B), dim3(256), lds, st, feats, labels, class_partials, K, C, HW, \
                       ignore_index)
        switch (cp) {
            case 1: METRIC_SUMS(1); break;
            case 2: METRIC_SUMS(2); break;
            case 4: METRIC_SUMS(4); break;
            case 8: METRIC_SUMS(8); break;
            case 16: METRIC_SUMS(16); break;
            default: METRIC_SUMS(32); break;
        }
#undef METRIC_SUMS
        hipLaunchKernelGGL(metric_means_kernel, dim3((K * C + 3) / 4, B), dim3(256), 0, st, class_partials, bpi, K, C, means, counts);
    }
    const int bpi_f = feats ? metric_bpi_flat(B, HW, C) : 1, bpi_l = logits ? metric_bpi_quads(B, HW) : 1;
    const int bpi = bpi_f > bpi_l ? bpi_f : bpi_l;
    const bool vf = feats && metric_vec(HW * C, feats, nullptr), vl = logits && metric_vec(HW, logits, nullptr);
    const FastDiv divC = make_fastdiv((uint32_t)C);
#define METRIC_TERMS(VF, VL)                                                                                                   \
    hipLaunchKernelGGL((metric_terms_kernel<VF, VL>), dim3(bpi, B), dim3(256), 0, st, logits, feats, labels, means, term_partials, \
                       K, C, HW, divC, ignore_index)
    if (vf && vl) METRIC_TERMS(true, true);
    else if (vf) METRIC_TERMS(true, false);
    else if (vl) METRIC_TERMS(false, true);
    else METRIC_TERMS(false, false);
#undef METRIC_TERMS
    hipLaunchKernelGGL(metric_fold_kernel, dim3(1), dim3(256), 0, st, term_partials, B, bpi, 1.0 / (double)HW, sums);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_metric_finalize(const double* sums, int B, float beta, float gamma, float n_images, float* term, void* stream) {
    if (!sums || !term || B <= 0 || !isfinite(beta) || !isfinite(gamma)) return DML_EINVAL;
    hipLaunchKernelGGL(metric_finalize_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sums, B, beta, gamma,
                       n_images, term);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_metric_bwd(const float* feats, const int64_t* labels, const float* means, const double* sums, const float* gout,
                              float* glogits, float* gfeats, int B, int K, int C, int H, int W, int64_t ignore_index, float beta,
                              float gamma, float n_images, void* stream) {
    if (!labels || !sums || (!glogits && !gfeats) || (gfeats && (!feats || !means))) return DML_EINVAL;
    if (!isfinite(beta) || !isfinite(gamma)) return DML_EINVAL;
    if (const int rc = metric_shape_check(B, K, C, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (gfeats) {
        const int bpi = metric_bpi_flat(B, HW, C);
        const FastDiv divC = make_fastdiv((uint32_t)C);
        if (metric_vec(HW * C, feats, gfeats))
            hipLaunchKernelGGL((metric_gfeats_kernel<true>), dim3(bpi, B), dim3(256), 0, st, feats, labels, means, sums, gout, gfeats, B,
                               K, C, HW, divC, ignore_index, gamma, n_images);
        else
            hipLaunchKernelGGL((metric_gfeats_kernel<false>), dim3(bpi, B), dim3(256), 0, st, feats, labels, means, sums, gout, gfeats,
                               B, K, C, HW, divC, ignore_index, gamma, n_images);
    }
    if (glogits) {
        const int bpi = metric_bpi_quads(B, HW);
        if (metric_vec(HW, glogits, nullptr))
            hipLaunchKernelGGL((metric_glogits_kernel<true>), dim3(bpi, B), dim3(256), 0, st, labels, sums, gout, glogits, B, K, HW,
                               ignore_index, beta, n_images);
        else
            hipLaunchKernelGGL((metric_glogits_kernel<false>), dim3(bpi, B), dim3(256), 0, st, labels, sums, gout, glogits, B, K, HW,
                               ignore_index, beta, n_images);
    }
    DML_LAUNCH_CHECK();
    return 0;
}
