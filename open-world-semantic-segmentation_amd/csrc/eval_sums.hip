// Sums of the evaluation, for gfx950: the confusion matrix of the stream metrics and the masked class feature sums behind the
// few-shot prototypes.  Both accumulate per workgroup in LDS and flush with one atomic per bin.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// confusion matrix (metrics/stream_metrics.py:49-55 of the reference): per-workgroup LDS histogram, int64 flush
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ lt, const int64_t* __restrict__ lp,
                                                        unsigned long long* __restrict__ hist, int64_t count, int n) {
    extern __shared__ uint32_t bins[];
    const int nb = n * n;
    for (int i = threadIdx.x; i < nb; i += 256) bins[i] = 0u;
    __syncthreads();
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const int64_t pairs = count >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * 256) {
        const ll2 t = reinterpret_cast<const ll2*>(lt)[i], p = reinterpret_cast<const ll2*>(lp)[i];
        if (t.x >= 0 && t.x < n && p.x >= 0 && p.x < n) atomicAdd(&bins[(int)t.x * n + (int)p.x], 1u);
        if (t.y >= 0 && t.y < n && p.y >= 0 && p.y < n) atomicAdd(&bins[(int)t.y * n + (int)p.y], 1u);
    }
    if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t t = lt[count - 1], p = lp[count - 1];
        if (t >= 0 && t < n && p >= 0 && p < n) atomicAdd(&bins[(int)t * n + (int)p], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256)
        if (bins[i]) atomicAdd(hist + i, (unsigned long long)bins[i]);
}

// ------------------------------------------------------------------------------------------------
// masked feature sum for the few-shot prototypes (test_embedding.py:413-425 of the reference)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void class_feature_sum_kernel(const float* __restrict__ feats, const int64_t* __restrict__ labels,
                                                                int64_t n_px, int C, int64_t class_id, double* __restrict__ sums,
                                                                unsigned long long* __restrict__ count) {
    __shared__ double sh[MAXC];
    __shared__ unsigned long long shn;
    if (threadIdx.x < MAXC) sh[threadIdx.x] = 0.0;
    if (threadIdx.x == 0) shn = 0ull;
    __syncthreads();
    float acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
    unsigned long long n = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_px; p += (int64_t)gridDim.x * 256) {
        if (labels[p] != class_id) continue;
        ++n;
        const float* f = feats + p * C;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) acc[c] += f[c];
    }
    if (n) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) atomicAdd(&sh[c], (double)acc[c]);
        atomicAdd(&shn, n);
    }
    __syncthreads();
    if (threadIdx.x < C && sh[threadIdx.x] != 0.0) atomicAdd(sums + threadIdx.x, sh[threadIdx.x]);
    if (threadIdx.x == 0 && shn) atomicAdd(count, shn);
}

// ------------------------------------------------------------------------------------------------
// the same for up to MAXM classes in one read of the features and labels (the shots of the 16+2 / 16+3 settings).
// QUADS lanes share a pixel, each owns 4 channels (one 16-byte load when C % 4 == 0), so a thread carries MAXM x 4 fp32
// partial sums instead of MAXM x C.  Accumulation as above: fp32 within a thread, double across threads.
// ------------------------------------------------------------------------------------------------
constexpr int MAXM = 8;

template <int QUADS, bool VEC>
__global__ __launch_bounds__(256) void class_feature_sums_kernel(const float* __restrict__ feats, const int64_t* __restrict__ labels,
                                                                 int64_t n_px, int C, const int64_t* __restrict__ class_ids, int M,
                                                                 double* __restrict__ sums, unsigned long long* __restrict__ counts) {
    __shared__ double sh[MAXM * MAXC];
    __shared__ unsigned long long shn[MAXM];
    for (int i = threadIdx.x; i < MAXM * MAXC; i += 256) sh[i] = 0.0;
    if (threadIdx.x < MAXM) shn[threadIdx.x] = 0ull;
    __syncthreads();
    int64_t ids[MAXM];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) ids[m] = class_ids[m < M ? m : 0];
    float acc[MAXM][4];
    unsigned n[MAXM];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        n[m] = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m][e] = 0.f;
    }
    constexpr int SLOTS = 256 / QUADS;                               // pixels a workgroup reads per iteration
    const int q = threadIdx.x % QUADS, c0 = 4 * q;
    for (int64_t p = (int64_t)blockIdx.x * SLOTS + threadIdx.x / QUADS; p < n_px; p += (int64_t)gridDim.x * SLOTS) {
        const int64_t lab = labels[p];
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (VEC) {
            if (c0 < C) {
                const float4 t = *reinterpret_cast<const float4*>(feats + p * C + c0);
                f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < C) f[e] = feats[p * C + c0 + e];
        }
#pragma unroll
        for (int m = 0; m < MAXM; ++m)
            if (m < M && lab == ids[m]) {
                ++n[m];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][e] += f[e];
            }
    }
#pragma unroll
    for (int m = 0; m < MAXM; ++m)
        if (n[m]) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < C) atomicAdd(&sh[m * MAXC + c0 + e], (double)acc[m][e]);
            if (q == 0) atomicAdd(&shn[m], (unsigned long long)n[m]);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < M * MAXC; i += 256) {
        const int m = i / MAXC, c = i % MAXC;
        if (c < C && sh[i] != 0.0) atomicAdd(sums + m * C + c, sh[i]);
    }
    if (threadIdx.x < M && shn[threadIdx.x]) atomicAdd(counts + threadIdx.x, shn[threadIdx.x]);
}

}  // namespace

extern "C" int dml_confusion_update(const int64_t* label_true, const int64_t* label_pred, int64_t* hist, int64_t count,
                                    int n_classes, void* stream) {
    if (!label_true || !label_pred || !hist || count < 0 || n_classes <= 0 || n_classes > 64) return DML_EINVAL;
    if (!aligned16(label_true, label_pred)) return DML_EALIGN;
    if (count == 0) return 0;
    // a workgroup's uint32 bins cannot overflow: it sees at most count / grid + 512 elements
    int64_t blocks = (count / 2 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    if (count / blocks >= (1ll << 31)) return DML_EUNSUPPORTED;
    hipLaunchKernelGGL(confusion_kernel, dim3((int)blocks), dim3(256), sizeof(uint32_t) * n_classes * n_classes,
                       static_cast<hipStream_t>(stream), label_true, label_pred, reinterpret_cast<unsigned long long*>(hist),
                       count, n_classes);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_class_feature_sum(const float* feats, const int64_t* labels, int64_t n_px, int C, int64_t class_id,
                                     double* sums, unsigned long long* count, void* stream) {
    if (!feats || !labels || !sums || !count || n_px <= 0 || C <= 0 || C > MAXC) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(sums, 0, sizeof(double) * C, st) != hipSuccess || hipMemsetAsync(count, 0, 8, st) != hipSuccess)
        return DML_EINVAL;
    hipLaunchKernelGGL(class_feature_sum_kernel, dim3(grid_for(n_px, 256, 1024)), dim3(256), 0, st, feats, labels, n_px, C,
                       class_id, sums, count);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_class_feature_sums(const float* feats, const int64_t* labels, int64_t n_px, int C,
                                      const int64_t* class_ids, int M, double* sums, unsigned long long* counts,
                                      void* stream) {
    if (!feats || !labels || !class_ids || !sums || !counts || n_px <= 0 || C <= 0 || C > MAXC || M <= 0 || M > MAXM)
        return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(sums, 0, sizeof(double) * M * C, st) != hipSuccess || hipMemsetAsync(counts, 0, 8 * M, st) != hipSuccess)
        return DML_EINVAL;
    // 1024 x 256 pixel slots at most, as the single-class kernel: a thread's fp32 partial has ceil(n_px / 262144) terms
    const int quads = C <= 4 ? 1 : C <= 8 ? 2 : C <= 16 ? 4 : 8;
    const dim3 grid(grid_for(n_px * quads, 256, 1024 * quads));
    const bool vec = C % 4 == 0 && aligned16(feats);
#define DML_FSUMS(Q)                                                                                                         \
    do {                                                                                                                     \
        if (vec)                                                                                                             \
            hipLaunchKernelGGL((class_feature_sums_kernel<Q, true>), grid, dim3(256), 0, st, feats, labels, n_px, C,         \
                               class_ids, M, sums, counts);                                                                  \
        else                                                                                                                 \
            hipLaunchKernelGGL((class_feature_sums_kernel<Q, false>), grid, dim3(256), 0, st, feats, labels, n_px, C,        \
                               class_ids, M, sums, counts);                                                                  \
    } while (0)
    if (quads == 1) DML_FSUMS(1);
    else if (quads == 2) DML_FSUMS(2);
    else if (quads == 4) DML_FSUMS(4);
    else DML_FSUMS(8);
#undef DML_FSUMS
    DML_LAUNCH_CHECK();
    return 0;
}
