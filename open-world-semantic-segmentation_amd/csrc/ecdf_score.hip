// The per-class ECDF certainty score (the recipe DeepLabV3Plus-Pytorch/main_embedding.py:106-113,172-226,249-260 and
// test_embedding.py:155-163,361-364 of the reference keep commented): over a calibration set, per class, the empirical CDF of the
// distance sums s = -sum_k L_k of the pixels that are labelled and predicted that class; then per pixel
// conf = sum_cl softmax_cl * Certainty(E_cl(s)).  The reference copies every logit map to the host, keeps 1 pixel in 500 and fits
// statsmodels' ECDF; here an ECDF is a histogram over NB bins of [0, clip] whose value is bitwise defined (the header), so
//   dml_ecdf_collect  counts every calibration pixel in one read of the logits and the labels (uint32 LDS cells, int64 atomics),
//   dml_ecdf_table    turns the counts into the certainty itself, bin-major, so that
//   dml_ecdf_score    is one read of the logits and one 16-byte-vector row lookup per pixel.
#include "common.h"

#include <cmath>

namespace {

constexpr int ECDF_MAX_CLASSES = 32, ECDF_MAX_BINS = 2048, ECDF_MAX_CELLS = 32768;   // 32768 uint32 cells: 128 of the CU's 160 KiB
constexpr int ECDF_KREG = 16;                  // classes a lane keeps in registers, as MIX_KREG of scores.hip
// The largest histogram leaves room for one workgroup per CU, so the workgroup is the largest there is: 16 waves, four per SIMD,
// each lane with a 4-pixel group of up to 16 planes in flight (16 x 16 bytes).  Smaller histograms let several such workgroups share
// a CU, up to the 32-wave cap.  (dmlnet/_lib.py ECDF_THREADS / ECDF_MAX_BLOCKS)
constexpr int ECDF_THREADS = 1024;
constexpr int ECDF_MAX_BLOCKS = 512;           // workgroups of a launch, all images together: each zeroes and flushes Kn * NB cells
constexpr int SCORE_GRID = 2048;
constexpr int SCORE_KREG_WIDE = 20;            // the score kernel's second register form

// bin of a distance sum that is not NaN (the header's definition; inv_w = (float)NB / clip)
__host__ __device__ __forceinline__ int ecdf_bin(float s, float clip, float inv_w, int NB) {
    if (s >= clip) return NB - 1;
    if (s <= 0.f) return 0;
    const int b = (int)(s * inv_w);
    return b < NB - 1 ? b : NB - 1;
}

template <int PX> __device__ __forceinline__ void load_labels(const int64_t* p, int64_t (&l)[PX]) {
    if constexpr (PX == 4) {
        typedef long long ll2 __attribute__((ext_vector_type(2)));
        const ll2 a = reinterpret_cast<const ll2*>(p)[0], b = reinterpret_cast<const ll2*>(p)[1];
        l[0] = a.x; l[1] = a.y; l[2] = b.x; l[3] = b.y;
    } else {
        l[0] = *p;
    }
}

// ---- collect: hist[label - k_first][bin(s)] += 1 where label == pred
template <int PX, bool REG>
__global__ __launch_bounds__(ECDF_THREADS) void ecdf_collect_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ labels,
                                                                    unsigned long long* __restrict__ hist, int K, int k_first,
                                                                    int64_t HW, float clip, float inv_w, int NB) {
    extern __shared__ uint32_t ecdf_cells[];
    const int Kn = K - k_first, n_cells = Kn * NB;
    for (int i = threadIdx.x; i < n_cells; i += ECDF_THREADS) ecdf_cells[i] = 0u;
    __syncthreads();
    const int b = blockIdx.y;
    const float* img = logits + ((int64_t)b * K + k_first) * HW;
    const int64_t* lab = labels + (int64_t)b * HW;
    const int64_t groups = (HW + PX - 1) / PX;                       // PX = 4 runs only when HW % 4 == 0
    for (int64_t g = (int64_t)blockIdx.x * ECDF_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * ECDF_THREADS) {
        const int64_t pix = g * PX;
        const float* src = img + pix;
        int64_t l[PX];
        load_labels<PX>(lab + pix, l);
        float sum[PX], best[PX];
        int bi[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { sum[p] = 0.f; best[p] = 0.f; bi[p] = 0; }
        if constexpr (REG) {
            float v[ECDF_KREG][PX];
#pragma unroll
            for (int k = 0; k < ECDF_KREG; ++k)
                if (k < Kn) load_px<PX>(src + (int64_t)k * HW, v[k]);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
#pragma unroll
                for (int k = 0; k < ECDF_KREG; ++k)
                    if (k < Kn) {
                        sum[p] += v[k][p];
                        if (k == 0 || v[k][p] > best[p]) { best[p] = v[k][p]; bi[p] = k; }
                    }
            }
        } else {
            for (int k = 0; k < Kn; ++k) {
                float v[PX];
                load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    sum[p] += v[p];
                    if (k == 0 || v[p] > best[p]) { best[p] = v[p]; bi[p] = k; }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float s = -sum[p] + 0.0f;                          // a zero sum is +0.0, never -0.0
            if (s != s || l[p] < k_first || l[p] >= K) continue;     // a NaN sum has no bin; 255, -1 and the background drop out
            const int cl = (int)l[p] - k_first;
            if (cl == bi[p]) atomicAdd(&ecdf_cells[cl * NB + ecdf_bin(s, clip, inv_w, NB)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_cells; i += ECDF_THREADS)
        if (ecdf_cells[i]) atomicAdd(hist + i, (unsigned long long)ecdf_cells[i]);
}

// ---- table: one workgroup per column.  A thread owns TABLE_PER consecutive bins; the 256 partial sums are scanned by one thread.
constexpr int TABLE_THREADS = 256, TABLE_PER = ECDF_MAX_BINS / TABLE_THREADS;

__global__ __launch_bounds__(TABLE_THREADS) void ecdf_table_kernel(const int64_t* __restrict__ hist, float* __restrict__ table,
                                                                   const float* __restrict__ thresholds, int Kn, int Kp, int NB,
                                                                   float clip, float inv_w, int mode, float cut, float slope) {
    __shared__ unsigned long long part[TABLE_THREADS];
    __shared__ float ecdf[ECDF_MAX_BINS];
    const int cl = blockIdx.x, t = threadIdx.x;
    if (cl >= Kn) {                                                   // a padding column
        for (int i = t; i < NB; i += TABLE_THREADS) table[(int64_t)i * Kp + cl] = 0.f;
        return;
    }
    const int64_t* h = hist + (int64_t)cl * NB;
    const int per = (NB + TABLE_THREADS - 1) / TABLE_THREADS, lo = t * per;
    unsigned long long c[TABLE_PER], mine = 0;
#pragma unroll
    for (int i = 0; i < TABLE_PER; ++i) {
        c[i] = (i < per && lo + i < NB) ? (unsigned long long)h[lo + i] : 0ull;
        mine += c[i];
    }
    part[t] = mine;
    __syncthreads();
    if (t == 0) {                                                     // exclusive scan
        unsigned long long run = 0;
        for (int i = 0; i < TABLE_THREADS; ++i) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        part[0] = run;                                                // thread 0's own offset is 0: its place holds the total n_cl
    }
    __syncthreads();
    const unsigned long long n = part[0];
    unsigned long long cum = t == 0 ? 0ull : part[t];
#pragma unroll
    for (int i = 0; i < TABLE_PER; ++i)
        if (i < per && lo + i < NB) {
            cum += c[i];                                              // inclusive: bin lo + i counts itself
            ecdf[lo + i] = n ? (float)((double)cum / (double)n) : 1.f;
        }
    __syncthreads();
    float at_thr = 0.f;
    if (mode == 1) {
        const float thr = thresholds[cl];
        at_thr = thr != thr ? thr : ecdf[ecdf_bin(thr, clip, inv_w, NB)];
    }
    for (int i = t; i < NB; i += TABLE_THREADS) {
        const float E = ecdf[i];
        float r = E;
        if (n == 0) r = 1.f;                                          // no evidence: the class's softmax weight passes through
        else if (mode == 0) r = E > cut ? 1.f : E;
        else if (mode == 1) r = 1.f / (1.f + expf(-slope * (E - at_thr)));
        table[(int64_t)i * Kp + cl] = r;
    }
}

// ---- score: conf = sum_k softmax_k * table[bin(s)][k - k_first].  KR > 0 keeps up to KR classes of a lane's pixels in registers (16, or
// 20 for the 19 classes of Cityscapes: 4 waves per SIMD instead of 5, and a third fewer loads than reading the logits twice);
// KR = 0 reads the logits a second time, from cache.
template <int PX, int KR>
__global__ __launch_bounds__(256) void ecdf_score_kernel(const float* __restrict__ logits, const float* __restrict__ table,
                                                         float* __restrict__ conf, int K, int k_first, int Kp, int64_t HW, float clip,
                                                         float inv_w, int NB) {
    const int b = blockIdx.y, Kn = K - k_first;
    const float* img = logits + ((int64_t)b * K + k_first) * HW;
    const int64_t groups = (HW + PX - 1) / PX;                       // PX = 4 runs only when HW % 4 == 0
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t pix = g * PX;
        const float* src = img + pix;
        float out[PX];
        if constexpr (KR > 0) {
            float v[KR][PX];
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < Kn) load_px<PX>(src + (int64_t)k * HW, v[k]);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                float sum = 0.f, best = v[0][p];
#pragma unroll
                for (int k = 0; k < KR; ++k)
                    if (k < Kn) { sum += v[k][p]; best = fmaxf(best, v[k][p]); }
                const float s = -sum + 0.0f;
                if (s != s) { out[p] = s; continue; }
                const float* row = table + (int64_t)ecdf_bin(s, clip, inv_w, NB) * Kp;
                float den = 0.f, num = 0.f;
#pragma unroll
                for (int q = 0; q < KR / 4; ++q)
                    if (4 * q < Kn) {
                        const float4 t4 = load4(row + 4 * q);
                        const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (4 * q + j < Kn) {
                                const float e = expf(v[4 * q + j][p] - best);
                                den += e;
                                num = fmaf(e, t[j], num);
                            }
                    }
                out[p] = num / den;
            }
        } else {
            float sum[PX], best[PX], v[PX];
            load_px<PX>(src, v);
#pragma unroll
            for (int p = 0; p < PX; ++p) { sum[p] = 0.f; best[p] = v[p]; }
            for (int k = 0; k < Kn; ++k) {
                load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                for (int p = 0; p < PX; ++p) { sum[p] += v[p]; best[p] = fmaxf(best[p], v[p]); }
            }
            const float* row[PX];
            float den[PX], num[PX];
            bool nan[PX];
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const float s = -sum[p] + 0.0f;
                nan[p] = s != s;
                row[p] = table + (int64_t)(nan[p] ? 0 : ecdf_bin(s, clip, inv_w, NB)) * Kp;
                den[p] = 0.f; num[p] = 0.f;
            }
            for (int q = 0; 4 * q < Kn; ++q) {                        // the second read of the logits comes from cache
                float t[PX][4];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const float4 t4 = load4(row[p] + 4 * q);
                    t[p][0] = t4.x; t[p][1] = t4.y; t[p][2] = t4.z; t[p][3] = t4.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < Kn) {
                        load_px<PX>(src + (int64_t)(4 * q + j) * HW, v);
#pragma unroll
                        for (int p = 0; p < PX; ++p) {
                            const float e = expf(v[p] - best[p]);
                            den[p] += e;
                            num[p] = fmaf(e, t[p][j], num[p]);
                        }
                    }
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) out[p] = nan[p] ? NAN : num[p] / den[p];
        }
        store_px<PX>(conf + (int64_t)b * HW + pix, out);
    }
}

// argument checks the three entry points share
int ecdf_check_bins(int Kn, int NB, float clip) {
    if (Kn < 1 || NB < 1 || !(clip > 0.f) || !std::isfinite(clip)) return DML_EINVAL;
    if (Kn > ECDF_MAX_CLASSES || NB > ECDF_MAX_BINS) return DML_EUNSUPPORTED;
    return 0;
}
int ecdf_check_frame(int B, int K, int H, int W, int k_first) {
    if (B <= 0 || K <= 0 || H <= 0 || W <= 0 || k_first < 0 || k_first >= K) return DML_EINVAL;
    return 0;
}
// the image index is the grid's y; 2^40 pixels keep every element offset (x K, x 8 bytes) inside int64
bool ecdf_too_large(int B, int H, int W) { return B > 65535 || (int64_t)H * W > (1ll << 40) / B; }

}  // namespace

extern "C" int dml_ecdf_collect(const float* logits, const int64_t* labels, int64_t* hist, int B, int K, int H, int W, int k_first,
                                float clip, int NB, void* stream) {
    if (!logits || !labels || !hist) return DML_EINVAL;
    int rc = ecdf_check_frame(B, K, H, W, k_first);
    if (rc == 0) rc = ecdf_check_bins(K - k_first, NB, clip);
    if (rc != 0) return rc;
    const int Kn = K - k_first;
    if (Kn * NB > ECDF_MAX_CELLS || ecdf_too_large(B, H, W)) return DML_EUNSUPPORTED;
    if (!aligned_to(4, logits) || !aligned_to(8, labels, hist)) return DML_EALIGN;
    const int64_t HW = (int64_t)H * W;
    const bool vec = HW % 4 == 0 && aligned16(logits, labels);
    const int64_t passes = ((vec ? HW / 4 : HW) + ECDF_THREADS - 1) / ECDF_THREADS;
    const int cap = ECDF_MAX_BLOCKS / B > 1 ? ECDF_MAX_BLOCKS / B : 1;
    const int blocks = (int)(passes < cap ? passes : cap);
    // a workgroup's uint32 cells cannot overflow: it sees at most ceil(passes / blocks) * ECDF_THREADS * 4 pixels
    if ((passes + blocks - 1) / blocks >= (1ll << 32) / (ECDF_THREADS * 4)) return DML_EUNSUPPORTED;
    const float inv_w = (float)NB / clip;
    const size_t lds = sizeof(uint32_t) * Kn * NB;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* hi = reinterpret_cast<unsigned long long*>(hist);
    const dim3 grid(blocks, B);
    // above 64 KiB of dynamic LDS the kernel opts in; a refusal is returned as what it is, not as the launch's error after it
#define ECDF_COLLECT(PX, REG)                                                                                                    \
    do {                                                                                                                         \
        if (lds > 65536) {                                                                                                       \
            const hipError_t e__ = hipFuncSetAttribute(reinterpret_cast<const void*>(&ecdf_collect_kernel<PX, REG>),             \
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,                              \
                                                       (int)(sizeof(uint32_t) * ECDF_MAX_CELLS));                                \
            if (e__ != hipSuccess) return (int)e__;                                                                              \
        }                                                                                                                        \
        hipLaunchKernelGGL((ecdf_collect_kernel<PX, REG>), grid, dim3(ECDF_THREADS), lds, st, logits, labels, hi, K, k_first, HW, \
                           clip, inv_w, NB);                                                                                     \
    } while (0)
    const bool reg = Kn <= ECDF_KREG;
    if (vec && reg) ECDF_COLLECT(4, true);
    else if (vec) ECDF_COLLECT(4, false);
    else if (reg) ECDF_COLLECT(1, true);
    else ECDF_COLLECT(1, false);
#undef ECDF_COLLECT
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_ecdf_table(const int64_t* hist, float* table, const float* thresholds, int Kn, int Kp, int NB, float clip,
                              int mode, float cut, float slope, void* stream) {
    if (!hist || !table) return DML_EINVAL;
    if (Kn < 1 || NB < 1 || !(clip > 0.f) || !std::isfinite(clip) || Kp % 4 != 0 || Kp < Kn || mode < 0 || mode > 2 ||
        (mode == 1 && !thresholds))
        return DML_EINVAL;
    if (Kn > ECDF_MAX_CLASSES || NB > ECDF_MAX_BINS) return DML_EUNSUPPORTED;
    if (!aligned_to(8, hist) || !aligned_to(4, thresholds) || !aligned16(table)) return DML_EALIGN;
    hipLaunchKernelGGL(ecdf_table_kernel, dim3(Kp), dim3(TABLE_THREADS), 0, static_cast<hipStream_t>(stream), hist, table,
                       thresholds, Kn, Kp, NB, clip, (float)NB / clip, mode, cut, slope);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_ecdf_score(const float* logits, const float* table, float* conf, int B, int K, int H, int W, int k_first, int Kp,
                              float clip, int NB, void* stream) {
    if (!logits || !table || !conf) return DML_EINVAL;
    int rc = ecdf_check_frame(B, K, H, W, k_first);
    if (rc == 0 && (Kp % 4 != 0 || Kp < K - k_first)) rc = DML_EINVAL;
    if (rc == 0) rc = ecdf_check_bins(K - k_first, NB, clip);
    if (rc != 0) return rc;
    if (ecdf_too_large(B, H, W)) return DML_EUNSUPPORTED;
    if (!aligned_to(4, logits, conf) || !aligned16(table)) return DML_EALIGN;
    const int64_t HW = (int64_t)H * W;
    // with H W % 4 == 0 every plane and every image keep the base pointer's alignment
    const bool vec = HW % 4 == 0 && aligned16(logits, conf);
    const int Kn = K - k_first, kr = Kn <= ECDF_KREG ? ECDF_KREG : Kn <= SCORE_KREG_WIDE ? SCORE_KREG_WIDE : 0;
    const dim3 grid(grid_for(vec ? HW / 4 : HW, 256, SCORE_GRID), B);
    const float inv_w = (float)NB / clip;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define ECDF_SCORE(PX, KR) \
    hipLaunchKernelGGL((ecdf_score_kernel<PX, KR>), grid, dim3(256), 0, st, logits, table, conf, K, k_first, Kp, HW, clip, inv_w, NB)
    if (vec && kr == ECDF_KREG) ECDF_SCORE(4, ECDF_KREG);
    else if (vec && kr) ECDF_SCORE(4, SCORE_KREG_WIDE);
    else if (vec) ECDF_SCORE(4, 0);
    else if (kr == ECDF_KREG) ECDF_SCORE(1, ECDF_KREG);
    else if (kr) ECDF_SCORE(1, SCORE_KREG_WIDE);
    else ECDF_SCORE(1, 0);
#undef ECDF_SCORE
    DML_LAUNCH_CHECK();
    return 0;
}
