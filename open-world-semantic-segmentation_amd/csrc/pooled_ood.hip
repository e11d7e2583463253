// Dataset-level (pooled) AUROC / AUPR / FPR at a recall level: the measures of anomaly/anom_utils.py:25-78 of the reference taken over
// all pixels of a dataset at once instead of per frame (eval_ood_traditional.py:128-148,587-589 averages per-frame figures).
//
// A per-frame sort (ood_measures.hip) needs every key resident; a dataset is 10^9 keys.  What streams is a histogram: the confidence
// is cut into NB equal bins of [lo, hi] and every pixel adds one to hist[positive ? 0 : 1][bin].  dml_pooled_ood_update makes one read of
// the confidence, the label and the mask of a frame (12 or 13 bytes per pixel) and counts as open_sweep.hip does -- uint32 LDS cells per
// workgroup, flushed with 64-bit integer atomics: exact, order-free, bitwise reproducible, and two states over disjoint frames simply
// add.  dml_pooled_ood_finalize turns the 2 NB counts into the measures of the quantised scores -bin with one workgroup; its integer
// sums are carried in 128 bits, so they stay exact up to 2^40 pixels.
#include "common.h"

#include <cmath>

namespace {

constexpr int POOLED_MAX_BINS = 8192, POOLED_MAX_OUT = 8;
constexpr int POOLED_THREADS = 256, POOLED_PX = 8;               // a lane holds 8 pixels of a pass, 256 apart: 16 or 24 loads in flight
constexpr int POOLED_SPAN = POOLED_THREADS * POOLED_PX;          // pixels of one workgroup's pass (dmlnet/_lib.py POOLED_OOD_SPAN)
// one workgroup per CU: each zeroes and flushes up to 2 * 8192 cells, and the flush -- 64-byte atomic requests at the L2's rate -- is what
// a frame spread over many bins waits for.  Measured against 512 (open_sweep.hip's cap) and 128: DESIGN.md 7n
constexpr int POOLED_MAX_BLOCKS = 256;                           // (dmlnet/_lib.py POOLED_OOD_MAX_BLOCKS)
constexpr int POOLED_COUNTERS = 5;                               // n_nan, n_below, n_above, n_masked, n_frames behind hist[2][NB]
constexpr int FIN_THREADS = 256;

struct PooledArgs {
    int64_t out[POOLED_MAX_OUT];
    float lo, hi, inv_w;
    int n_out, NB;
};

// the bitwise definition of the header: one rounding per operation, nothing to contract
__device__ __forceinline__ int pooled_bin(float c, float lo, float hi, float inv_w, int NB) {
    if (c >= hi) return NB - 1;
    if (c <= lo) return 0;
    const int b = (int)__fmul_rn(__fsub_rn(c, lo), inv_w);
    return b < NB - 1 ? b : NB - 1;
}

template <bool MASK>
__global__ __launch_bounds__(POOLED_THREADS) void pooled_update_kernel(const float* __restrict__ conf, const int64_t* __restrict__ label,
                                                                       const uint8_t* __restrict__ mask, int64_t n, PooledArgs a,
                                                                       unsigned long long* __restrict__ state) {
    extern __shared__ uint32_t pooled_cells[];                   // [2][NB], then n_nan, n_below, n_above, n_masked
    const int NB = a.NB, n_cells = 2 * NB + 4;
    for (int i = threadIdx.x; i < n_cells; i += POOLED_THREADS) pooled_cells[i] = 0u;
    __syncthreads();
    uint32_t n_nan = 0, n_below = 0, n_above = 0, n_masked = 0;
    for (int64_t base = (int64_t)blockIdx.x * POOLED_SPAN; base < n; base += (int64_t)gridDim.x * POOLED_SPAN) {
        float c[POOLED_PX];
        int64_t l[POOLED_PX];
        uint8_t m[POOLED_PX];
#pragma unroll
        for (int k = 0; k < POOLED_PX; ++k) {
            const int64_t p = base + k * POOLED_THREADS + threadIdx.x;
            const bool in = p < n;
            c[k] = in ? conf[p] : 0.f;
            l[k] = in ? label[p] : 0;
            m[k] = (MASK && in) ? mask[p] : (uint8_t)1;
        }
#pragma unroll
        for (int k = 0; k < POOLED_PX; ++k) {
            const int64_t p = base + k * POOLED_THREADS + threadIdx.x;
            if (p >= n) continue;
            if (MASK && m[k] == 0) {
                ++n_masked;
                continue;
            }
            if (c[k] != c[k]) {
                ++n_nan;
                continue;
            }
            n_below += c[k] < a.lo ? 1u : 0u;
            n_above += c[k] > a.hi ? 1u : 0u;
            int row = 1;
#pragma unroll
            for (int o = 0; o < POOLED_MAX_OUT; ++o)
                if (o < a.n_out && l[k] == a.out[o]) row = 0;
            atomicAdd(&pooled_cells[row * NB + pooled_bin(c[k], a.lo, a.hi, a.inv_w, NB)], 1u);
        }
    }
    if (n_nan) atomicAdd(&pooled_cells[2 * NB + 0], n_nan);
    if (n_below) atomicAdd(&pooled_cells[2 * NB + 1], n_below);
    if (n_above) atomicAdd(&pooled_cells[2 * NB + 2], n_above);
    if (n_masked) atomicAdd(&pooled_cells[2 * NB + 3], n_masked);
    __syncthreads();
    for (int i = threadIdx.x; i < n_cells; i += POOLED_THREADS)
        if (pooled_cells[i]) atomicAdd(state + i, (unsigned long long)pooled_cells[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(state + 2 * NB + POOLED_COUNTERS - 1, 1ull);       // n_frames
}

// ---------------------------------------------------------------------------------------------------------------------------
// finalize
// ---------------------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 u128;

// a 128-bit integer to the nearest double in one rounding: the top 64 bits with a sticky bit for what was shifted out (64 bits hold
// more than the 53 + 2 a correct rounding needs), then an exact scaling
__device__ double u128_to_double(u128 x) {
    const uint64_t hi = (uint64_t)(x >> 64), lo = (uint64_t)x;
    if (hi == 0) return (double)lo;
    const int s = 64 - __clzll((long long)hi);                   // 1 .. 64 bits above the low limb
    const uint64_t top = (uint64_t)(x >> s);
    const bool sticky = (x & ((((u128)1) << s) - 1)) != 0;
    return ldexp((double)(top | (sticky ? 1ull : 0ull)), s);
}

struct FinCand {
    double d, r;                                                 // |recall - level| and the recall: smaller d, then larger r
    unsigned long long fp;
    int cut;
};

__device__ __forceinline__ void fin_take(FinCand& best, double level, unsigned long long tp, unsigned long long P,
                                         unsigned long long fp, int cut) {
    const double r = (double)tp / (double)P, d = fabs(r - level);
    if (best.cut < 0 || d < best.d || (d == best.d && r > best.r)) {
        best.d = d;
        best.r = r;
        best.fp = fp;
        best.cut = cut;
    }
}

__global__ __launch_bounds__(FIN_THREADS) void pooled_finalize_kernel(const unsigned long long* __restrict__ state, int NB,
                                                                      double level, double* __restrict__ result) {
    __shared__ unsigned long long sP[FIN_THREADS], sN[FIN_THREADS];
    __shared__ int sLast[FIN_THREADS];
    __shared__ unsigned long long sAl[FIN_THREADS], sAh[FIN_THREADS], sTl[FIN_THREADS], sTh[FIN_THREADS];
    __shared__ FinCand sC[FIN_THREADS];
    __shared__ double sPr[FIN_THREADS];                          // AUPR: a lane's bins summed ascending, then the lanes ascending
    __shared__ unsigned long long totP, totN;
    const int t = threadIdx.x, per = (NB + FIN_THREADS - 1) / FIN_THREADS;
    const int b0 = t * per < NB ? t * per : NB, b1 = b0 + per < NB ? b0 + per : NB;
    const unsigned long long* hp = state;
    const unsigned long long* hn = state + NB;
    // the chunk's totals and its last bin with a positive
    unsigned long long cp = 0, cn = 0;
    int last = -1;
    for (int b = b0; b < b1; ++b) {
        cp += hp[b];
        cn += hn[b];
        if (hp[b]) last = b;
    }
    sP[t] = cp;
    sN[t] = cn;
    sLast[t] = last;
    __syncthreads();
    if (t == 0) {                                                // exclusive scan of 256 chunks: sums, and the running last positive bin
        unsigned long long ap = 0, an = 0;
        int al = -1;
        for (int i = 0; i < FIN_THREADS; ++i) {
            const unsigned long long p = sP[i], q = sN[i];
            const int l = sLast[i];
            sP[i] = ap;
            sN[i] = an;
            sLast[i] = al;
            ap += p;
            an += q;
            if (l >= 0) al = l;
        }
        totP = ap;
        totN = an;
    }
    __syncthreads();
    const unsigned long long P = totP, N = totN;
    if (P == 0 || N == 0) {
        if (t == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            result[0] = result[1] = result[2] = nan;
            result[3] = (double)P;
            result[4] = (double)N;
            result[5] = nan;
            result[6] = -1.0;
            result[7] = 0.0;
        }
        return;
    }
    unsigned long long tp = sP[t], fp = sN[t];                   // exclusive prefixes at b0
    int prev = sLast[t];                                         // the last bin below b0 that holds a positive
    u128 au = 0, tie = 0;
    double pr = 0.0;
    FinCand best;
    best.d = 0.0;
    best.r = 0.0;
    best.fp = 0;
    best.cut = -1;
    for (int b = b0; b < b1; ++b) {
        const unsigned long long pb = hp[b], nb = hn[b];
        if (pb) {
            // the candidate of the previous positive bin: flagged are the bins up to it, the negatives counted reach to b - 1
            if (prev >= 0) fin_take(best, level, tp, P, fp, prev);
            prev = b;
        }
        tp += pb;
        fp += nb;
        au += (u128)pb * (u128)(2ull * (N - fp) + nb);
        tie += (u128)pb * (u128)nb;
        if (pb) pr += ((double)pb / (double)P) * ((double)tp / (double)(tp + fp));
        if (pb && tp == P) fin_take(best, level, P, P, fp, b);   // the highest positive bin: full recall, its own fp
    }
    sAl[t] = (unsigned long long)au;
    sAh[t] = (unsigned long long)(au >> 64);
    sTl[t] = (unsigned long long)tie;
    sTh[t] = (unsigned long long)(tie >> 64);
    sC[t] = best;
    sPr[t] = pr;
    __syncthreads();
    if (t == 0) {
        u128 a = 0, ti = 0;
        FinCand bc = sC[0];
        for (int i = 0; i < FIN_THREADS; ++i) {
            a += ((u128)sAh[i] << 64) | (u128)sAl[i];
            ti += ((u128)sTh[i] << 64) | (u128)sTl[i];
            const FinCand c = sC[i];
            if (c.cut >= 0 && (bc.cut < 0 || c.d < bc.d || (c.d == bc.d && c.r > bc.r))) bc = c;
        }
        double aupr = 0.0;
        for (int i = 0; i < FIN_THREADS; ++i) aupr += sPr[i];
        const double dP = (double)P, dN = (double)N;
        result[0] = u128_to_double(a) / ((2.0 * dP) * dN);
        result[1] = aupr;
        result[2] = (double)bc.fp / dN;
        result[3] = dP;
        result[4] = dN;
        result[5] = u128_to_double(ti) / (dP * dN);
        result[6] = (double)bc.cut;
        result[7] = 0.0;
    }
}

}  // namespace

extern "C" int dml_pooled_ood_update(const float* conf, const int64_t* seg_label, const uint8_t* mask, int64_t n,
                                     const int64_t* out_labels, int n_out, float lo, float hi, int NB, int64_t* state, void* stream) {
    if (!conf || !seg_label || !out_labels || !state || n < 0) return DML_EINVAL;
    if (NB < 1 || NB > POOLED_MAX_BINS || n_out < 1 || n_out > POOLED_MAX_OUT) return DML_EINVAL;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return DML_EINVAL;
    const float width = hi - lo;                                 // float32, one rounding
    if (!std::isfinite(width)) return DML_EINVAL;                // a range wider than FLT_MAX has no bin width
    if ((reinterpret_cast<uintptr_t>(conf) & 3) || ((reinterpret_cast<uintptr_t>(seg_label) | reinterpret_cast<uintptr_t>(state)) & 7))
        return DML_EALIGN;
    if (n == 0) return 0;
    PooledArgs a;
    for (int o = 0; o < POOLED_MAX_OUT; ++o) a.out[o] = o < n_out ? out_labels[o] : 0;
    a.lo = lo;
    a.hi = hi;
    a.inv_w = (float)NB / width;
    a.n_out = n_out;
    a.NB = NB;
    const int64_t passes = (n + POOLED_SPAN - 1) / POOLED_SPAN;
    const int blocks = (int)(passes < POOLED_MAX_BLOCKS ? passes : POOLED_MAX_BLOCKS);
    // a workgroup's uint32 cells cannot overflow: it sees at most ceil(passes / blocks) * POOLED_SPAN pixels
    if ((passes + blocks - 1) / blocks >= (1ll << 32) / POOLED_SPAN) return DML_EUNSUPPORTED;
    const size_t lds = sizeof(uint32_t) * (2 * (size_t)NB + 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* s = reinterpret_cast<unsigned long long*>(state);
#define POOLED_UPDATE(M)                                                                                                         \
    do {                                                                                                                         \
        if (lds > 65536) {                                                                                                       \
            const hipError_t e__ = hipFuncSetAttribute(reinterpret_cast<const void*>(&pooled_update_kernel<M>),                  \
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,                              \
                                                       (int)(sizeof(uint32_t) * (2 * POOLED_MAX_BINS + 4)));                     \
            if (e__ != hipSuccess) return (int)e__;                                                                              \
        }                                                                                                                        \
        hipLaunchKernelGGL((pooled_update_kernel<M>), dim3(blocks), dim3(POOLED_THREADS), lds, st, conf, seg_label, mask, n, a, \
                           s);                                                                                                   \
    } while (0)
    if (mask)
        POOLED_UPDATE(true);
    else
        POOLED_UPDATE(false);
#undef POOLED_UPDATE
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_pooled_ood_finalize(const int64_t* state, int NB, double recall_level, double* result, void* stream) {
    if (!state || !result || NB < 1 || NB > POOLED_MAX_BINS || std::isnan(recall_level)) return DML_EINVAL;
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(result)) & 7) return DML_EALIGN;
    hipLaunchKernelGGL(pooled_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(state), NB, recall_level, result);
    DML_LAUNCH_CHECK();
    return 0;
}
