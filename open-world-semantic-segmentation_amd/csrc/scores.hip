// Open-world scores on the distance head's logits[B,K,H,W] (NCHW) and features[B,H,W,C], for gfx950: argmax and maximum softmax
// probability, the clipped distance sum, its mix with the MSP ("EDS + MMSP"), the relabel against few-shot prototypes, and all of
// them in one pass (open_world_post).  HBM-bound: a lane owns 4 consecutive pixels and reads every plane with a 16-byte load.
//
// Replaces the host numpy post-processing of test_embedding.py:339-350,428-445 and anomaly/eval_ood_traditional.py:301-305.
#include "common.h"

namespace {

// ---- argmax / max-softmax-probability
__global__ __launch_bounds__(256) void argmax_msp_kernel(const float* __restrict__ logits,
                                                         int64_t* __restrict__ preds, float* __restrict__ msp,
                                                         int B, int K, int64_t HW) {
    const int64_t total = (int64_t)B * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, pix = i - b * HW;
        const float* src = logits + b * K * HW + pix;
        float best = src[0];
        int bi = 0;
        for (int k = 1; k < K; ++k) {
            const float v = src[(int64_t)k * HW];
            if (v > best) { best = v; bi = k; }
        }
        if (preds) preds[i] = bi;
        if (msp) {
            float den = 0.f;
            for (int k = 0; k < K; ++k) den += expf(src[(int64_t)k * HW] - best);
            msp[i] = 1.f - 1.f / den;
        }
    }
}

// ---- dissum score: clip(-sum_k logit_k), then per-image min-max normalisation
// The integer atomic is chosen by the SIGN BIT, not by `v >= 0.f`: -0.0f compares >= 0 but its bit pattern is INT_MIN, which
// as a signed int never raises a stored maximum and replaces every stored negative minimum.
__device__ __forceinline__ void atomic_min_f(float* addr, float v) {
    if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f(float* addr, float v) {
    if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__global__ void minmax_init_kernel(float* work, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { work[2 * i] = INFINITY; work[2 * i + 1] = -INFINITY; }
}
__global__ __launch_bounds__(256) void dissum_kernel(const float* __restrict__ logits, float* __restrict__ score,
                                                     float* work, int K, int64_t HW, float clip, int inclusive) {
    __shared__ float smin[4], smax[4];
    const int b = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < HW;
         pix += (int64_t)gridDim.x * blockDim.x) {
        const float* src = logits + (int64_t)b * K * HW + pix;
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += src[(int64_t)k * HW];
        s = -s + 0.0f;                                          // a zero sum scores +0.0, never -0.0
        if (inclusive ? (s >= clip) : (s > clip)) s = clip;
        score[(int64_t)b * HW + pix] = s;
        lo = fminf(lo, s);
        hi = fmaxf(hi, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) { lo = fminf(lo, smin[i]); hi = fmaxf(hi, smax[i]); }
        lo = fminf(smin[0], lo); hi = fmaxf(smax[0], hi);
        if (lo <= hi) { atomic_min_f(work + 2 * b, lo); atomic_max_f(work + 2 * b + 1, hi); }
    }
}
__global__ __launch_bounds__(256) void minmax_norm_kernel(float* __restrict__ score, const float* work,
                                                          int64_t HW) {
    const int b = blockIdx.y;
    const float lo = work[2 * b], hi = work[2 * b + 1];
    const float den = hi - lo;
    for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < HW;
         pix += (int64_t)gridDim.x * blockDim.x) {
        float* p = score + (int64_t)b * HW + pix;
        *p = (*p - lo) / den;
    }
}

// ---- EDS + MMSP: the clipped distance sum and the maximum softmax probability (or the maximum logit), each min-max normalised
// per image, mixed through a sigmoid gate on the first (anomaly/eval_ood_traditional.py:302-305,434-435,447-448 of the
// reference; test_embedding.py:366-369 with prob_logit).  Pass 1 writes the raw maps s and m and leaves their ranges in
// work[4 b .. 4 b + 3]; pass 2 normalises and mixes.  The signed-zero rule of atomic_min_f / atomic_max_f serves both ranges:
// s is never -0.0 (the + 0.0f below), m can be (a maximum logit of -0.0).  PX = 4: a lane owns 4 consecutive pixels and reads
// every plane with one 16-byte load.  REG keeps up to MIX_KREG planes in registers; beyond that the softmax denominator reads
// the logits a second time, from cache (as argmax_msp_kernel does).  Both forms do the same operations in the same order.
constexpr int MIX_KREG = 16;
// workgroups of pass 1 per image: with every workgroup of a 720 x 1280 frame resident at once their atomics on the same four
// words arrive together and cost more than the loads; fewer workgroups that loop, and mix_range_update, cut the call from
// 0.058 to 0.032 ms there.  The form that re-reads wants more waves in flight.
constexpr int MIX_GRID_REG = 512, MIX_GRID_REREAD = 2048;

// One atomic pair at most: a stored minimum only falls and a stored maximum only rises while pass 1 runs, so a value read
// beforehand -- however stale -- that already is at or beyond ours means the atomic could change nothing, and it is skipped.
// Two zeros are ordered by their sign (see atomic_min_f), which a float comparison cannot see: they go to the atomic.
__device__ __forceinline__ void mix_range_update(float* lohi, float lo, float hi) {
    const volatile float* cur = lohi;
    const float clo = cur[0], chi = cur[1];
    if (!(clo <= lo) || (lo == 0.f && clo == 0.f)) atomic_min_f(lohi, lo);
    if (!(chi >= hi) || (hi == 0.f && chi == 0.f)) atomic_max_f(lohi + 1, hi);
}

template <int PX, bool REG>
__global__ __launch_bounds__(256) void dissum_msp_maps_kernel(const float* __restrict__ logits, float* __restrict__ smap,
                                                              float* __restrict__ mmap, float* work, int K, int k_first,
                                                              int64_t HW, float clip, int prob_logit) {
    __shared__ float sred[4][4];
    const int b = blockIdx.y, Kn = K - k_first;
    const float* img = logits + ((int64_t)b * K + k_first) * HW;
    float slo = INFINITY, shi = -INFINITY, mlo = INFINITY, mhi = -INFINITY;
    for (int64_t pix = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX; pix < HW;
         pix += (int64_t)gridDim.x * blockDim.x * PX) {
        const float* src = img + pix;
        float sum[PX], best[PX], den[PX], s[PX], m[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { sum[p] = 0.f; den[p] = 0.f; }
        if constexpr (REG) {
            float v[MIX_KREG][PX];
#pragma unroll
            for (int k = 0; k < MIX_KREG; ++k)
                if (k < Kn) load_px<PX>(src + (int64_t)k * HW, v[k]);
#pragma unroll
            for (int p = 0; p < PX; ++p) best[p] = v[0][p];
#pragma unroll
            for (int k = 0; k < MIX_KREG; ++k)
                if (k < Kn) {
#pragma unroll
                    for (int p = 0; p < PX; ++p) { sum[p] += v[k][p]; best[p] = fmaxf(best[p], v[k][p]); }
                }
            if (!prob_logit) {
#pragma unroll
                for (int k = 0; k < MIX_KREG; ++k)
                    if (k < Kn) {
#pragma unroll
                        for (int p = 0; p < PX; ++p) den[p] += expf(v[k][p] - best[p]);
                    }
            }
        } else {
            float v[PX];
            load_px<PX>(src, v);
#pragma unroll
            for (int p = 0; p < PX; ++p) best[p] = v[p];
            for (int k = 0; k < Kn; ++k) {
                load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                for (int p = 0; p < PX; ++p) { sum[p] += v[p]; best[p] = fmaxf(best[p], v[p]); }
            }
            if (!prob_logit) {
                for (int k = 0; k < Kn; ++k) {
                    load_px<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                    for (int p = 0; p < PX; ++p) den[p] += expf(v[p] - best[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            s[p] = -sum[p] + 0.0f;                                  // a zero sum scores +0.0, never -0.0
            if (s[p] >= clip) s[p] = clip;
            m[p] = prob_logit ? best[p] : 1.f / den[p];
            slo = fminf(slo, s[p]); shi = fmaxf(shi, s[p]);
            mlo = fminf(mlo, m[p]); mhi = fmaxf(mhi, m[p]);
        }
        store_px<PX>(smap + (int64_t)b * HW + pix, s);
        store_px<PX>(mmap + (int64_t)b * HW + pix, m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        slo = fminf(slo, __shfl_xor(slo, o, 64)); shi = fmaxf(shi, __shfl_xor(shi, o, 64));
        mlo = fminf(mlo, __shfl_xor(mlo, o, 64)); mhi = fmaxf(mhi, __shfl_xor(mhi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        float* r = sred[threadIdx.x >> 6];
        r[0] = slo; r[1] = shi; r[2] = mlo; r[3] = mhi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            slo = fminf(slo, sred[w][0]); shi = fmaxf(shi, sred[w][1]);
            mlo = fminf(mlo, sred[w][2]); mhi = fmaxf(mhi, sred[w][3]);
        }
        if (slo <= shi) mix_range_update(work + 4 * b, slo, shi);
        if (mlo <= mhi) mix_range_update(work + 4 * b + 2, mlo, mhi);
    }
}

// the gate is the plain division: an exp that overflows gives c = +0, 1 - c = 1 and conf = q
template <int PX>
__global__ __launch_bounds__(256) void dissum_msp_mix_kernel(const float* __restrict__ smap, const float* __restrict__ mmap,
                                                             const float* __restrict__ work, float* __restrict__ conf,
                                                             int64_t HW, float threshold, float slope) {
    const int b = blockIdx.y;
    const float slo = work[4 * b], sden = work[4 * b + 1] - slo;
    const float mlo = work[4 * b + 2], mden = work[4 * b + 3] - mlo;
    for (int64_t pix = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX; pix < HW;
         pix += (int64_t)gridDim.x * blockDim.x * PX) {
        const int64_t i = (int64_t)b * HW + pix;
        float s[PX], m[PX], out[PX];
        load_px<PX>(smap + i, s);
        load_px<PX>(mmap + i, m);
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float d = (s[p] - slo) / sden;
            const float q = (m[p] - mlo) / mden;
            const float c = 1.f / (1.f + expf(slope * (d - threshold)));
            out[p] = c * d + (1.f - c) * q;
        }
        store_px<PX>(conf + i, out);
    }
}

__global__ __launch_bounds__(256) void novel_relabel_kernel(const float* __restrict__ feats,
                                                            const float* __restrict__ logits,
                                                            const float* __restrict__ proto,
                                                            int64_t* __restrict__ preds, int B, int C, int K,
                                                            int64_t HW, float thresh, int64_t new_label) {
    const int64_t total = (int64_t)B * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, pix = i - b * HW;
        float d = 0.f;
        for (int c = 0; c < C; ++c) {
            const float t = feats[i * C + c] - proto[c];
            d += t * t;
        }
        d = -d;
        const float* src = logits + b * K * HW + pix;
        float best = src[0];
        for (int k = 1; k < K; ++k) best = fmaxf(best, src[(int64_t)k * HW]);
        if (d > thresh && d > best) preds[i] = new_label;
    }
}

// ---- open-world post-processing in one pass: argmax, MSP, raw dissum (+ per-image range) and the relabel against up to
// MAXN few-shot prototypes (test_embedding.py:339-350,365,445 and the 2- / 3-class rules at :510-511,:520-522 of the
// reference).  One read of the logits, one of the features.  PX = 4: a lane owns 4 consecutive pixels, every logit plane is
// read with one 16-byte load; PX = 1 serves H W % 4 != 0 and unaligned tensors.  FAST fixes C = K = 16: logits and the
// four 64-byte feature rows stay in registers.  The generic path keeps nothing: it re-reads the logits for the softmax
// denominator (as argmax_msp_kernel does) and the feature row per prototype; those hit in cache.
// POST = false is novel_relabel_multi: given preds, only the relabelled pixels are written.
constexpr int MAXN = 8;

// the strict winner among the prototype distances: `tie` when another one equals the best
__device__ __forceinline__ void top_update(float d, int j, float& best, int& bj, bool& tie) {
    if (j == 0 || d > best) { best = d; bj = j; tie = false; }
    else if (d == best) tie = true;
}

template <int PX, bool FAST, bool POST, bool NT>
__global__ __launch_bounds__(256) void open_world_post_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ feats,
                                                              const float* __restrict__ protos,
                                                              const int64_t* __restrict__ new_labels,
                                                              int64_t* __restrict__ preds, float* __restrict__ msp,
                                                              float* __restrict__ score, float* work, int Cr, int Kr,
                                                              int64_t HW, int N, float thresh, int vs_known, float clip,
                                                              int inclusive) {
    __shared__ __attribute__((aligned(16))) float sp[MAXN * MAXC];
    __shared__ int64_t slab[MAXN];
    __shared__ float smin[4], smax[4];
    const int C = FAST ? 16 : Cr, K = FAST ? 16 : Kr;
    if (threadIdx.x < N) slab[threadIdx.x] = new_labels[threadIdx.x];
    load_protos(sp, protos, N * C);                                  // ends with the block barrier (N = 0: nothing read)
    const int b = blockIdx.y;
    const float* lg = logits + (int64_t)b * K * HW;
    const bool need_logits = POST || vs_known;
    float lo = INFINITY, hi = -INFINITY;
    const int64_t groups = (HW + PX - 1) / PX;                       // PX = 4 runs only when HW % 4 == 0
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t pix = g * PX, i = (int64_t)b * HW + pix;
        float best[PX], sum[PX], den[PX];
        int bi[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { best[p] = -INFINITY; sum[p] = 0.f; den[p] = 0.f; bi[p] = 0; }
        if (need_logits) {
            if constexpr (FAST) {
                float l[16][PX];
#pragma unroll
                for (int k = 0; k < 16; ++k) load_px<PX, NT>(lg + (int64_t)k * HW + pix, l[k]);
#pragma unroll
                for (int k = 0; k < 16; ++k)
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        sum[p] += l[k][p];
                        if (k == 0 || l[k][p] > best[p]) { best[p] = l[k][p]; bi[p] = k; }
                    }
                if (POST && msp != nullptr)
#pragma unroll
                    for (int k = 0; k < 16; ++k)
#pragma unroll
                        for (int p = 0; p < PX; ++p) den[p] += expf(l[k][p] - best[p]);
            } else {
                for (int k = 0; k < K; ++k) {
                    float v[PX];
                    load_px<PX, false>(lg + (int64_t)k * HW + pix, v);
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        sum[p] += v[p];
                        if (k == 0 || v[p] > best[p]) { best[p] = v[p]; bi[p] = k; }
                    }
                }
                if (POST && msp != nullptr)
                    for (int k = 0; k < K; ++k) {
                        float v[PX];
                        load_px<PX, false>(lg + (int64_t)k * HW + pix, v);
#pragma unroll
                        for (int p = 0; p < PX; ++p) den[p] += expf(v[p] - best[p]);
                    }
            }
        }
        // relabel: the prototype that is strictly nearer than every other one, above the threshold (and the known classes)
        float top[PX];
        int tj[PX];
        bool tie[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { top[p] = -INFINITY; tj[p] = 0; tie[p] = false; }
        if (N > 0) {
            if constexpr (FAST) {
                float f[PX][16];
#pragma unroll
                for (int p = 0; p < PX; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 t = load4<NT>(feats + (i + p) * 16 + q * 4);
                        f[p][4 * q] = t.x; f[p][4 * q + 1] = t.y; f[p][4 * q + 2] = t.z; f[p][4 * q + 3] = t.w;
                    }
                // the prototype loop sits INSIDE the unrolled pixel loop, here and below: with the loops the other way
                // round hipcc keeps the winner's index in a scalar register (one value per wave, set from the uniform
                // loop counter only at j == 0) although the comparison that selects it is per lane, and every relabelled
                // pixel gets new_labels[0]
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    float tp = -INFINITY;
                    int jp = 0;
                    bool tp_tie = false;
                    for (int j = 0; j < N; ++j) {
                        float d = 0.f;
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            const float t = f[p][c] - sp[j * 16 + c];     // same address in every lane: an LDS broadcast
                            d += t * t;
                        }
                        top_update(-d, j, tp, jp, tp_tie);
                    }
                    top[p] = tp; tj[p] = jp; tie[p] = tp_tie;
                }
            } else {
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const float* fr = feats + (i + p) * C;
                    float tp = -INFINITY;
                    int jp = 0;
                    bool tp_tie = false;
                    for (int j = 0; j < N; ++j) {
                        float d = 0.f;
                        for (int c = 0; c < C; ++c) {
                            const float t = fr[c] - sp[j * C + c];
                            d += t * t;
                        }
                        top_update(-d, j, tp, jp, tp_tie);
                    }
                    top[p] = tp; tj[p] = jp; tie[p] = tp_tie;
                }
            }
        }
        int64_t out[PX];
        bool hit[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            hit[p] = N > 0 && !tie[p] && top[p] > thresh && (!vs_known || top[p] > best[p]);
            out[p] = hit[p] ? slab[tj[p]] : (int64_t)bi[p];
        }
        if constexpr (POST) {
            if constexpr (PX == 4) {
                typedef long long ll2 __attribute__((ext_vector_type(2)));
                ll2* dst = reinterpret_cast<ll2*>(preds + i);
                dst[0] = ll2{out[0], out[1]};
                dst[1] = ll2{out[2], out[3]};
                if (msp != nullptr)
                    store4(msp + i, make_float4(1.f - 1.f / den[0], 1.f - 1.f / den[1], 1.f - 1.f / den[2], 1.f - 1.f / den[3]));
            } else {
                preds[i] = out[0];
                if (msp != nullptr) msp[i] = 1.f - 1.f / den[0];
            }
            if (score != nullptr) {
                float s[PX];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    s[p] = -sum[p] + 0.0f;                            // a zero sum scores +0.0, never -0.0
                    if (inclusive ? (s[p] >= clip) : (s[p] > clip)) s[p] = clip;
                    lo = fminf(lo, s[p]);
                    hi = fmaxf(hi, s[p]);
                }
                store_px<PX>(score + i, s);
            }
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p)
                if (hit[p]) preds[i + p] = out[p];
        }
    }
    if (POST && score != nullptr) {                                   // per-image range, as dissum_kernel leaves it
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) { lo = fminf(lo, smin[w]); hi = fmaxf(hi, smax[w]); }
            if (lo <= hi) { atomic_min_f(work + 2 * b, lo); atomic_max_f(work + 2 * b + 1, hi); }
        }
    }
}

// argument checks shared by dml_open_world_post and dml_novel_relabel_multi
int open_world_check(const float* logits, const float* feats, const float* protos, const int64_t* new_labels,
                     const int64_t* preds, int B, int C, int K, int H, int W, int N) {
    if (!logits || !preds || B <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || N < 0) return DML_EINVAL;
    if (N > 0 && (!feats || !protos || !new_labels)) return DML_EINVAL;
    if (C > MAXC || K > MAXK || N > MAXN) return DML_EUNSUPPORTED;
    // the image index is the grid's y; 2^40 pixels keep every element offset (x K, x C, x 8 bytes) inside int64
    if (B > 65535 || (int64_t)B * H * W > (1ll << 40)) return DML_EUNSUPPORTED;
    return 0;
}

template <bool POST>
void open_world_launch(const float* logits, const float* feats, const float* protos, const int64_t* new_labels,
                       int64_t* preds, float* msp, float* score, float* work, int B, int C, int K, int64_t HW, int N,
                       float thresh, int vs_known, float clip, int inclusive, hipStream_t st) {
    // the generic 4-pixel path reads the feature rows with scalar loads: only the register path needs them aligned
    const bool vec = HW % 4 == 0 && aligned16(logits, preds, msp, score);
    const dim3 grid(grid_for(vec ? HW / 4 : HW, 256, 4096), B);
    if (vec && C == 16 && K == 16 && (N == 0 || aligned16(feats)))
        hipLaunchKernelGGL((open_world_post_kernel<4, true, POST, DIST_NT_DEFAULT>), grid, dim3(256), 0, st, logits, feats,
                           protos, new_labels, preds, msp, score, work, C, K, HW, N, thresh, vs_known, clip, inclusive);
    else if (vec)
        hipLaunchKernelGGL((open_world_post_kernel<4, false, POST, false>), grid, dim3(256), 0, st, logits, feats, protos,
                           new_labels, preds, msp, score, work, C, K, HW, N, thresh, vs_known, clip, inclusive);
    else
        hipLaunchKernelGGL((open_world_post_kernel<1, false, POST, false>), grid, dim3(256), 0, st, logits, feats, protos,
                           new_labels, preds, msp, score, work, C, K, HW, N, thresh, vs_known, clip, inclusive);
}

}  // namespace

extern "C" int dml_argmax_msp(const float* logits, int64_t* preds, float* msp, int B, int K, int H, int W,
                              void* stream) {
    if (!logits || B <= 0 || K <= 0) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(argmax_msp_kernel, dim3(grid_for(B * HW, 256, 256 * 16)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), logits, preds, msp, B, K, HW);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_dissum_score(const float* logits, float* score, float* work, int B, int K, int H, int W,
                                float clip, int inclusive, void* stream) {
    if (!logits || !score || !work || B <= 0 || K <= 0) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(minmax_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, work, B);
    dim3 grid(grid_for(HW, 256, 1024), B);
    hipLaunchKernelGGL(dissum_kernel, grid, dim3(256), 0, st, logits, score, work, K, HW, clip, inclusive);
    hipLaunchKernelGGL(minmax_norm_kernel, grid, dim3(256), 0, st, score, work, HW);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_novel_relabel(const float* feats, const float* logits, const float* proto, int64_t* preds,
                                 int B, int C, int K, int H, int W, float thresh, int64_t new_label,
                                 void* stream) {
    if (!feats || !logits || !proto || !preds) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(novel_relabel_kernel, dim3(grid_for(B * HW, 256, 256 * 16)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), feats, logits, proto, preds, B, C, K, HW, thresh,
                       new_label);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_open_world_post(const float* logits, const float* feats, const float* protos,
                                   const int64_t* new_labels, int64_t* preds, float* msp, float* score, float* work,
                                   int B, int C, int K, int H, int W, int N, float thresh, int vs_known, float clip,
                                   int inclusive, void* stream) {
    const int rc = open_world_check(logits, feats, protos, new_labels, preds, B, C, K, H, W, N);
    if (rc != 0) return rc;
    if (score && !work) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (score) hipLaunchKernelGGL(minmax_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, work, B);
    open_world_launch<true>(logits, feats, protos, new_labels, preds, msp, score, work, B, C, K, HW, N, thresh, vs_known,
                            clip, inclusive, st);
    if (score)
        hipLaunchKernelGGL(minmax_norm_kernel, dim3(grid_for(HW, 256, 1024), B), dim3(256), 0, st, score, work, HW);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_novel_relabel_multi(const float* feats, const float* logits, const float* protos,
                                       const int64_t* new_labels, int64_t* preds, int B, int C, int K, int H, int W,
                                       int N, float thresh, int vs_known, void* stream) {
    const int rc = open_world_check(logits, feats, protos, new_labels, preds, B, C, K, H, W, N);
    if (rc != 0) return rc;
    if (N == 0) return 0;
    open_world_launch<false>(logits, feats, protos, new_labels, preds, nullptr, nullptr, nullptr, B, C, K, (int64_t)H * W,
                             N, thresh, vs_known, 0.f, 0, static_cast<hipStream_t>(stream));
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_dissum_msp_score(const float* logits, float* conf, float* work, int B, int K, int H, int W, int k_first,
                                    float clip, float threshold, float slope, int prob_logit, void* stream) {
    if (!logits || !conf || !work || B <= 0 || K <= 0 || H <= 0 || W <= 0 || k_first < 0 || k_first >= K) return DML_EINVAL;
    if (K - k_first > MAXC || B > 65535) return DML_EUNSUPPORTED;
    // the image index is the grid's y; 2^40 pixels keep every offset into the maps inside int64
    if ((int64_t)H * W > (1ll << 40) / B) return DML_EUNSUPPORTED;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* smap = work + 4 * (int64_t)B;
    float* mmap = smap + (int64_t)B * HW;
    // with H W % 4 == 0 every plane, every image of the maps and the first class's plane keep the base pointer's alignment
    const bool vec_maps = HW % 4 == 0 && aligned16(work);
    const bool vec1 = vec_maps && aligned16(logits), vec2 = vec_maps && aligned16(conf);    const bool reg = K - k_first <= MIX_KREG;
    hipLaunchKernelGGL(minmax_init_kernel, dim3((2 * B + 63) / 64), dim3(64), 0, st, work, 2 * B);
    const dim3 grid1(grid_for(vec1 ? HW / 4 : HW, 256, reg ? MIX_GRID_REG : MIX_GRID_REREAD), B);
    const dim3 grid2(grid_for(vec2 ? HW / 4 : HW, 256, 2048), B);
#define MIX_MAPS(PX, REG)                                                                                              \
    hipLaunchKernelGGL((dissum_msp_maps_kernel<PX, REG>), grid1, dim3(256), 0, st, logits, smap, mmap, work, K, k_first, \
                       HW, clip, prob_logit)
    if (vec1 && reg) MIX_MAPS(4, true);
    else if (vec1) MIX_MAPS(4, false);
    else if (reg) MIX_MAPS(1, true);
    else MIX_MAPS(1, false);
#undef MIX_MAPS
    if (vec2)
        hipLaunchKernelGGL(dissum_msp_mix_kernel<4>, grid2, dim3(256), 0, st, smap, mmap, work, conf, HW, threshold, slope);
    else
        hipLaunchKernelGGL(dissum_msp_mix_kernel<1>, grid2, dim3(256), 0, st, smap, mmap, work, conf, HW, threshold, slope);
    DML_LAUNCH_CHECK();
    return 0;
}
