// Reconstruction-consistency score of the anomaly sub-project's second open-set driver (anomaly/eval_ood_rec.py:90-150 of the
// reference, `--ood rec`): the decoder's pyramid concat of a frame and of its reconstruction, each the mean over the n resized copies
// of its bilinear resize to (Hq, Wq) = (H / 4, W / 4), compared by cosine similarity; that map, resized to (H, W), is the confidence
// wherever the maximum score does not exceed a threshold.
//
// dml_rec_cosine: one launch, no workspace.  The reference adds n full-size resizes into two [C, Hq, Wq] fp32 tensors; here the sum
// over the scales is taken per output pixel and channel in registers and only the three channel sums (a1.a2, |a1|^2, |a2|^2) survive.
// A workgroup owns a strip of REC_TX output pixels of one row.  A thread owns 4 channels of a 1024-channel chunk: the channels of a
// source pixel are contiguous, so a wave reads 256 consecutive channels per load.  Walking the strip, a thread keeps per scale and
// input the two source columns its pixel lies between, already blended over the two source rows; a column is loaded once per strip
// (2 loads) and serves every output pixel between it and its neighbour.  Rows share their source rows through L2: strips are
// numbered row by row and every eighth workgroup id, which is what shares an L2, takes consecutive numbers.  Per pixel and chunk a
// thread adds its three partial sums to its own LDS slots; at the end wave v folds pixels v, v + 4, ... over the 256 slots in a fixed
// order.  No atomics, no dependence on placement: bitwise reproducible.
//
// dml_rec_confidence: one launch, one thread per pixel of (H, W): the maximum (soft-max) score over the classes from first_class on,
// the four bilinear taps of cos, and the gate.
#include "common.h"

namespace {

constexpr int REC_TX = 16, REC_THREADS = 256, REC_MAXS = DML_REC_MAX_SCALES, REC_W = 4;

struct RecArgs {
    const void* f1[REC_MAXS];
    const void* f2[REC_MAXS];
    int h[REC_MAXS], w[REC_MAXS], ld[REC_MAXS];
    float sy[REC_MAXS], sx[REC_MAXS];
    int n, C, Hq, Wq;
};

// W consecutive channels as floats: 16 bytes of fp32 or 8 bytes of bf16 for W = 4, one element for W = 1
template <typename T, int W> struct RecLoad;
template <> struct RecLoad<float, 4> {
    __device__ static __forceinline__ void ld(const float* p, float (&v)[4]) { Vec16<float>::load(p, v); }
};
template <> struct RecLoad<bf16_t, 4> {
    __device__ static __forceinline__ void ld(const bf16_t* p, float (&v)[4]) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    }
};
template <typename T> struct RecLoad<T, 1> {
    __device__ static __forceinline__ void ld(const T* p, float (&v)[1]) { v[0] = Elem<T>::ld(p); }
};

// One thread, W channels from channel c on, the nx pixels of the strip at row y from column x0: adds the thread's partial sums of
// pixel p to part[(p * 3 + j) * REC_THREADS + tid].  Every branch on an index is uniform over the workgroup.
template <typename T, int W, int NS>
__device__ __forceinline__ void rec_walk(const RecArgs& a, int b, int y, int x0, int nx, int c, float inv_n, float* __restrict__ part,
                                         int tid) {
    int ro0[NS], ro1[NS];          // element offsets of the two source rows of this output row (uniform; below 2^31, see the launch)
    float ly0[NS], ly1[NS];
    float va[2][NS][W], vb[2][NS][W];      // columns ja / jb, blended over the two rows
    int ja[NS], jb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        ja[s] = jb[s] = -1;
        if (s < a.n) {
            const Tap ly = src_tap(a.sy[s], y, a.h[s]);
            ly0[s] = ly.l0; ly1[s] = ly.l1;
            ro0[s] = ((b * a.h[s] + ly.i0) * a.w[s]) * a.ld[s];
            ro1[s] = ((b * a.h[s] + ly.i1) * a.w[s]) * a.ld[s];
        }
    }
    for (int p = 0; p < nx; ++p) {
        float acc[2][W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[0][e] = acc[1][e] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s < a.n) {
                const Tap lx = src_tap(a.sx[s], x0 + p, a.w[s]);
                const int ld = a.ld[s];
                const T* base[2] = {static_cast<const T*>(a.f1[s]) + c, static_cast<const T*>(a.f2[s]) + c};
                if (lx.i0 != ja[s]) {
                    if (lx.i0 == jb[s]) {
#pragma unroll
                        for (int k = 0; k < 2; ++k)
#pragma unroll
                            for (int e = 0; e < W; ++e) va[k][s][e] = vb[k][s][e];
                    } else {
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            float t0[W], t1[W];
                            RecLoad<T, W>::ld(base[k] + (ro0[s] + lx.i0 * ld), t0);
                            RecLoad<T, W>::ld(base[k] + (ro1[s] + lx.i0 * ld), t1);
#pragma unroll
                            for (int e = 0; e < W; ++e) va[k][s][e] = ly0[s] * t0[e] + ly1[s] * t1[e];
                        }
                    }
                    ja[s] = lx.i0;
                }
                if (lx.i1 != jb[s]) {
                    if (lx.i1 == ja[s]) {
#pragma unroll
                        for (int k = 0; k < 2; ++k)
#pragma unroll
                            for (int e = 0; e < W; ++e) vb[k][s][e] = va[k][s][e];
                    } else {
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            float t0[W], t1[W];
                            RecLoad<T, W>::ld(base[k] + (ro0[s] + lx.i1 * ld), t0);
                            RecLoad<T, W>::ld(base[k] + (ro1[s] + lx.i1 * ld), t1);
#pragma unroll
                            for (int e = 0; e < W; ++e) vb[k][s][e] = ly0[s] * t0[e] + ly1[s] * t1[e];
                        }
                    }
                    jb[s] = lx.i1;
                }
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int e = 0; e < W; ++e) acc[k][e] += lx.l0 * va[k][s][e] + lx.l1 * vb[k][s][e];
            }
        }
        float d = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float a1 = acc[0][e] * inv_n, a2 = acc[1][e] * inv_n;
            d = fmaf(a1, a2, d); s1 = fmaf(a1, a1, s1); s2 = fmaf(a2, a2, s2);
        }
        float* q = part + p * 3 * REC_THREADS + tid;
        q[0] += d; q[REC_THREADS] += s1; q[2 * REC_THREADS] += s2;
    }
}

// VEC: every pointer and every ld allow a load of 4 channels (16 bytes of fp32, 8 of bf16); the C % 4 last channels go one by one.
// Otherwise one channel per thread and step.
template <typename T, bool VEC, int NS>
__global__ __launch_bounds__(REC_THREADS) void rec_cosine_kernel(RecArgs a, float* __restrict__ cosv, int nxs, int nblk) {
    __shared__ float part[REC_TX * 3 * REC_THREADS];
    const int tid = threadIdx.x;
    // workgroup ids that share an L2 (id % 8) take consecutive strips; a bijection for every nblk
    const int bid = blockIdx.x, q8 = nblk / 8, r8 = nblk % 8, xcd = bid % 8, idx = bid / 8;
    const int lb = xcd < r8 ? xcd * (q8 + 1) + idx : r8 * (q8 + 1) + (xcd - r8) * q8 + idx;
    const int xs = lb % nxs, y = (lb / nxs) % a.Hq, b = lb / (nxs * a.Hq);
    const int x0 = xs * REC_TX, nx = min(REC_TX, a.Wq - x0);
    const float inv_n = 1.f / (float)a.n;
    for (int i = tid; i < REC_TX * 3 * REC_THREADS; i += REC_THREADS) part[i] = 0.f;     // a thread clears its own slots only
    const int C = a.C;
    if constexpr (VEC) {
        const int nvec = C / REC_W;
        for (int v = tid; v < nvec; v += REC_THREADS) rec_walk<T, REC_W, NS>(a, b, y, x0, nx, v * REC_W, inv_n, part, tid);
        if (tid < C - nvec * REC_W) rec_walk<T, 1, NS>(a, b, y, x0, nx, nvec * REC_W + tid, inv_n, part, tid);
    } else {
        for (int c = tid; c < C; c += REC_THREADS) rec_walk<T, 1, NS>(a, b, y, x0, nx, c, inv_n, part, tid);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int p = wave; p < nx; p += REC_THREADS / 64) {
        float t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float* q = part + (p * 3 + j) * REC_THREADS + lane;
            t[j] = wave_sum((q[0] + q[64]) + (q[128] + q[192]));
        }
        if (lane == 0) {
            // u_k = a_k / max(|a_k|, 1e-12) (F.normalize), cos = sum (u_1 / max(|u_1|, 1e-8)) (u_2 / max(|u_2|, 1e-8))
            // (F.cosine_similarity); |u_k| = |a_k| / max(|a_k|, 1e-12).  An all-zero vector gives d = 0 and 0 / 1e-8 = 0.
            const float n1 = sqrtf(t[1]), n2 = sqrtf(t[2]);
            const float m1 = fmaxf(n1, 1e-12f), m2 = fmaxf(n2, 1e-12f);
            const float du = (t[0] / m1) / m2;
            cosv[((int64_t)b * a.Hq + y) * a.Wq + x0 + p] = du / (fmaxf(n1 / m1, 1e-8f) * fmaxf(n2 / m2, 1e-8f)) + 0.f;
        }
    }
}

// conf = msp > threshold ? msp : bilinear(cos -> (H, W)); msp = max_c tmp (prob_logit) or max_c softmax(tmp), tmp = scores[:, k_first:]
__global__ __launch_bounds__(256) void rec_confidence_kernel(const float* __restrict__ scores, const float* __restrict__ cosv,
                                                             float* __restrict__ conf, int B, int K, int H, int W, int Hq, int Wq,
                                                             int k_first, float threshold, int prob_logit, float sy, float sx) {
    const int64_t plane = (int64_t)H * W, total = (int64_t)B * plane;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / plane);
        const int64_t px = i - (int64_t)b * plane;
        const int Y = (int)(px / W), X = (int)(px - (int64_t)Y * W);
        const float* sp = scores + ((int64_t)b * K + k_first) * plane + px;
        float m = *sp, sum = 1.f;          // running maximum and sum of exp(v - m)
        for (int c = 1; c < K - k_first; ++c) {
            const float v = sp[(int64_t)c * plane];
            if (v > m) {
                sum = sum * __expf(m - v) + 1.f;
                m = v;
            } else {
                sum += __expf(v - m);
            }
        }
        const float msp = prob_logit ? m : 1.f / sum;
        const Tap ly = src_tap(sy, Y, Hq), lx = src_tap(sx, X, Wq);
        const float* c0 = cosv + ((int64_t)b * Hq + ly.i0) * Wq;
        const float* c1 = cosv + ((int64_t)b * Hq + ly.i1) * Wq;
        const float rec = ly.l0 * (lx.l0 * c0[lx.i0] + lx.l1 * c0[lx.i1]) + ly.l1 * (lx.l0 * c1[lx.i0] + lx.l1 * c1[lx.i1]);
        conf[i] = msp > threshold ? msp : rec;
    }
}

}  // namespace

extern "C" int dml_rec_cosine(const void* const* f1, const void* const* f2, const int* h, const int* w, const int* ld, int n, int B,
                              int C, int dtype, float* cosv, int Hq, int Wq, void* stream) {
    if (!f1 || !f2 || !h || !w || !ld || !cosv || n < 1 || n > REC_MAXS || B <= 0 || C <= 0 || Hq <= 0 || Wq <= 0) return DML_EINVAL;
    if (dtype != DML_F32 && dtype != DML_BF16) return DML_EINVAL;
    const int es = dtype == DML_BF16 ? 2 : 4;
    RecArgs a;
    bool vec = true;
    for (int s = 0; s < REC_MAXS; ++s) {
        const int k = s < n ? s : 0;          // unused entries repeat scale 0: never read, never wild
        if (!f1[k] || !f2[k] || h[k] <= 0 || w[k] <= 0 || ld[k] < C) return DML_EINVAL;
        // the kernel's element offsets are 32-bit
        if ((int64_t)B * h[k] * w[k] * ld[k] > (1ll << 31) - 1) return DML_EUNSUPPORTED;
        a.f1[s] = f1[k]; a.f2[s] = f2[k];
        a.h[s] = h[k]; a.w[s] = w[k]; a.ld[s] = ld[k];
        a.sy[s] = (float)h[k] / (float)Hq; a.sx[s] = (float)w[k] / (float)Wq;
        vec = vec && ld[k] % REC_W == 0 && aligned_to(REC_W * es, f1[k], f2[k]);
    }
    a.n = n; a.C = C; a.Hq = Hq; a.Wq = Wq;
    const int nxs = (Wq + REC_TX - 1) / REC_TX;
    const int64_t nblk = (int64_t)B * Hq * nxs;
    if (nblk > (1ll << 31) - 1) return DML_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)nblk), block(REC_THREADS);
    // NS: the scales the walk is unrolled for -- 5 (StreetHazards' count) keeps the column cache within two waves per SIMD
#define REC_LAUNCH(T, VEC)                                                                                          \
    do {                                                                                                            \
        if (n <= 5) hipLaunchKernelGGL((rec_cosine_kernel<T, VEC, 5>), grid, block, 0, st, a, cosv, nxs, (int)nblk); \
        else hipLaunchKernelGGL((rec_cosine_kernel<T, VEC, REC_MAXS>), grid, block, 0, st, a, cosv, nxs, (int)nblk); \
    } while (0)
    if (dtype == DML_BF16) {
        if (vec) REC_LAUNCH(bf16_t, true);
        else REC_LAUNCH(bf16_t, false);
    } else {
        if (vec) REC_LAUNCH(float, true);
        else REC_LAUNCH(float, false);
    }
#undef REC_LAUNCH
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_rec_confidence(const float* scores, const float* cosv, float* conf, int B, int K, int H, int W, int Hq, int Wq,
                                  int k_first, float threshold, int prob_logit, void* stream) {
    if (!scores || !cosv || !conf || B <= 0 || K <= 0 || H <= 0 || W <= 0 || Hq <= 0 || Wq <= 0 || k_first < 0 || k_first >= K)
        return DML_EINVAL;
    if (K - k_first > MAXC) return DML_EINVAL;
    if ((int64_t)H * W > (1ll << 40) / B || (int64_t)B * Hq * Wq > (1ll << 40)) return DML_EUNSUPPORTED;
    hipLaunchKernelGGL(rec_confidence_kernel, dim3(grid_for((int64_t)B * H * W, 256, 256 * 32)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), scores, cosv, conf, B, K, H, W, Hq, Wq, k_first, threshold, prob_logit,
                       (float)Hq / (float)H, (float)Wq / (float)W);
    DML_LAUNCH_CHECK();
    return 0;
}
