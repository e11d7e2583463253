// Pixel -> prototype squared-Euclidean-distance head, its backward, the DML loss and the open-world
// scores, for gfx950.  All HBM-bound (about 4 flop/byte): one lane owns 4 consecutive pixels so that
// every global access is a 16-byte vector; prototypes sit in LDS and are read as broadcasts.
//
// Replaces network/utils.py:92-118 (the reference materialises a B x HW x K x C tensor twice),
// utils/loss.py:34-42 / anomaly/models/models.py:42-78 (per-image per-class Python loop with host
// round trips), and the host numpy post-processing of test_embedding.py:339-350,428-445 and
// anomaly/eval_ood_traditional.py:301-305.
#include "common.h"
#include <cstdlib>

namespace {

// non-temporal stores of logits / features: standalone head 0.378 -> 0.358 ms, staged x4 kernel 0.237 -> 0.219 ms
// (tools/bench_dist_variants.py, 768 x 768 x 16)
constexpr bool DIST_NT_DEFAULT = true;
constexpr int MAXC = 32, MAXK = 33;   // embedding dim / prototype count supported by these kernels

// 16-byte store of an output that nobody re-reads from cache (logits / features: 1.2 GB per step, far beyond L2):
// NT = true marks it non-temporal
template <bool NT> __device__ __forceinline__ void store4(float* p, const float4 v) {
    if constexpr (NT) {
        typedef float f32x4_nt __attribute__((ext_vector_type(4)));
        f32x4_nt t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<f32x4_nt*>(p));
    } else {
        *reinterpret_cast<float4*>(p) = v;
    }
}

// ---- bilinear resize, align_corners = False (F.interpolate at network/utils.py:88): the two source taps of output
// index I on an axis of n samples at scale s = n / N, and the blend of the four samples they select.  Every kernel that
// resizes the embedding goes through these two, so they all see the same coordinates and weights.
struct Tap {
    int i0, i1;        // clamped neighbours (i1 == i0 on the last sample)
    float l0, l1;      // their weights
};
__device__ __forceinline__ Tap src_tap(float s, int I, int n) {
    float sI = s * ((float)I + 0.5f) - 0.5f;
    sI = sI < 0.f ? 0.f : sI;
    Tap t;
    t.i0 = min((int)sI, n - 1);
    t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
    t.l1 = sI - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
__device__ __forceinline__ float bilerp(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
    return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

__device__ __forceinline__ void load_protos(float* sp, const float* __restrict__ protos, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = protos[i];
    __syncthreads();
}

// logits for PX pixels held as f[c][px]; writes NCHW planes / argmax / dissum
template <int PX, int CM>
__device__ __forceinline__ void dist_and_store(const float (&f)[CM][PX], const float* sp, int C, int K,
                                               float* __restrict__ logits, uint8_t* __restrict__ argmax,
                                               float* __restrict__ dissum, int64_t plane, int64_t pix_in_img,
                                               int64_t img_base_logits, int64_t img_pix_base) {
    float best[PX], sum[PX];
    int bi[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) { best[p] = -INFINITY; bi[p] = 0; sum[p] = 0.f; }
    for (int k = 0; k < K; ++k) {
        float d[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) d[p] = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if (c < C) {
                const float m = sp[k * C + c];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const float t = f[c][p] - m;
                    d[p] += t * t;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float lg = -d[p];
            d[p] = lg;
            sum[p] += d[p];
            if (lg > best[p]) { best[p] = lg; bi[p] = k; }
        }
        if (logits != nullptr) {
            float* o = logits + img_base_logits + (int64_t)k * plane + pix_in_img;
            if constexpr (PX == 4) *reinterpret_cast<float4*>(o) = make_float4(d[0], d[1], d[2], d[3]);
            else o[0] = d[0];
        }
    }
    if (argmax != nullptr) {
#pragma unroll
        for (int p = 0; p < PX; ++p) argmax[img_pix_base + pix_in_img + p] = (uint8_t)bi[p];
    }
    if (dissum != nullptr) {
#pragma unroll
        for (int p = 0; p < PX; ++p) dissum[img_pix_base + pix_in_img + p] = -sum[p];
    }
}

template <int PX, int CM>
__device__ __forceinline__ void store_feats(const float (&f)[CM][PX], int C, float* __restrict__ feats,
                                            int64_t pix_global) {
    if (feats == nullptr) return;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        float* o = feats + (pix_global + p) * C;
        if ((C & 3) == 0) {
#pragma unroll
            for (int c = 0; c < CM; c += 4)
                if (c < C) *reinterpret_cast<float4*>(o + c) = make_float4(f[c][p], f[c + 1][p], f[c + 2][p], f[c + 3][p]);
        } else {
#pragma unroll
            for (int c = 0; c < CM; ++c)
                if (c < C) o[c] = f[c][p];
        }
    }
}

// ---- standalone head: x NCHW (what F.interpolate returns) -> logits NCHW, features NHWC
template <int PX, int CM>
__global__ __launch_bounds__(256) void proto_dist_fwd_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ protos,
                                                             float* __restrict__ logits, float* __restrict__ feats,
                                                             uint8_t* __restrict__ argmax,
                                                             float* __restrict__ dissum, int B, int C, int K,
                                                             int64_t HW) {
    __shared__ float sp[MAXK * MAXC];
    load_protos(sp, protos, K * C);
    const int64_t groups_per_img = HW / PX;
    const int64_t total = (int64_t)B * groups_per_img;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / groups_per_img;
        const int64_t pix = (i - b * groups_per_img) * PX;
        float f[CM][PX];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if (c < C) {
                const float* src = x + (b * C + c) * HW + pix;
                if constexpr (PX == 4) {
                    const float4 t = *reinterpret_cast<const float4*>(src);
                    f[c][0] = t.x; f[c][1] = t.y; f[c][2] = t.z; f[c][3] = t.w;
                } else {
                    f[c][0] = src[0];
                }
            }
        }
        store_feats<PX, CM>(f, C, feats, b * HW + pix);
        dist_and_store<PX, CM>(f, sp, C, K, logits, argmax, dissum, HW, pix, b * K * HW, b * HW);
    }
}

// ---- per-wave NHWC <-> "4 pixels per lane" transposition through a 16 KB LDS image (C = 16 floats per pixel).
// Lane l owns pixel groups wave_first + l (4 pixels = 256 B = 16 chunks of 16 B).  Global accesses are issued so
// that lane l touches chunk j*64 + l of the wave's contiguous 16 KB: 1 KB of consecutive bytes per instruction.
template <bool NT = false>
__device__ __forceinline__ void wave_store_nhwc16(float4* st, const float (&f)[16][4], float* __restrict__ dst,
                                                  int lane, int64_t wave_first, int64_t total) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4)
            st[lane * 16 + ((p * 4 + c4) ^ (lane & 15))] =
                make_float4(f[c4 * 4][p], f[c4 * 4 + 1][p], f[c4 * 4 + 2][p], f[c4 * 4 + 3][p]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int q = j * 64 + lane, r = q >> 4;
        const float4 v = st[r * 16 + ((q & 15) ^ (r & 15))];
        if (wave_first + r < total) store4<NT>(dst + (wave_first + r) * 64 + (q & 15) * 4, v);
    }
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void wave_load_nhwc16(float4* st, float (&f)[16][4], const float* __restrict__ src,
                                                 int lane, int64_t wave_first, int64_t total) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int q = j * 64 + lane, r = q >> 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (wave_first + r < total) v = *reinterpret_cast<const float4*>(src + (wave_first + r) * 64 + (q & 15) * 4);
        st[r * 16 + ((q & 15) ^ (r & 15))] = v;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const float4 v = st[lane * 16 + ((p * 4 + c4) ^ (lane & 15))];
            f[c4 * 4][p] = v.x; f[c4 * 4 + 1][p] = v.y; f[c4 * 4 + 2][p] = v.z; f[c4 * 4 + 3][p] = v.w;
        }
    __builtin_amdgcn_wave_barrier();
}

// The same store in two halves (pixels 0-1, then 2-3) through an 8 KB-per-wave image: a 256-thread workgroup then needs
// 32 KB of LDS instead of 64 KB.  Store instruction j of a half covers chunks j*64 + lane of the wave's 8 KB: 128
// contiguous bytes per 8 lanes.  `bound`: first pixel group that must not be written.
template <bool NT>
__device__ __forceinline__ void wave_store_nhwc16_halves(float4* st, const float (&f)[16][4], float* __restrict__ dst,
                                                         int lane, int64_t wave_first, int64_t bound) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int p = half * 2 + pp;
                st[lane * 8 + ((pp * 4 + c4) ^ (lane & 7))] =
                    make_float4(f[c4 * 4][p], f[c4 * 4 + 1][p], f[c4 * 4 + 2][p], f[c4 * 4 + 3][p]);
            }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int qq = j * 64 + lane, r = qq >> 3;
            const float4 v = st[r * 8 + ((qq & 7) ^ (r & 7))];
            if (wave_first + r < bound) store4<NT>(dst + (wave_first + r) * 64 + half * 32 + (qq & 7) * 4, v);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- fused upsample + head, K = C = 16: one pixel group per lane, features stored through the LDS transpose
template <bool NT>
__global__ __launch_bounds__(256) void upsample_dist_fwd_c16_kernel(const float* __restrict__ e,
                                                                    const float* __restrict__ protos,
                                                                    float* __restrict__ logits,
                                                                    float* __restrict__ feats, int B, int h, int w,
                                                                    int H, int W, float sy, float sx) {
    constexpr int C = 16, K = 16;
    __shared__ __attribute__((aligned(16))) float4 stage[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int WG = W / 4;
    const int64_t HW = (int64_t)H * W, groups_per_img = HW / 4, total = (int64_t)B * groups_per_img;
    const int64_t wave_first = ((int64_t)blockIdx.x * 4 + wave) * 64;
    const int64_t i = wave_first + lane;
    const bool active = i < total;
    const int64_t ic = active ? i : total - 1;
    const int b = (int)(ic / groups_per_img);
    const int64_t g = ic - (int64_t)b * groups_per_img;
    const int Y = (int)(g / WG), xg = (int)(g - (int64_t)Y * WG);
    const Tap ty = src_tap(sy, Y, h);
    const float* r0 = e + ((int64_t)b * h + ty.i0) * w * C;
    const float* r1 = e + ((int64_t)b * h + ty.i1) * w * C;
    float f[C][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const Tap tx = src_tap(sx, xg * 4 + p, w);
#pragma unroll
        for (int c = 0; c < C; c += 4) {
            const float4 a = *reinterpret_cast<const float4*>(r0 + tx.i0 * C + c);
            const float4 bq = *reinterpret_cast<const float4*>(r0 + tx.i1 * C + c);
            const float4 cq = *reinterpret_cast<const float4*>(r1 + tx.i0 * C + c);
            const float4 d = *reinterpret_cast<const float4*>(r1 + tx.i1 * C + c);
            f[c][p] = bilerp(ty, tx, a.x, bq.x, cq.x, d.x);
            f[c + 1][p] = bilerp(ty, tx, a.y, bq.y, cq.y, d.y);
            f[c + 2][p] = bilerp(ty, tx, a.z, bq.z, cq.z, d.z);
            f[c + 3][p] = bilerp(ty, tx, a.w, bq.w, cq.w, d.w);
        }
    }
    if (feats != nullptr) wave_store_nhwc16<NT>(stage[wave], f, feats, lane, wave_first, total);
    const int64_t pix = g * 4;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = protos[k * C + c];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float t = f[c][p] - m;
                d[p] += t * t;
            }
        }
        if (logits != nullptr && active)
            store4<NT>(logits + ((int64_t)b * K + k) * HW + pix, make_float4(-d[0], -d[1], -d[2], -d[3]));
    }
}

// ---- the same for an exact x4 upsample (H = 4h, W = 4w: the DeepLabV3+ head, network/utils.py:88) with the low-resolution
// operand staged in LDS.  A workgroup owns a band of up to four output rows that interpolate between the SAME two
// low-resolution rows (rows 4j+2 .. 4j+5 lie between rows j and j+1) and 256 output columns: 2 x 66 low-resolution
// pixels = 8.4 KB are fetched once, coalesced, instead of 64 gathered 16-byte loads per lane; each lane then blends the
// two rows for its three source columns and forms its 4 pixels with three weights per pixel.  The NHWC copy goes out
// through an 8 KB-per-wave transposition in two halves, so a workgroup needs 40 KB of LDS (4 per CU, the gathered
// kernel's 64 KB allow 2).
template <bool NT>
__global__ __launch_bounds__(256) void upsample4_dist_fwd_c16_kernel(const float* __restrict__ e,
                                                                     const float* __restrict__ protos,
                                                                     float* __restrict__ logits,
                                                                     float* __restrict__ feats, int B, int h, int w) {
    constexpr int C = 16, K = 16, COLS = 66;
    __shared__ __attribute__((aligned(16))) float4 low[2][COLS][4];       // [row][column][16-byte chunk, swizzled]
    __shared__ __attribute__((aligned(16))) float4 stage[4][512];         // per wave: 64 lanes x 2 pixels x 64 B
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = 4 * h, W = 4 * w;
    const int segs = (W + 255) / 256;
    int bid = blockIdx.x;
    const int seg = bid % segs;
    bid /= segs;
    const int jb = bid % (h + 1) - 1, b = bid / (h + 1);                  // band -1 .. h-1
    const int r0 = max(jb, 0), r1 = min(jb + 1, h - 1);
    const int Q0 = seg * 64;                                              // first low-resolution column of the segment
    for (int idx = tid; idx < 2 * COLS * 4; idx += 256) {
        const int row = idx / (COLS * 4), rem = idx - row * (COLS * 4);
        const int ci = rem >> 2, c4 = rem & 3;
        const int col = min(max(Q0 - 1 + ci, 0), w - 1);
        const float4 v = *reinterpret_cast<const float4*>(e + (((int64_t)b * h + (row ? r1 : r0)) * w + col) * C + c4 * 4);
        low[row][ci][c4 ^ (ci & 3)] = v;
    }
    __syncthreads();
    const int Y = 4 * jb + 2 + wave;
    if (Y < 0 || Y >= H) return;                                          // (whole waves: no barrier below)
    const Tap ty = src_tap(0.25f, Y, h);
    const int y0 = ty.i0;
    const float ly1 = ty.l1, ly0 = ty.l0;
    // y0 is r0 except on the last band's clamp, y1 = y0 + 1 clamped is r1 -- or both rows coincide
    const int ra = (y0 == r0) ? 0 : 1, rb = (min(y0 + 1, h - 1) == r1) ? 1 : 0;
    const int q = Q0 + lane;                                              // this lane's low-resolution column
    const bool active = q < w;
    // rows blended for the three source columns q-1, q, q+1 (LDS columns lane, lane+1, lane+2)
    float T[3][C];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
        const int ci = lane + s3;
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const float4 a = low[ra][ci][c4 ^ (ci & 3)], bq = low[rb][ci][c4 ^ (ci & 3)];
            T[s3][c4 * 4] = ly0 * a.x + ly1 * bq.x;
            T[s3][c4 * 4 + 1] = ly0 * a.y + ly1 * bq.y;
            T[s3][c4 * 4 + 2] = ly0 * a.z + ly1 * bq.z;
            T[s3][c4 * 4 + 3] = ly0 * a.w + ly1 * bq.w;
        }
    }
    float f[C][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const Tap tx = src_tap(0.25f, 4 * q + p, w);
        const int x0 = tx.i0, x1 = tx.i1;
        const float l1 = tx.l1, l0 = tx.l0;
        const float wl = (x0 == q - 1 ? l0 : 0.f) + (x1 == q - 1 ? l1 : 0.f);
        const float wc = (x0 == q ? l0 : 0.f) + (x1 == q ? l1 : 0.f);
        const float wr = (x0 == q + 1 ? l0 : 0.f) + (x1 == q + 1 ? l1 : 0.f);
#pragma unroll
        for (int c = 0; c < C; ++c) f[c][p] = wl * T[0][c] + wc * T[1][c] + wr * T[2][c];
    }
    const int64_t HW = (int64_t)H * W;
    const int64_t row_first = (((int64_t)b * H + Y) * W) / 4;             // first pixel group of this output row
    const int64_t wave_first = row_first + Q0, row_end = row_first + w;
    if (feats != nullptr) wave_store_nhwc16_halves<NT>(stage[wave], f, feats, lane, wave_first, row_end);
    if (logits == nullptr || !active) return;
    const int64_t pix = (int64_t)Y * W + 4 * q;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = protos[k * C + c];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float t = f[c][p] - m;
                d[p] += t * t;
            }
        }
        store4<NT>(logits + ((int64_t)b * K + k) * HW + pix, make_float4(-d[0], -d[1], -d[2], -d[3]));
    }
}

// ---- backward of the head, K = C = 16: df = -2 sum_k g_k (f - m_k) (+ gfeats); NHWC tensors through the transpose
__global__ __launch_bounds__(256) void proto_dist_bwd_c16_kernel(const float* __restrict__ glogits,
                                                                 const float* __restrict__ gfeats,
                                                                 const float* __restrict__ feats,
                                                                 const float* __restrict__ protos,
                                                                 float* __restrict__ df, int B, int64_t HW) {
    constexpr int C = 16, K = 16;
    __shared__ __attribute__((aligned(16))) float4 stage[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t groups_per_img = HW / 4, total = (int64_t)B * groups_per_img;
    const int64_t wave_first = ((int64_t)blockIdx.x * 4 + wave) * 64;
    const int64_t i = wave_first + lane;
    const bool active = i < total;
    const int64_t ic = active ? i : total - 1;
    const int64_t b = ic / groups_per_img;
    const int64_t pix = (ic - b * groups_per_img) * 4;
    float gs[4] = {0.f, 0.f, 0.f, 0.f};
    float o[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) o[c][p] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(glogits + (b * K + k) * HW + pix);
        const float g[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) gs[p] += g[p];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = protos[k * C + c];
#pragma unroll
            for (int p = 0; p < 4; ++p) o[c][p] += g[p] * m;              // sum_k g_k m_kc
        }
    }
    float f[C][4];
    wave_load_nhwc16(stage[wave], f, feats, lane, wave_first, total);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) o[c][p] = -2.f * (gs[p] * f[c][p] - o[c][p]);
    if (gfeats != nullptr) {
        wave_load_nhwc16(stage[wave], f, gfeats, lane, wave_first, total);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p) o[c][p] += f[c][p];
    }
    wave_store_nhwc16(stage[wave], o, df, lane, wave_first, total);
}

// ---- standalone head, K = C = 16 fast path (the reference's configuration).  Per lane: 4 consecutive pixels,
// 16-byte loads of the 16 channel planes, 16-byte stores of the 16 logit planes; the NHWC copy of the features is
// transposed through a per-wave 16 KB LDS image (XOR-swizzled 16-byte chunks) so that every store instruction
// writes 1 KB of consecutive addresses instead of 64 scattered 16-byte pieces.  Prototypes are read with a
// wave-uniform index (scalar loads), no LDS, no block barrier.
template <bool NT>
__global__ __launch_bounds__(256) void proto_dist_fwd_c16_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ protos,
                                                                 float* __restrict__ logits,
                                                                 float* __restrict__ feats,
                                                                 uint8_t* __restrict__ argmax,
                                                                 float* __restrict__ dissum, int B, int64_t HW) {
    constexpr int C = 16, K = 16;
    __shared__ __attribute__((aligned(16))) float4 stage[4][512];       // per wave: 64 lanes x 2 px x 64 B (two halves)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t groups_per_img = HW / 4;
    const int64_t total = (int64_t)B * groups_per_img;
    const int64_t wave_first = ((int64_t)blockIdx.x * 4 + wave) * 64;    // first pixel group of this wave
    const int64_t i = wave_first + lane;
    const bool active = i < total;
    const int64_t ic = active ? i : total - 1;
    const int64_t b = ic / groups_per_img;
    const int64_t pix = (ic - b * groups_per_img) * 4;
    float f[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 t = *reinterpret_cast<const float4*>(x + (b * C + c) * HW + pix);
        f[c][0] = t.x; f[c][1] = t.y; f[c][2] = t.z; f[c][3] = t.w;
    }
    // NHWC features: pixel group g of the flattened (image, pixel / 4) order sits at feats + g * 64 floats
    if (feats != nullptr) wave_store_nhwc16_halves<NT>(stage[wave], f, feats, lane, wave_first, total);
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = protos[k * C + c];                            // wave-uniform -> scalar load
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float t = f[c][p] - m;
                d[p] += t * t;
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            d[p] = -d[p];
            sum[p] += d[p];
            if (d[p] > best[p]) { best[p] = d[p]; bi[p] = k; }
        }
        if (logits != nullptr && active)
            store4<NT>(logits + (b * K + k) * HW + pix, make_float4(d[0], d[1], d[2], d[3]));
    }
    if (active) {
        if (argmax != nullptr)
#pragma unroll
            for (int p = 0; p < 4; ++p) argmax[b * HW + pix + p] = (uint8_t)bi[p];
        if (dissum != nullptr)
            *reinterpret_cast<float4*>(dissum + b * HW + pix) = make_float4(-sum[0], -sum[1], -sum[2], -sum[3]);
    }
}

// ---- fused: bilinear upsample of the low-resolution embedding e[B,h,w,C] + head at [H,W]
template <int PX, int CM>
__global__ __launch_bounds__(256) void upsample_dist_fwd_kernel(const float* __restrict__ e,
                                                                const float* __restrict__ protos,
                                                                float* __restrict__ logits,
                                                                float* __restrict__ feats,
                                                                uint8_t* __restrict__ argmax,
                                                                float* __restrict__ dissum, int B, int h, int w,
                                                                int C, int K, int H, int W, float sy, float sx) {
    __shared__ float sp[MAXK * MAXC];
    load_protos(sp, protos, K * C);
    const int WG = W / PX;
    const int64_t HW = (int64_t)H * W;
    const int64_t total = (int64_t)B * H * WG;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int xg = (int)(i % WG);
        int64_t t = i / WG;
        const int Y = (int)(t % H);
        const int b = (int)(t / H);
        const Tap ty = src_tap(sy, Y, h);
        const float* r0 = e + ((int64_t)b * h + ty.i0) * w * C;
        const float* r1 = e + ((int64_t)b * h + ty.i1) * w * C;
        float f[CM][PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const Tap tx = src_tap(sx, xg * PX + p, w);
            if ((C & 3) == 0) {
#pragma unroll
                for (int c = 0; c < CM; c += 4) {
                    if (c < C) {
                        const float4 a = *reinterpret_cast<const float4*>(r0 + tx.i0 * C + c);
                        const float4 bq = *reinterpret_cast<const float4*>(r0 + tx.i1 * C + c);
                        const float4 cq = *reinterpret_cast<const float4*>(r1 + tx.i0 * C + c);
                        const float4 d = *reinterpret_cast<const float4*>(r1 + tx.i1 * C + c);
                        f[c][p] = bilerp(ty, tx, a.x, bq.x, cq.x, d.x);
                        f[c + 1][p] = bilerp(ty, tx, a.y, bq.y, cq.y, d.y);
                        f[c + 2][p] = bilerp(ty, tx, a.z, bq.z, cq.z, d.z);
                        f[c + 3][p] = bilerp(ty, tx, a.w, bq.w, cq.w, d.w);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C)
                        f[c][p] = bilerp(ty, tx, r0[tx.i0 * C + c], r0[tx.i1 * C + c], r1[tx.i0 * C + c], r1[tx.i1 * C + c]);
                }
            }
        }
        const int64_t pix = (int64_t)Y * W + xg * PX;
        store_feats<PX, CM>(f, C, feats, (int64_t)b * HW + pix);
        dist_and_store<PX, CM>(f, sp, C, K, logits, argmax, dissum, HW, pix, (int64_t)b * K * HW, (int64_t)b * HW);
    }
}

// ---- merged prediction of the incremental multi-head model (test_self_distillation.py:292-297 of the reference) straight
// from the heads' low-resolution embeddings: no full-resolution logits or features exist.  With the prototypes 3 I_K
// (network/utils.py:103-106; a K = C + 1 head's last row, cut to the C carried channels, is zero)
//     -d_k = sum_c (f_c - 3 delta_kc)^2 = S + 9 - 6 f_k,  S = sum_c f_c^2 the same for every k    (k < C)
//     -d_C = S = S + 9 - 6 * 1.5
// so the first maximal d_k is the first maximal f_k over k < K, with 1.5 standing in for f_C.  The kernel compares the
// interpolated f_k themselves: K channels per tap instead of C, no S (whose rounding would only create ties), and exact
// ties of f stay exact ties of d.
struct PredictArgs {
    DmlPredictHead head[DML_PREDICT_MAX_HEADS];
    int n;
    unsigned vec;      // bit i: head i's rows can be read as 16-byte vectors
};

__device__ __forceinline__ int head_first_max(const DmlPredictHead& hd, bool vec, int b, const Tap& ty, const Tap& tx,
                                              int h, int w) {
    const int64_t ld = hd.ld;
    const float* r0 = hd.e + ((int64_t)b * h + ty.i0) * w * ld;
    const float* r1 = hd.e + ((int64_t)b * h + ty.i1) * w * ld;
    const float* p00 = r0 + tx.i0 * ld;
    const float* p01 = r0 + tx.i1 * ld;
    const float* p10 = r1 + tx.i0 * ld;
    const float* p11 = r1 + tx.i1 * ld;
    const int Kc = min(hd.K, hd.C);
    float best = -INFINITY;
    int bi = 0;
    if (vec) {
        for (int c = 0; c < Kc; c += 4) {              // (vec: C % 4 == 0, so c + 3 < C)
            const float4 a = *reinterpret_cast<const float4*>(p00 + c);
            const float4 bq = *reinterpret_cast<const float4*>(p01 + c);
            const float4 cq = *reinterpret_cast<const float4*>(p10 + c);
            const float4 d = *reinterpret_cast<const float4*>(p11 + c);
            const float v[4] = {bilerp(ty, tx, a.x, bq.x, cq.x, d.x), bilerp(ty, tx, a.y, bq.y, cq.y, d.y),
                                bilerp(ty, tx, a.z, bq.z, cq.z, d.z), bilerp(ty, tx, a.w, bq.w, cq.w, d.w)};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < Kc && v[j] > best) { best = v[j]; bi = c + j; }
        }
    } else {
        for (int c = 0; c < Kc; ++c) {
            const float v = bilerp(ty, tx, p00[c], p01[c], p10[c], p11[c]);
            if (v > best) { best = v; bi = c; }
        }
    }
    if (hd.K > hd.C && 1.5f > best) bi = hd.C;
    return bi;
}

// One lane owns two consecutive pixels of the flat [B H W] index space = one 16-byte store of preds.  `off` (0 / 1) shifts
// the pairs so that they start on a 16-byte boundary of preds: pair g is pixels 2 g - off, 2 g - off + 1, and a pair
// with only one pixel inside [0, total) -- the first one of a misaligned buffer, the last one of an odd count -- stores
// that pixel alone.
__global__ __launch_bounds__(256) void incremental_predict_kernel(const PredictArgs args, int64_t* __restrict__ preds,
                                                                  uint8_t* __restrict__ head_argmax, int B, int h,
                                                                  int w, int H, int W, float sy, float sx, int off) {
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW, pairs = (total + off + 1) / 2;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < pairs; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t first = 2 * g - off;
        // (b, Y, X) of the pair's first pixel inside the range; its neighbour follows by carry
        int64_t cur = first < 0 ? 0 : first;
        int b, Y, X;
        if (total <= 0x7fffffffll) {
            const unsigned u = (unsigned)cur, hw = (unsigned)HW;
            b = (int)(u / hw);
            const unsigned r = u - (unsigned)b * hw;
            Y = (int)(r / (unsigned)W);
            X = (int)(r - (unsigned)Y * (unsigned)W);
        } else {
            b = (int)(cur / HW);
            const int64_t r = cur - (int64_t)b * HW;
            Y = (int)(r / W);
            X = (int)(r - (int64_t)Y * W);
        }
        int64_t res[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t pix = first + p;
            res[p] = 0;
            if (pix < 0 || pix >= total) continue;
            if (pix != cur) {
                cur = pix;
                if (++X == W) { X = 0; if (++Y == H) { Y = 0; ++b; } }
            }
            const Tap ty = src_tap(sy, Y, h), tx = src_tap(sx, X, w);
            int pred = 0;
            for (int i = 0; i < args.n; ++i) {
                const int am = head_first_max(args.head[i], (args.vec >> i) & 1u, b, ty, tx, h, w);
                if (head_argmax != nullptr) head_argmax[(int64_t)i * total + pix] = (uint8_t)am;
                if (i == 0 || am == args.head[i].novel_id) pred = am;      // a later head overrides an earlier one
            }
            res[p] = pred;
        }
        if (first >= 0 && first + 1 < total) {
            typedef long long i64x2 __attribute__((ext_vector_type(2)));
            const i64x2 v = {(long long)res[0], (long long)res[1]};
            *reinterpret_cast<i64x2*>(preds + first) = v;
        } else {
            if (first >= 0 && first < total) preds[first] = res[0];
            if (first + 1 >= 0 && first + 1 < total) preds[first + 1] = res[1];
        }
    }
}

// ---- backward of the head: df = -2 sum_k g_k (f - m_k) (+ gfeats)
template <int PX, int CM>
__global__ __launch_bounds__(256) void proto_dist_bwd_kernel(const float* __restrict__ glogits,
                                                             const float* __restrict__ gfeats,
                                                             const float* __restrict__ feats,
                                                             const float* __restrict__ protos,
                                                             float* __restrict__ df, int B, int C, int K,
                                                             int64_t HW) {
    __shared__ float sp[MAXK * MAXC];
    load_protos(sp, protos, K * C);
    const int64_t groups_per_img = HW / PX;
    const int64_t total = (int64_t)B * groups_per_img;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / groups_per_img;
        const int64_t pix = (i - b * groups_per_img) * PX;
        float gs[PX];                 // sum_k g_k
        float gm[CM][PX];           // sum_k g_k m_kc
#pragma unroll
        for (int p = 0; p < PX; ++p) gs[p] = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c)
#pragma unroll
            for (int p = 0; p < PX; ++p) gm[c][p] = 0.f;
        for (int k = 0; k < K; ++k) {
            float g[PX];
            const float* src = glogits + (b * K + k) * HW + pix;
            if constexpr (PX == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
            } else {
                g[0] = src[0];
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) gs[p] += g[p];
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c < C) {
                    const float m = sp[k * C + c];
#pragma unroll
                    for (int p = 0; p < PX; ++p) gm[c][p] += g[p] * m;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int64_t o = (b * HW + pix + p) * C;
            if ((C & 3) == 0) {
#pragma unroll
                for (int c = 0; c < CM; c += 4) {
                    if (c < C) {
                        const float4 fv = *reinterpret_cast<const float4*>(feats + o + c);
                        float4 v;
                        v.x = -2.f * (gs[p] * fv.x - gm[c][p]);
                        v.y = -2.f * (gs[p] * fv.y - gm[c + 1][p]);
                        v.z = -2.f * (gs[p] * fv.z - gm[c + 2][p]);
                        v.w = -2.f * (gs[p] * fv.w - gm[c + 3][p]);
                        if (gfeats != nullptr) {
                            const float4 gq = *reinterpret_cast<const float4*>(gfeats + o + c);
                            v.x += gq.x; v.y += gq.y; v.z += gq.z; v.w += gq.w;
                        }
                        *reinterpret_cast<float4*>(df + o + c) = v;
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C) {
                        float v = -2.f * (gs[p] * feats[o + c] - gm[c][p]);
                        if (gfeats != nullptr) v += gfeats[o + c];
                        df[o + c] = v;
                    }
                }
            }
        }
    }
}

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
constexpr int MIX_MAXK = 32, MIX_KREG = 16;
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

template <int PX> __device__ __forceinline__ void mix_load(const float* p, float (&v)[PX]) {
    if constexpr (PX == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int PX> __device__ __forceinline__ void mix_store(float* p, const float (&v)[PX]) {
    if constexpr (PX == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
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
                if (k < Kn) mix_load<PX>(src + (int64_t)k * HW, v[k]);
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
            mix_load<PX>(src, v);
#pragma unroll
            for (int p = 0; p < PX; ++p) best[p] = v[p];
            for (int k = 0; k < Kn; ++k) {
                mix_load<PX>(src + (int64_t)k * HW, v);
#pragma unroll
                for (int p = 0; p < PX; ++p) { sum[p] += v[p]; best[p] = fmaxf(best[p], v[p]); }
            }
            if (!prob_logit) {
                for (int k = 0; k < Kn; ++k) {
                    mix_load<PX>(src + (int64_t)k * HW, v);
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
        mix_store<PX>(smap + (int64_t)b * HW + pix, s);
        mix_store<PX>(mmap + (int64_t)b * HW + pix, m);
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
        mix_load<PX>(smap + i, s);
        mix_load<PX>(mmap + i, m);
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float d = (s[p] - slo) / sden;
            const float q = (m[p] - mlo) / mden;
            const float c = 1.f / (1.f + expf(slope * (d - threshold)));
            out[p] = c * d + (1.f - c) * q;
        }
        mix_store<PX>(conf + i, out);
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

// 16-byte load of a stream that is read once (logits 134 MB, features 134 MB per 1024 x 2048 frame): NT marks it non-temporal
template <bool NT> __device__ __forceinline__ float4 load4(const float* p) {
    if constexpr (NT) {
        typedef float f32x4_nt __attribute__((ext_vector_type(4)));
        const f32x4_nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(p));
        return make_float4(t.x, t.y, t.z, t.w);
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}

template <int PX, bool NT> __device__ __forceinline__ void load_px(const float* p, float (&v)[PX]) {
    if constexpr (PX == 4) {
        const float4 t = load4<NT>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

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
                    *reinterpret_cast<float4*>(msp + i) =
                        make_float4(1.f - 1.f / den[0], 1.f - 1.f / den[1], 1.f - 1.f / den[2], 1.f - 1.f / den[3]);
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
                if constexpr (PX == 4) *reinterpret_cast<float4*>(score + i) = make_float4(s[0], s[1], s[2], s[3]);
                else score[i] = s[0];
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

// ---- DML loss
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
            if constexpr (PX == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)k * HW);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                v[0] = src[(int64_t)k * HW];
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                // online log-sum-exp: one pass over the K planes
                if (v[p] > mx[p]) { den[p] = den[p] * expf(mx[p] - v[p]) + 1.f; mx[p] = v[p]; bi[p] = k; }
                else den[p] += expf(v[p] - mx[p]);
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
    __shared__ double sh[4][4];
    double acc[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += (double)partials[(int64_t)i * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = wave_sum_d(acc[q]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[threadIdx.x >> 6][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        double v = sh[0][q] + sh[1][q] + sh[2][q] + sh[3][q];
        if (q == 2) v *= inv_hw;       // VAR = sum_i (1/HW_i) sum_valid(-logit_y), HW_i identical in a batch
        sums[q] = v;
    }
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
            if constexpr (PX == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)k * HW);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                v[0] = src[(int64_t)k * HW];
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                if (v[p] > mx[p]) { den[p] = den[p] * expf(mx[p] - v[p]) + 1.f; mx[p] = v[p]; }
                else den[p] += expf(v[p] - mx[p]);
            }
        }
        float inv[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) inv[p] = lab[p] == ignore_index ? 0.f : w_ce / den[p];
        for (int k = 0; k < K; ++k) {
            float v[PX], g[PX];
            if constexpr (PX == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)k * HW);   // L2-resident re-read
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                v[0] = src[(int64_t)k * HW];
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                g[p] = expf(v[p] - mx[p]) * inv[p];
                if ((int64_t)k == lab[p] && lab[p] != ignore_index) g[p] -= w_ce + w_var;
            }
            if constexpr (PX == 4) *reinterpret_cast<float4*>(dst + (int64_t)k * HW) = make_float4(g[0], g[1], g[2], g[3]);
            else dst[(int64_t)k * HW] = g[0];
        }
    }
}


// ---- fused backward of loss + distance head + final x4 upsample (C = K = 16, H = 4h, W = 4w).
// The unfused chain moves 394 B per full-resolution pixel (loss_bwd writes d loss / d logits, proto_dist_bwd reads it and
// writes d loss / d features, bilinear_bwd reads that); none of the two intermediates is needed by anyone else.  Here a
// workgroup owns a TJ x TI tile of the LOW-resolution embedding gradient.  Phase 1: for the (4 TJ + 4) x (4 TI + 8)
// full-resolution pixels that reach the tile, one work item = 4 consecutive pixels of a row: features (64 B) and label in,
// logits recomputed (-|f - m_k|^2, same arithmetic as the forward), softmax, d loss / d logits, d loss / d features, and
// the row's bilinear weights folded at once into three low-resolution column partials (left neighbour, own, right
// neighbour) that go to an LDS row buffer in three conflict-free sub-phases (deterministic: no atomics).  Phase 2: each
// thread gathers the <= 8 rows that reach its low-resolution pixel for 8 channels and writes 16 bytes.
// Traffic: 72 B per pixel (+ halo re-reads that hit in L2) + the low-resolution result.
constexpr int HB_TJ = 7, HB_TI = 14;                 // tile of the low-resolution map per workgroup
constexpr int HB_ROWS = 4 * HB_TJ + 4;               // 32 full-resolution rows reach it
constexpr int HB_GRPS = HB_TI + 2;                   // 16 groups of 4 pixels per row (one halo group each side)

template <typename TO>
__global__ __launch_bounds__(256) void head_bwd_fused_c16_kernel(
    const float* __restrict__ feats, const int64_t* __restrict__ labels, const double* __restrict__ sums,
    const float* __restrict__ gout, const float* __restrict__ protos, TO* __restrict__ de, int B, int h, int w,
    int64_t ignore_index, float alpha, float n_images_arg) {
    constexpr int C = 16, K = 16;
    __shared__ __attribute__((aligned(16))) float t[HB_ROWS][HB_GRPS][C];      // 32 KB: x-reduced rows
    const int tid = threadIdx.x;
    const int H = 4 * h, W = 4 * w;
    const int tiles_x = (w + HB_TI - 1) / HB_TI, tiles_y = (h + HB_TJ - 1) / HB_TJ;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y, b = bid / tiles_y;
    const int j0 = ty * HB_TJ, i0 = tx * HB_TI;
    const int Y0 = 4 * j0 - 2;                         // first full-resolution row of the region
    const int q0 = i0 - 1;                             // first pixel group of the region
    const float go = gout ? *gout : 1.f;
    const float n_images = n_images_arg > 0.f ? n_images_arg : (float)sums[4];
    const float w_ce = go / ((float)sums[1] * n_images);
    const float w_var = go * alpha / ((float)((int64_t)H * W) * n_images);
    // DIAGONAL prototype matrix (the reference's centers are 3 * I, network/utils.py:103-106): the distances collapse to
    // |f|^2 - 2 d_k f_k + d_k^2, whose |f|^2 cancels in the softmax, and sum_k g_k m_k to g_c d_c: ~250 VALU instructions per
    // pixel instead of ~1000 (the general path is VALU-bound at 18 % of the HBM roof).  Checked here, wave-uniformly, from the
    // 256 scalars themselves -- no flag in the ABI, any other matrix takes the general path.
    bool diag = true;
    float dk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = protos[k * C + c];
            if (c == k) dk[k] = v;
            else diag = diag && (v == 0.f);
        }
    }

    // two passes of 256 work items (16 rows x 16 groups each); a pass owns its rows of `t`, so the passes do not interact
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        const int id = it * 256 + tid;
        const int r = id / HB_GRPS, g = id - r * HB_GRPS;
        const int Y = Y0 + r, q = q0 + g;
        float pl[C], pc[C], pr[C];                     // column partials: left neighbour (q - 1), own (q), right (q + 1)
#pragma unroll
        for (int c = 0; c < C; ++c) { pl[c] = 0.f; pc[c] = 0.f; pr[c] = 0.f; }
        if (Y >= 0 && Y < H && q >= 0 && q < w) {
            // halo groups only reach the tile through their inner two pixels
            const int p_lo = (g == 0) ? 2 : 0, p_hi = (g == HB_GRPS - 1) ? 2 : 4;
            const float* frow = feats + (((int64_t)b * H + Y) * W + 4 * q) * C;
            const int64_t* lrow = labels + ((int64_t)b * H + Y) * W + 4 * q;
            // the next pixel's features / label are requested before the current pixel's ~1000 VALU instructions
            float4 nf[4];
            int64_t nlab = lrow[p_lo];
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) nf[c4] = *reinterpret_cast<const float4*>(frow + p_lo * C + c4 * 4);
#pragma unroll 1
            for (int p = p_lo; p < p_hi; ++p) {
                // keep the prototype loads (256 wave-uniform scalars) inside the iteration, 4 prototypes at a time:
                // hoisted out of the loop they need 256 SGPRs and spill
                asm volatile("" ::: "memory");
                float f[C];
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    f[c4 * 4] = nf[c4].x; f[c4 * 4 + 1] = nf[c4].y; f[c4 * 4 + 2] = nf[c4].z; f[c4 * 4 + 3] = nf[c4].w;
                }
                const int64_t lab = nlab;
                if (p + 1 < p_hi) {
                    nlab = lrow[p + 1];
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) nf[c4] = *reinterpret_cast<const float4*>(frow + (p + 1) * C + c4 * 4);
                }
                float lg[K];
                float mx = -INFINITY;
                const bool valid = lab != ignore_index;
                float gs = 0.f, gm[C];
                if (diag) {
                    // logit_k - logit_j = (2 d_k f_k - d_k^2) - (2 d_j f_j - d_j^2): softmax over t_k, |f|^2 drops out
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        lg[k] = dk[k] * (2.f * f[k] - dk[k]);
                        mx = fmaxf(mx, lg[k]);
                    }
                    float den = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        lg[k] = __expf(lg[k] - mx);          // v_exp_f32 (2 ulp): the softmax weights carry 1e-7 relative
                        den += lg[k];
                    }
                    const float inv = valid ? w_ce / den : 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        float gk = lg[k] * inv;
                        if (valid && (int64_t)k == lab) gk -= w_ce + w_var;
                        gs += gk;
                        gm[k] = gk * dk[k];                  // sum_k g_k m_k has one term per channel
                    }
                } else {
#pragma unroll 4
                    for (int k = 0; k < K; ++k) {          // prototypes: wave-uniform addresses -> scalar loads
                        float d = 0.f;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float u = f[c] - protos[k * C + c];
                            d += u * u;
                        }
                        lg[k] = -d;
                        mx = fmaxf(mx, lg[k]);
                    }
                    float den = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        lg[k] = expf(lg[k] - mx);
                        den += lg[k];
                    }
                    const float inv = valid ? w_ce / den : 0.f;
                    // d loss / d features = -2 sum_k g_k (f - m_k) = -2 (f sum_k g_k - sum_k g_k m_k)
#pragma unroll
                    for (int c = 0; c < C; ++c) gm[c] = 0.f;
#pragma unroll 4
                    for (int k = 0; k < K; ++k) {
                        float gk = lg[k] * inv;
                        if (valid && (int64_t)k == lab) gk -= w_ce + w_var;
                        gs += gk;
#pragma unroll
                        for (int c = 0; c < C; ++c) gm[c] += gk * protos[k * C + c];
                    }
                }
                // bilinear weights of full-resolution column X = 4 q + p (align_corners = False, scale 1/4)
                const int X = 4 * q + p;
                float sX = 0.25f * ((float)X + 0.5f) - 0.5f;
                sX = sX < 0.f ? 0.f : sX;
                const int x0 = min((int)sX, w - 1), x1 = x0 + (x0 < w - 1 ? 1 : 0);
                const float l1 = sX - (float)x0, l0 = 1.f - l1;
                // columns x0 / x1 are q - 1, q or q + 1
                const float wl = (x0 == q - 1 ? l0 : 0.f) + (x1 == q - 1 ? l1 : 0.f);
                const float wc = (x0 == q ? l0 : 0.f) + (x1 == q ? l1 : 0.f);
                const float wr = (x0 == q + 1 ? l0 : 0.f) + (x1 == q + 1 ? l1 : 0.f);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float dfc = -2.f * (gs * f[c] - gm[c]);
                    pl[c] += wl * dfc;
                    pc[c] += wc * dfc;
                    pr[c] += wr * dfc;
                }
            }
        }
        // three sub-phases: every (row, column) cell of this pass's rows is written by exactly one thread in each
#pragma unroll
        for (int c = 0; c < C; c += 4)
            *reinterpret_cast<float4*>(&t[r][g][c]) = make_float4(pc[c], pc[c + 1], pc[c + 2], pc[c + 3]);
        __syncthreads();
        if (g + 1 < HB_GRPS) {
#pragma unroll
            for (int c = 0; c < C; c += 4) {
                float4 v = *reinterpret_cast<float4*>(&t[r][g + 1][c]);
                v.x += pr[c]; v.y += pr[c + 1]; v.z += pr[c + 2]; v.w += pr[c + 3];
                *reinterpret_cast<float4*>(&t[r][g + 1][c]) = v;
            }
        }
        __syncthreads();
        if (g >= 1) {
#pragma unroll
            for (int c = 0; c < C; c += 4) {
                float4 v = *reinterpret_cast<float4*>(&t[r][g - 1][c]);
                v.x += pl[c]; v.y += pl[c + 1]; v.z += pl[c + 2]; v.w += pl[c + 3];
                *reinterpret_cast<float4*>(&t[r][g - 1][c]) = v;
            }
        }
    }
    __syncthreads();

    // phase 2: low-resolution pixel (j, i) x 8 channels per thread (98 pixels x 2 halves = 196 threads)
    const int px = tid >> 1, half = tid & 1;
    if (px >= HB_TJ * HB_TI) return;
    const int jj = px / HB_TI, ii = px - jj * HB_TI;
    const int j = j0 + jj, i = i0 + ii;
    if (j >= h || i >= w) return;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    for (int dy = 0; dy < 8; ++dy) {
        const int Y = 4 * j - 2 + dy;
        if (Y < 0 || Y >= H) continue;
        float sY = 0.25f * ((float)Y + 0.5f) - 0.5f;
        sY = sY < 0.f ? 0.f : sY;
        const int y0 = min((int)sY, h - 1), y1 = y0 + (y0 < h - 1 ? 1 : 0);
        const float l1 = sY - (float)y0;
        const float wy = (y0 == j ? 1.f - l1 : 0.f) + (y1 == j ? l1 : 0.f);
        if (wy == 0.f) continue;
        const float* src = &t[Y - Y0][ii + 1][half * 8];
        const float4 a = *reinterpret_cast<const float4*>(src), c4 = *reinterpret_cast<const float4*>(src + 4);
        acc[0] += wy * a.x; acc[1] += wy * a.y; acc[2] += wy * a.z; acc[3] += wy * a.w;
        acc[4] += wy * c4.x; acc[5] += wy * c4.y; acc[6] += wy * c4.z; acc[7] += wy * c4.w;
    }
    TO* dst = de + (((int64_t)b * h + j) * w + i) * C + half * 8;
    if constexpr (sizeof(TO) == 2) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]),
                                                    pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7]));
    } else {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

}  // namespace

extern "C" int dml_proto_dist_fwd(const float* x_nchw, const float* protos, float* logits, float* feats,
                                  uint8_t* argmax, float* dissum, int B, int C, int K, int H, int W,
                                  void* stream) {
    if (!x_nchw || !protos || B <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if (C <= 0 || C > MAXC || K <= 0 || K > MAXK) return DML_EUNSUPPORTED;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (HW % 4 == 0 && C == 16 && K == 16) {
        const int64_t groups = (int64_t)B * HW / 4;
        constexpr bool nt = DIST_NT_DEFAULT;
        if (nt)
            hipLaunchKernelGGL(proto_dist_fwd_c16_kernel<true>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                               x_nchw, protos, logits, feats, argmax, dissum, B, HW);
        else
            hipLaunchKernelGGL(proto_dist_fwd_c16_kernel<false>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                               x_nchw, protos, logits, feats, argmax, dissum, B, HW);
    } else if (HW % 4 == 0) {
        const int grid = grid_for((int64_t)B * HW / 4, 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((proto_dist_fwd_kernel<4, 16>), dim3(grid), dim3(256), 0, st, x_nchw, protos, logits, feats,
                           argmax, dissum, B, C, K, HW);
        else hipLaunchKernelGGL((proto_dist_fwd_kernel<4, 32>), dim3(grid), dim3(256), 0, st, x_nchw, protos, logits, feats,
                           argmax, dissum, B, C, K, HW);
    } else {
        const int grid = grid_for((int64_t)B * HW, 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((proto_dist_fwd_kernel<1, 16>), dim3(grid), dim3(256), 0, st, x_nchw, protos, logits, feats,
                           argmax, dissum, B, C, K, HW);
        else hipLaunchKernelGGL((proto_dist_fwd_kernel<1, 32>), dim3(grid), dim3(256), 0, st, x_nchw, protos, logits, feats,
                           argmax, dissum, B, C, K, HW);
    }
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_upsample_dist_fwd(const float* e, const float* protos, float* logits, float* feats,
                                     uint8_t* argmax, float* dissum, int B, int h, int w, int C, int K, int H,
                                     int W, void* stream) {
    if (!e || !protos || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if (C <= 0 || C > MAXC || K <= 0 || K > MAXK) return DML_EUNSUPPORTED;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr bool staged = true;      // (the gathered variant it replaced: profiles/r02_dist_variants.txt)
    if (staged && H == 4 * h && W == 4 * w && C == 16 && K == 16 && argmax == nullptr && dissum == nullptr) {
        constexpr bool nt4 = DIST_NT_DEFAULT;
        const int64_t blocks = (int64_t)B * (h + 1) * ((W + 255) / 256);
        if (blocks >= (1ll << 31)) return DML_EINVAL;
        if (nt4)
            hipLaunchKernelGGL(upsample4_dist_fwd_c16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, e, protos, logits,
                               feats, B, h, w);
        else
            hipLaunchKernelGGL(upsample4_dist_fwd_c16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, e, protos, logits,
                               feats, B, h, w);
    } else if (W % 4 == 0 && C == 16 && K == 16 && argmax == nullptr && dissum == nullptr) {
        const int64_t groups = (int64_t)B * H * (W / 4);
        constexpr bool nt = DIST_NT_DEFAULT;
        if (nt)
            hipLaunchKernelGGL(upsample_dist_fwd_c16_kernel<true>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, e,
                               protos, logits, feats, B, h, w, H, W, sy, sx);
        else
            hipLaunchKernelGGL(upsample_dist_fwd_c16_kernel<false>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, e,
                               protos, logits, feats, B, h, w, H, W, sy, sx);
    } else if (W % 4 == 0) {
        const int grid = grid_for((int64_t)B * H * (W / 4), 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((upsample_dist_fwd_kernel<4, 16>), dim3(grid), dim3(256), 0, st, e, protos, logits, feats,
                           argmax, dissum, B, h, w, C, K, H, W, sy, sx);
        else hipLaunchKernelGGL((upsample_dist_fwd_kernel<4, 32>), dim3(grid), dim3(256), 0, st, e, protos, logits, feats,
                           argmax, dissum, B, h, w, C, K, H, W, sy, sx);
    } else {
        const int grid = grid_for((int64_t)B * H * W, 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((upsample_dist_fwd_kernel<1, 16>), dim3(grid), dim3(256), 0, st, e, protos, logits, feats,
                           argmax, dissum, B, h, w, C, K, H, W, sy, sx);
        else hipLaunchKernelGGL((upsample_dist_fwd_kernel<1, 32>), dim3(grid), dim3(256), 0, st, e, protos, logits, feats,
                           argmax, dissum, B, h, w, C, K, H, W, sy, sx);
    }
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_incremental_predict(const DmlPredictHead* heads, int n, int64_t* preds, uint8_t* head_argmax,
                                       int B, int h, int w, int H, int W, void* stream) {
    if (!heads || !preds || n < 1 || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if (n > DML_PREDICT_MAX_HEADS) return DML_EUNSUPPORTED;
    PredictArgs args = {};
    args.n = n;
    for (int i = 0; i < n; ++i) {
        const DmlPredictHead& hd = heads[i];
        if (!hd.e || hd.C <= 0 || hd.K <= 0 || hd.ld < hd.C) return DML_EINVAL;
        if (hd.C > MAXC || hd.K > MAXK || hd.K > hd.C + 1) return DML_EUNSUPPORTED;
        args.head[i] = hd;
        if ((hd.C & 3) == 0 && (hd.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(hd.e) & 15) == 0) args.vec |= 1u << i;
    }
    if ((reinterpret_cast<uintptr_t>(preds) & 7) != 0) return DML_EALIGN;
    const int off = (int)((reinterpret_cast<uintptr_t>(preds) >> 3) & 1);
    const int64_t pairs = ((int64_t)B * H * W + off + 1) / 2;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipLaunchKernelGGL(incremental_predict_kernel, dim3(grid_for(pairs, 256, 256 * 16)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), args, preds, head_argmax, B, h, w, H, W, sy, sx, off);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_proto_dist_bwd(const float* glogits, const float* gfeats, const float* feats,
                                  const float* protos, float* df, int B, int C, int K, int H, int W,
                                  void* stream) {
    if (!glogits || !feats || !protos || !df || B <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if (C <= 0 || C > MAXC || K <= 0 || K > MAXK) return DML_EUNSUPPORTED;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (HW % 4 == 0 && C == 16 && K == 16) {
        const int64_t groups = (int64_t)B * HW / 4;
        hipLaunchKernelGGL(proto_dist_bwd_c16_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, glogits,
                           gfeats, feats, protos, df, B, HW);
    } else if (HW % 4 == 0) {
        const int grid = grid_for((int64_t)B * HW / 4, 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((proto_dist_bwd_kernel<4, 16>), dim3(grid), dim3(256), 0, st, glogits, gfeats, feats, protos,
                           df, B, C, K, HW);
        else hipLaunchKernelGGL((proto_dist_bwd_kernel<4, 32>), dim3(grid), dim3(256), 0, st, glogits, gfeats, feats, protos,
                           df, B, C, K, HW);
    } else {
        const int grid = grid_for((int64_t)B * HW, 256, 256 * 16);
        if (C <= 16) hipLaunchKernelGGL((proto_dist_bwd_kernel<1, 16>), dim3(grid), dim3(256), 0, st, glogits, gfeats, feats, protos,
                           df, B, C, K, HW);
        else hipLaunchKernelGGL((proto_dist_bwd_kernel<1, 32>), dim3(grid), dim3(256), 0, st, glogits, gfeats, feats, protos,
                           df, B, C, K, HW);
    }
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_head_bwd_fused(const float* feats, const int64_t* labels, const double* sums, const float* gout,
                                  const float* protos, void* de, int B, int h, int w, int C, int K, int H, int W,
                                  int64_t ignore_index, float alpha, float n_images, int dtype, void* stream) {
    if (!feats || !labels || !sums || !protos || !de || B <= 0 || h <= 0 || w <= 0) return DML_EINVAL;
    if (dtype != DML_F32 && dtype != DML_BF16) return DML_EINVAL;
    if (C != 16 || K != 16 || H != 4 * h || W != 4 * w) return DML_EUNSUPPORTED;
    const int tiles = ((w + HB_TI - 1) / HB_TI) * ((h + HB_TJ - 1) / HB_TJ);
    if ((int64_t)tiles * B >= (1ll << 31)) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DML_BF16)
        hipLaunchKernelGGL(head_bwd_fused_c16_kernel<bf16_t>, dim3(tiles * B), dim3(256), 0, st, feats, labels, sums, gout,
                           protos, static_cast<bf16_t*>(de), B, h, w, ignore_index, alpha, n_images);
    else
        hipLaunchKernelGGL(head_bwd_fused_c16_kernel<float>, dim3(tiles * B), dim3(256), 0, st, feats, labels, sums, gout,
                           protos, static_cast<float*>(de), B, h, w, ignore_index, alpha, n_images);
    DML_LAUNCH_CHECK();
    return 0;
}

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

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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
    const bool vec = HW % 4 == 0 && aligned16(logits) && aligned16(preds) && aligned16(msp) && aligned16(score);
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
    if (K - k_first > MIX_MAXK || B > 65535) return DML_EUNSUPPORTED;
    // the image index is the grid's y; 2^40 pixels keep every offset into the maps inside int64
    if ((int64_t)H * W > (1ll << 40) / B) return DML_EUNSUPPORTED;
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* smap = work + 4 * (int64_t)B;
    float* mmap = smap + (int64_t)B * HW;
    // with H W % 4 == 0 every plane, every image of the maps and the first class's plane keep the base pointer's alignment
    const bool vec_maps = HW % 4 == 0 && aligned16(work);
    const bool vec1 = vec_maps && aligned16(logits), vec2 = vec_maps && aligned16(conf);
    const bool reg = K - k_first <= MIX_KREG;
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

#define DML_LOSS_BLOCKS 2048

extern "C" int dml_loss_fwd(const float* logits, const int64_t* labels, double* sums, float* block_partials,
                            int B, int K, int H, int W, int64_t ignore_index, void* stream) {
    if (!logits || !labels || !sums || !block_partials || B <= 0 || K <= 0) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const bool v4 = (HW % 4) == 0;
    const int grid = grid_for(B * HW / (v4 ? 4 : 1), 256, DML_LOSS_BLOCKS);
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

// ------------------------------------------------------------------------------------------------
// confusion matrix (metrics/stream_metrics.py:49-55 of the reference): per-workgroup LDS histogram, int64 flush
// ------------------------------------------------------------------------------------------------
namespace {
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
}  // namespace

extern "C" int dml_confusion_update(const int64_t* label_true, const int64_t* label_pred, int64_t* hist, int64_t count,
                                    int n_classes, void* stream) {
    if (!label_true || !label_pred || !hist || count < 0 || n_classes <= 0 || n_classes > 64) return DML_EINVAL;
    if ((reinterpret_cast<uintptr_t>(label_true) | reinterpret_cast<uintptr_t>(label_pred)) & 15) return DML_EALIGN;
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

// ------------------------------------------------------------------------------------------------
// masked feature sum for the few-shot prototypes (test_embedding.py:413-425 of the reference)
// ------------------------------------------------------------------------------------------------
namespace {
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
}  // namespace

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

// ------------------------------------------------------------------------------------------------
// the same for up to MAXM classes in one read of the features and labels (the shots of the 16+2 / 16+3 settings).
// QUADS lanes share a pixel, each owns 4 channels (one 16-byte load when C % 4 == 0), so a thread carries MAXM x 4 fp32
// partial sums instead of MAXM x C.  Accumulation as above: fp32 within a thread, double across threads.
// ------------------------------------------------------------------------------------------------
namespace {
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
    const bool vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(feats) & 15) == 0;
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
