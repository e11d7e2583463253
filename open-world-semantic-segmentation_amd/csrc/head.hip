// Pixel -> prototype squared-Euclidean-distance head, its backward (alone and fused with the loss and the final upsample) and
// the merged prediction of the incremental heads, for gfx950.  All HBM-bound (about 4 flop/byte): one lane owns 4 consecutive
// pixels so that every global access is a 16-byte vector; prototypes sit in LDS and are read as broadcasts.
//
// Replaces network/utils.py:92-118 (the reference materialises a B x HW x K x C tensor twice).  The DML loss is dml_loss.hip, the
// open-world scores scores.hip, the confusion matrix and the class feature sums eval_sums.hip.
#include "common.h"

namespace {

// the blend of the four samples that a row tap and a column tap (common.h's src_tap) select
__device__ __forceinline__ float bilerp(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
    return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
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
        if (logits != nullptr) store_px<PX>(logits + img_base_logits + (int64_t)k * plane + pix_in_img, d);
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
            if (c < C) load_px<PX>(x + (b * C + c) * HW + pix, f[c]);
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
            load_px<PX>(glogits + (b * K + k) * HW + pix, g);
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
                // a pixel reaches two of the three columns (one where x1 == x0): the third's weight is zero and is skipped, not
                // multiplied -- 0 * NaN would carry a non-finite pixel into a column it does not interpolate into
                float dfc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    dfc[c] = -2.f * (gs * f[c] - gm[c]);
                    pc[c] += wc * dfc[c];
                }
                if (wl != 0.f) {
#pragma unroll
                    for (int c = 0; c < C; ++c) pl[c] += wl * dfc[c];
                }
                if (wr != 0.f) {
#pragma unroll
                    for (int c = 0; c < C; ++c) pr[c] += wr * dfc[c];
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
        if ((hd.C & 3) == 0 && (hd.ld & 3) == 0 && aligned16(hd.e)) args.vec |= 1u << i;
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
