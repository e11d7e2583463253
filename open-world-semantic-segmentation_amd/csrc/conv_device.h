// What the convolution translation units share: conv_igemm.hip (host side, tile and weight-gradient kernels) and conv_ws.hip with
// conv_ws_dgrad.hip (the wave-specialised kernel of conv_ws.h).  Here are the kernel arguments, the tile constants, the device
// helpers that more than one kernel family uses -- the shared epilogue among them -- and the launchers through which the host side
// reaches the kernels of another translation unit.  Internal to the library: no other source includes it.
#pragma once
#include "common.h"
#include "conv_choice.h"

// conv_igemm.hip fills the kernel arguments and a launcher in another translation unit passes them to the kernel, so they are the
// same type everywhere: a named namespace, where the kernels and the device helpers keep to anonymous ones.
namespace conv_device {

struct ConvArgs {
    const void* x;
    const void* w;
    void* y;
    const float* bias;
    float* stats;
    int B, Hi, Wi, C, ldx;
    int Ho, Wo, N, ldy;
    int R, S, stride, dil, pad;
    int M, Ktot;
    int y_f32, accum;
    int nblk_n, nblk_m;
    FastDiv div_wo, div_howo, div_c;
    float* unused0_;             // unused0_ / unused1_: unused, they keep the layout and with it the kernels' code as it was
    uint32_t x_bytes, w_bytes;   // operand extents for the buffer descriptors (fast path: both < 2^31)
    int w_tiled;                 // weights in the tile-major layout (DmlConvDesc::w_tiled): LDS-DMA kernels only
    int ws_min_tiles;            // DmlConvDesc::ws_min_tiles: host side only and read by no code (conv_choice.h looks at the descriptor)
    // f32_split == 2: operands as two fp16 planes of the power-of-two-scaled fp32 tensors (DmlConvDesc::x_planes ...)
    const void* x_planes;
    const void* w_planes;
    const float* x_unscale;      // device scalars: 1 / scale of the operand (dml_h2_split)
    const float* w_unscale;
    uint32_t x_plane_bytes, w_plane_bytes;      // distance from the hi plane to the lo plane
    // data-gradient mode: BN-backward partial sums of the tensor being written (DmlConvDesc::bnr_*)
    const void* bnr_y;
    const uint8_t* bnr_mask;
    const float* bnr_mean;
    const float* bnr_invstd;
    float* bnr_partials;
    float* bnr_gmax;
    int bnr_ldy, bnr_relu;
    // forward mode: inference epilogue (DmlConvDesc::post_*)
    const float* post_scale;
    const float* post_shift;
    const float* post_mean;
    const void* post_res;
    int post_ldres, post_relu;
    // K-split of the remainder tiles (DmlConvDesc::tail_*): tiles >= tail_full are computed by tail_q workgroups each
    float* tail_ws;
    int* tail_cnt;
    int tail_full, tail_q;
    int64_t tail_ws_elems_;      // host side only and read by no code: capacities of the two buffers (conv_choice.h looks at the
    int tail_cnt_len_;           // descriptor)
    // data-gradient mode: masked residual gradient added in the epilogue (DmlConvDesc::res_*)
    const void* res_dz;
    const uint8_t* res_mask;
    int res_ld;
    // data-gradient mode: fp32 sum of the earlier producers of this gradient, added before the one rounding (DmlConvDesc::acc32)
    const float* acc32;
    int acc32_ld;
    int f32_split;      // fp32 tensors: products through the three-term bf16 split (DmlConvDesc::f32_split)
    // bit 0: the epilogue's bf16 output stores carry the non-temporal hint, bit 1: its partial-statistics stores (conv_choice.h)
    int nt_out;
    int unused1_;
    // one parity class of a stride-2 data gradient as a stride-1 launch on dY's grid (DmlConvDesc::sub_grid): the launch's rows are
    // the pixels (b, 2 y2 + sub_y, 2 x2 + sub_x) of the B x 2 Ho x 2 Wo tensors y / res_dz / bnr_y / masks (ws_out_row)
    int pad_x;             // padding along the width (== pad unless DmlConvDesc::pad_w_set)
    int sub_grid, sub_y, sub_x;
    int bnr_inc;           // fused BN-backward sums over the launch's increment, not the stored total (DmlConvDesc::bnr_inc)
};

// The launchers of conv_ws.hip (ConvChoice::family == CONV_WS) and of conv_ws_dgrad.hip, to which the former hands the two-plane
// data gradients: each maps the choice to the template instantiation it names and launches it.  Hidden: the library exports its C
// entry points only.
__attribute__((visibility("hidden"))) void launch_conv_ws(const conv_choice::ConvChoice& c, const ConvArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) void launch_conv_ws_dgrad_planes(const conv_choice::ConvChoice& c, const ConvArgs& a, hipStream_t st);

}  // namespace conv_device

namespace {

using namespace conv_device;
namespace cc = conv_choice;

constexpr int BK = 32;
constexpr int NTHREADS = 256;
// wave-specialised forward / data-gradient kernel (conv_ws.h)
constexpr int WS_MT = 9;                       // 16-row fragments per wave tile (144 rows)
constexpr int WS_STAT_ROWS = 48;               // rows per statistics group of this kernel
constexpr int WS_NST = 6, WS_D = 2;            // ring stages; stages in flight per loader behind the published one
constexpr int WS_PLANES_NLD = 3;               // loader waves of the two-plane instantiation

typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 mfma_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_ws __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// physical pixel row of row m of the launch in the epilogue's tensors (y, accumulate / identity operand, bnr_y, masks); a row beyond
// M maps to the first row beyond those tensors (buffer accesses with the tensor's size as range drop it / read zeros, pointer
// accesses are guarded by their callers)
__device__ __forceinline__ uint32_t ws_out_row(const ConvArgs& a, const uint32_t m) {
    if (!a.sub_grid) return m;
    if (m >= (uint32_t)a.M) return 4u * (uint32_t)a.M;
    const uint32_t b = fdiv(m, a.div_howo);
    const uint32_t rem = m - b * (uint32_t)(a.Ho * a.Wo);
    const uint32_t y2 = fdiv(rem, a.div_wo);
    const uint32_t x2 = rem - y2 * (uint32_t)a.Wo;
    return ((b * 2u * (uint32_t)a.Ho + 2u * y2 + (uint32_t)a.sub_y) * 2u * (uint32_t)a.Wo) + 2u * x2 + (uint32_t)a.sub_x;
}
// rows of those tensors (range of the epilogue's buffer descriptors)
__device__ __forceinline__ uint32_t ws_out_rows(const ConvArgs& a) { return a.sub_grid ? 4u * (uint32_t)a.M : (uint32_t)a.M; }

constexpr int WGRAD_DEPTH = 2;      // K steps per barrier of the 256 x 256 weight-gradient kernel (one: 3-12 % slower)

// bijective XCD-aware remap: consecutive logical tiles land on the same XCD (private L2)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

template <typename T> __device__ __forceinline__ int swz_chunk(int row, int chunk);
// bf16: 64-byte rows, ds_read_b128 lane groups {0-3,12-15,20-27}... -> conflict-free permutation
template <> __device__ __forceinline__ int swz_chunk<bf16_t>(int row, int chunk) {
    return chunk ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3);
}
// fp32: 128-byte rows, 8 chunks of 16 B
template <> __device__ __forceinline__ int swz_chunk<float>(int row, int chunk) { return chunk ^ (row & 7); }

// ------------------------------------------------------------------------------------------------
// Weight-tile row order.  MFMA tile i of a wave's TN = 16 NT channels does not take channels 16 i .. 16 i + 15:
// its row rho = 4 g + e (g = rho >> 2 is the accumulator's lane group, e the register) is channel
// g * (4 NT) + 4 i + e, so that after NT tiles every lane holds CL = 4 NT CONSECUTIVE channels of one pixel and the
// epilogue stores whole 16-byte vectors straight from the accumulators (a wave writes full 128-byte rows; no
// LDS staging, no barriers).  In LDS the tile stays in plain channel order; the fragment read just picks row
// b_row(i, rho), and the chunk swizzle is keyed on rho (recovered from the row by b_rho) so the bank pattern of
// the fragment reads is the conflict-free one of swz_chunk.
// ------------------------------------------------------------------------------------------------
// NT = 4 (wave tile 64 channels): the lane's 16 channels are two runs of 8, 32 apart -- tiles 2p, 2p+1 of lane group g are
// channels 32 p + 8 g .. 32 p + 8 g + 7 -- so that ONE store instruction (8 channels = 16 bytes per lane) writes 64
// contiguous bytes per pixel row (the four lane groups side by side) instead of four 16-byte pieces 32 bytes apart.
// (Throughput-neutral -- the L2 merges either pattern, and the store-heavy 1x1 layers sit at the ~2.7 TB/s the chip
// sustains for writes: 64 -> 256 channels at 192 x 192 writes 302 MB in 111 us -- but the epilogue needs 20-30 fewer
// VGPRs with it.)
template <int NT> __device__ __forceinline__ int frag_chan(int i, int g) {      // first channel of tile i in lane group g
    return NT == 4 ? (i >> 1) * 32 + g * 8 + (i & 1) * 4 : g * (4 * NT) + i * 4;
}
template <int NT> __device__ __forceinline__ int b_row(int i, int rho) { return frag_chan<NT>(i, rho >> 2) + (rho & 3); }
template <int NT> __device__ __forceinline__ int b_rho(int row) {
    return NT == 4 ? ((row >> 3) & 3) * 4 + (row & 3) : ((row / (4 * NT)) & 3) * 4 + (row & 3);
}

template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 16 lanes of a DPP row (every lane gets the total): quad xor 1, xor 2, half mirror, row mirror
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}

// 16-byte store, optionally with the non-temporal hint.  Why the hint: a conv output of 75-300 MB passes through 32 MB of
// L2; with plain stores the lines stay dirty until capacity evicts them, the evictions stall the allocating stores, the
// stalled stores block the CU's memory pipeline and the operand loads of the other workgroups queue behind them -- the
// store time ADDS to the compute time instead of hiding under it (1x1 256 -> 1024 at 48 x 48: 53 us, 30 us without the
// stores, 36 us with the stores aimed at an L2-resident region).  Non-temporal stores stream to memory: 36.4 us.
typedef unsigned int u32x4_st __attribute__((ext_vector_type(4)));
typedef float f32x4_st __attribute__((ext_vector_type(4)));
// (inline asm: with __builtin_nontemporal_store in one arm of a run-time branch the optimiser merges the two stores to the
// same address into one plain store and the hint is gone)
__device__ __forceinline__ void st16(void* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d, const bool nt) {
    const u32x4_st v = {a, b, c, d};
    if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
    else *reinterpret_cast<u32x4_st*>(p) = v;
}
__device__ __forceinline__ void st16f(float* p, float a, float b, float c, float d, const bool nt) {
    const f32x4_st v = {a, b, c, d};
    if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
    else *reinterpret_cast<f32x4_st*>(p) = v;
}

// ------------------------------------------------------------------------------------------------
// shared epilogue: BN partial statistics, bias, accumulate, fp32 / storage-dtype stores
// acc[i][j][e] = out[m = mw0 + j*16 + (lane&15)][n = nw0 + frag_chan<NT>(i, lane>>4) + e]
// ------------------------------------------------------------------------------------------------
template <typename T, int NT, int MT, int MODE, bool WIDE_MASK = true, bool STATS_ONLY = false>
__device__ __forceinline__ void conv_epilogue(f32x4 (&acc)[NT][MT], const ConvArgs& a, const int mw0, const int nw0,
                                              const int lr, const int lq) {
    constexpr int TM = MT * 16;
    constexpr int CL = NT * 4;
    auto ch = [&](int c) { return nw0 + frag_chan<NT>(c >> 2, lq) + (c & 3); };      // channel of the lane's c-th value

    if (a.stats != nullptr) {
        const int cnt = min(TM, max(0, a.M - mw0));
        if (cnt > 0) {
            const float inv = 1.0f / (float)cnt;
            const int grp = mw0 / TM;
            float* sg = a.stats + (int64_t)grp * a.N * 2;
            const bool pair_ok = (a.N & 1) == 0;
            // whole wave tile inside N: the partials leave in ONE store instruction -- lane (lq, lr = 2 i + h) writes the
            // (sum, M2) pairs of channels 2h, 2h+1 of tile i, 32 lanes x 16 B covering the wave's 64 channels contiguously --
            // instead of two 64-byte stores from four lanes per tile (8 instructions per wave: at ~1 us per 128 x 128 tile
            // the statistics cost 13-34 us per launch on the large maps)
            const bool gather = pair_ok && nw0 + NT * 16 <= a.N;
            float S[NT][4], Q[NT][4];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const bool v = (mw0 + j * 16 + lr) < a.M;
#pragma unroll
                    for (int q = 0; q < 4; ++q) s[q] += v ? acc[i][j][q] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = row16_sum(s[q]);
                float m2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const bool v = (mw0 + j * 16 + lr) < a.M;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float dlt = acc[i][j][q] - s[q] * inv;
                        m2[q] += v ? dlt * dlt : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) m2[q] = row16_sum(m2[q]);
#pragma unroll
                for (int q = 0; q < 4; ++q) { S[i][q] = s[q]; Q[i][q] = m2[q]; }
                if (lr == 0 && !gather) {
                    const int n = ch(i * 4);
                    float* sp = sg + (int64_t)n * 2 - i * 8;
                    if (pair_ok && n + 3 < a.N) {
                        st16f(sp + i * 8, s[0], m2[0], s[1], m2[1], (a.nt_out & 2) != 0);
                        st16f(sp + i * 8 + 4, s[2], m2[2], s[3], m2[3], (a.nt_out & 2) != 0);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (n + q < a.N) {
                                sp[(i * 4 + q) * 2] = s[q];
                                sp[(i * 4 + q) * 2 + 1] = m2[q];
                            }
                    }
                }
            }
            if (gather && lr < 2 * NT) {
                float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (lr == 2 * i + h) { v0 = S[i][2 * h]; v1 = Q[i][2 * h]; v2 = S[i][2 * h + 1]; v3 = Q[i][2 * h + 1]; }
                const int n = nw0 + frag_chan<NT>(lr >> 1, lq) + (lr & 1) * 2;
                st16f(sg + (int64_t)n * 2, v0, v1, v2, v3, (a.nt_out & 2) != 0);
            }
        }
    }

    if constexpr (STATS_ONLY) return;      // (the caller stores the tile itself: conv_epilogue_rows)

    float bv[CL];
#pragma unroll
    for (int c = 0; c < CL; ++c) bv[c] = (MODE == 0 && a.bias != nullptr && ch(c) < a.N) ? a.bias[ch(c)] : 0.f;

    const bool out_f32 = a.y_f32 || sizeof(T) == 4;
    const uintptr_t yb = reinterpret_cast<uintptr_t>(a.y);
    const bool v4_ok = ((a.N & 3) == 0) && ((a.ldy & 3) == 0) && ((yb & (out_f32 ? 15 : 7)) == 0);
    const bool v8_ok = ((a.N & 7) == 0) && ((a.ldy & 7) == 0) && ((yb & 15) == 0);

    if constexpr (sizeof(T) == 2 && CL >= 8) {
        if (!out_f32 && v8_ok) {
            // bf16 rows of 16-byte vectors: 8-channel group outer, rows inner, so that the optional BN-backward sums
            // of the group (below) live in 32 registers.
            // Data gradient whose result is the output gradient dz of a BatchNorm(+ReLU): emit that BN's backward
            // partial sums (sum g, sum g * xhat per 64 rows, g = dz * relu') from the bf16-rounded values being
            // stored -- exactly what dml_bn_bwd_reduce would compute from the stored tensor -- so the separate pass
            // over dz / y / mask disappears.
            const bool bnr = MODE == 1 && a.bnr_partials != nullptr;
            const bool resm = MODE == 1 && a.res_dz != nullptr;
            constexpr bool a32 = MODE == 2;      // its own instantiation: the hot MODE 1 kernels keep their register budget
            const bool post = MODE == 0 && a.post_scale != nullptr;
            // ReLU-mask bits of the wave's whole 64 x 64 tile in ONE instruction per mask: lane L fetches row L's 64 bits (8
            // bytes), and lane (lr, lq) later takes byte 4 g + lq of row 16 j + lr through a lane permute -- instead of one
            // byte-load instruction per (j, g), each of which costs the texture addresser as much as a 1 KB load
            // (profiles/r03_epi_pmc.txt).  Wave tiles of 64 channels inside N only; the others load bytes.
            // (WIDE_MASK = false: the 256-row tile's kernel, at its 256-register limit, keeps the byte loads)
            const bool wide_mask = WIDE_MASK && MODE == 1 && NT == 4 && MT == 4 && (a.N & 63) == 0 && nw0 + 64 <= a.N;
            uint32_t rm_lo = 0xffffffffu, rm_hi = 0xffffffffu, bm_lo = 0xffffffffu, bm_hi = 0xffffffffu;
            if (MODE == 1 && wide_mask) {
                const int mrow = mw0 + lq * 16 + lr;              // lane L = lq * 16 + lr holds row L of the tile
                if (mrow < a.M) {
                    const int64_t mo = (int64_t)mrow * (a.N >> 3) + (nw0 >> 3);
                    if (resm) {
                        const uint2 v = *reinterpret_cast<const uint2*>(a.res_mask + mo);
                        rm_lo = v.x; rm_hi = v.y;
                    }
                    if (bnr && a.bnr_relu) {
                        const uint2 v = *reinterpret_cast<const uint2*>(a.bnr_mask + mo);
                        bm_lo = v.x; bm_hi = v.y;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < CL / 8; ++g) {
                const int n8 = ch(g * 8);
                if (n8 >= a.N) continue;
                float r1[8], r2[8], rmu[8], ris[8];      // MODE 1: BN-backward sums; MODE 0: inference BN coefficients
                if (post) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        r1[e] = a.post_scale[n8 + e];
                        r2[e] = a.post_shift[n8 + e];
                        rmu[e] = a.post_mean[n8 + e];
                    }
                }
                if (bnr) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        r1[e] = 0.f;
                        r2[e] = 0.f;
                        rmu[e] = a.bnr_mean[n8 + e];
                        ris[e] = a.bnr_invstd[n8 + e];
                    }
                }
                // all of the group's loads (accumulate operand, BN input, mask bytes) are issued before the first
                // use: one memory round trip per group instead of one per row
                uint4 told[MT], ty[MT];      // (acc32: the row's eight floats, in told and ty -- never together with bnr)
                uint32_t bits[MT], rbits[MT];
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const int m = mw0 + j * 16 + lr;
                    told[j] = make_uint4(0, 0, 0, 0);
                    ty[j] = make_uint4(0, 0, 0, 0);
                    bits[j] = 0xffu;
                    rbits[j] = 0xffu;
                    if (m < a.M) {
                        if (resm) {
                            told[j] = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(a.res_dz) +
                                                                      (int64_t)m * a.res_ld + n8);
                            if (!wide_mask) rbits[j] = a.res_mask[(int64_t)m * (a.N >> 3) + (n8 >> 3)];
                        }
                        if (post && a.post_res != nullptr)
                            told[j] = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(a.post_res) +
                                                                      (int64_t)m * a.post_ldres + n8);
                        else if (a32) {
                            // (32-bit element offset from the uniform base: the staging tensors stay below 2^32 bytes)
                            const uint32_t ao = (uint32_t)m * (uint32_t)a.acc32_ld + (uint32_t)n8;
                            told[j] = *reinterpret_cast<const uint4*>(a.acc32 + ao);
                            ty[j] = *reinterpret_cast<const uint4*>(a.acc32 + ao + 4);
                        } else if (a.accum)
                            told[j] = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(a.y) + (int64_t)m * a.ldy + n8);
                        if (bnr) {
                            ty[j] = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(a.bnr_y) +
                                                                    (int64_t)m * a.bnr_ldy + n8);
                            if (a.bnr_relu && !wide_mask) bits[j] = a.bnr_mask[(int64_t)m * (a.N >> 3) + (n8 >> 3)];
                        }
                    }
                }
                if (MODE == 1 && wide_mask) {
                    // (executed by every lane: the permute reads another lane's register)
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
                        const int src = j * 16 + lr;
                        if (resm) rbits[j] = ((uint32_t)__shfl((int)(g == 0 ? rm_lo : rm_hi), src) >> (lq * 8)) & 0xffu;
                        if (bnr && a.bnr_relu) bits[j] = ((uint32_t)__shfl((int)(g == 0 ? bm_lo : bm_hi), src) >> (lq * 8)) & 0xffu;
                    }
                }
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const int m = mw0 + j * 16 + lr;
                    if (m >= a.M) continue;
                    float w[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = acc[(g * 8 + e) >> 2][j][e & 3] + bv[g * 8 + e];
                    if (post) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) w[e] = (w[e] - rmu[e]) * r1[e] + r2[e];
                    }
                    bf16_t* yp = static_cast<bf16_t*>(a.y) + (int64_t)m * a.ldy + n8;
                    if (a32) {             // fp32 running sum of the earlier producers: this launch rounds the total once
                        w[0] += __uint_as_float(told[j].x); w[1] += __uint_as_float(told[j].y);
                        w[2] += __uint_as_float(told[j].z); w[3] += __uint_as_float(told[j].w);
                        w[4] += __uint_as_float(ty[j].x); w[5] += __uint_as_float(ty[j].y);
                        w[6] += __uint_as_float(ty[j].z); w[7] += __uint_as_float(ty[j].w);
                    } else {
                        const uint32_t tt[4] = {told[j].x, told[j].y, told[j].z, told[j].w};      // zeros unless accumulating
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (resm) {          // masked residual gradient: a cleared ReLU bit drops the element
                                w[2 * e] += (rbits[j] >> (2 * e)) & 1u ? __uint_as_float(tt[e] << 16) : 0.f;
                                w[2 * e + 1] += (rbits[j] >> (2 * e + 1)) & 1u ? __uint_as_float(tt[e] & 0xffff0000u) : 0.f;
                            } else {
                                w[2 * e] += __uint_as_float(tt[e] << 16);
                                w[2 * e + 1] += __uint_as_float(tt[e] & 0xffff0000u);
                            }
                        }
                    }
                    if (post && a.post_relu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) w[e] = w[e] > 0.f ? w[e] : 0.f;
                    }
                    const uint32_t pk[4] = {pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3]), pack_bf16x2(w[4], w[5]),
                                            pack_bf16x2(w[6], w[7])};
                    st16(yp, pk[0], pk[1], pk[2], pk[3], (a.nt_out & 1) != 0);
                    if (bnr) {
                        const uint32_t yy[4] = {ty[j].x, ty[j].y, ty[j].z, ty[j].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float g0 = (bits[j] >> (2 * e)) & 1u ? __uint_as_float(pk[e] << 16) : 0.f;
                            const float g1 = (bits[j] >> (2 * e + 1)) & 1u ? __uint_as_float(pk[e] & 0xffff0000u) : 0.f;
                            r1[2 * e] += g0;
                            r2[2 * e] += g0 * (__uint_as_float(yy[e] << 16) - rmu[2 * e]) * ris[2 * e];
                            r1[2 * e + 1] += g1;
                            r2[2 * e + 1] += g1 * (__uint_as_float(yy[e] & 0xffff0000u) - rmu[2 * e + 1]) * ris[2 * e + 1];
                        }
                    }
                }
                if (bnr && mw0 < a.M) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        r1[e] = row16_sum(r1[e]);
                        r2[e] = row16_sum(r2[e]);
                    }
                    if (lr < 4) {            // lane lr writes the pairs of channels 2 lr, 2 lr + 1: one instruction per group
                        float* pp = a.bnr_partials + ((int64_t)(mw0 / TM) * a.N + n8) * 2;
                        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (lr == e) { v0 = r1[2 * e]; v1 = r2[2 * e]; v2 = r1[2 * e + 1]; v3 = r2[2 * e + 1]; }
                        st16f(pp + 4 * lr, v0, v1, v2, v3, (a.nt_out & 2) != 0);
                    }
                }
            }
            return;
        }
    }

#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int m = mw0 + j * 16 + lr;
        if (m >= a.M) continue;
        float v[CL];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[i * 4 + q] = acc[i][j][q] + bv[i * 4 + q];
        if (MODE == 0 && a.post_scale != nullptr) {          // inference epilogue on the generic path (fp32, odd shapes)
#pragma unroll
            for (int c = 0; c < CL; ++c) {
                if (ch(c) >= a.N) continue;
                float t = (v[c] - a.post_mean[ch(c)]) * a.post_scale[ch(c)] + a.post_shift[ch(c)];
                if (a.post_res != nullptr)
                    t += Elem<T>::ld(static_cast<const T*>(a.post_res) + (int64_t)m * a.post_ldres + ch(c));
                v[c] = a.post_relu ? (t > 0.f ? t : 0.f) : t;
            }
        }
        // yp + g * 4 below addresses the lane's g-th run of four channels: rebase per run through ch()
        const int64_t off = (int64_t)m * a.ldy;
        if (out_f32) {
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const int n = ch(g * 4);
                float* yp = static_cast<float*>(a.y) + off + n - g * 4;
                if (n >= a.N) continue;
                if (v4_ok) {
                    float4 o = make_float4(v[g * 4], v[g * 4 + 1], v[g * 4 + 2], v[g * 4 + 3]);
                    if (a.accum) {
                        const float4 t = *reinterpret_cast<const float4*>(yp + g * 4);
                        o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
                    }
                    *reinterpret_cast<float4*>(yp + g * 4) = o;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (n + q < a.N) yp[g * 4 + q] = a.accum ? yp[g * 4 + q] + v[g * 4 + q] : v[g * 4 + q];
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const int n = ch(g * 4);
                bf16_t* yp = static_cast<bf16_t*>(a.y) + off + n - g * 4;
                if (n >= a.N) continue;
                float* w = v + g * 4;
                if (v4_ok) {
                    if (a.accum) {
                        const uint2 t = *reinterpret_cast<const uint2*>(yp + g * 4);
                        w[0] += __uint_as_float(t.x << 16);
                        w[1] += __uint_as_float(t.x & 0xffff0000u);
                        w[2] += __uint_as_float(t.y << 16);
                        w[3] += __uint_as_float(t.y & 0xffff0000u);
                    }
                    *reinterpret_cast<uint2*>(yp + g * 4) = make_uint2(pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3]));
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (n + q < a.N) yp[g * 4 + q] = f32_to_bf16(a.accum ? bf16_to_f32(yp[g * 4 + q]) + w[q] : w[q]);
                }
            }
        }
    }
}

// LDS-DMA piece (16 B per lane, 1 KB per wave) from inline asm: m0 = LDS byte address of the piece (wave-uniform), voff per
// lane, soff scalar; offsets beyond the descriptor write zeros.  Not counted by hipcc: completion by wait_vmcnt only.
__device__ __forceinline__ void ws_dma16(const u32x4_ws rsrc, const uint32_t lds_addr, const uint32_t voff, const uint32_t soff) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff)
                 : "memory");
}
__device__ __forceinline__ u32x4_ws ws_make_rsrc(const void* base, const uint32_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    u32x4_ws r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane(bytes);
    r[3] = 0x00020000u;
    return r;
}
__device__ __forceinline__ uint32_t ws_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void ws_st(uint32_t* p, const uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

}  // namespace
