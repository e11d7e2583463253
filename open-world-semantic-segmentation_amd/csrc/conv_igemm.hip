// Implicit-GEMM convolution on MFMA for gfx950 (MI355X).
//
//   forward : y[m][n]  = sum_{r,s,c} x[src(m,r,s)][c] * w[n][r][s][c]          m = (b,yo,xo)
//   dgrad   : dx[m][n] = sum_{r,s,c} dy[srcT(m,r,s)][c] * wt[n][r][s][c]       m = (b,yi,xi), n = Cin
//   wgrad   : dw[n][r][s][c] += sum_m dy[m][n] * x[src(m,r,s)][c]
//
// Replaces nn.Conv2d at network/backbone/resnet.py:24-32,139 and network/utils.py:11-23,311,322,
// 337-352 of the reference (cuDNN there).  Layout NHWC / KRSC so that the GEMM K dimension is
// contiguous in both operands; 128-row pixel tiles; bf16 (v_mfma_f32_16x16x32_bf16) or exact fp32
// (v_mfma_f32_16x16x4_f32) with fp32 accumulation.  The MFMA "row" operand is the weight tile, fed in a permuted
// row order, so that every lane ends up with 16 consecutive output channels of one pixel (16-byte stores).
// Epilogue options, all on the fp32 accumulators: per-channel BatchNorm partial statistics (training forward),
// BatchNorm + residual + ReLU (inference), bias, accumulate, and -- data gradient -- the BN-backward partial sums
// of the tensor being written.
//
// The wave-specialised kernel is conv_ws.h, instantiated in conv_ws.hip and conv_ws_dgrad.hip; conv_device.h holds what those share
// with this file.
#include "conv_device.h"
#include <cstdlib>

namespace {

// ------------------------------------------------------------------------------------------------
// forward / data-gradient kernel
// ------------------------------------------------------------------------------------------------
template <typename T, int BN, bool ALIGNED, int MODE>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(3))) void conv_igemm_kernel(const ConvArgs a) {
    constexpr int BM = 128;
    constexpr int VEC = Elem<T>::VEC;
    constexpr int KV = BK / VEC;                 // 16-byte chunks per tile row
    constexpr int RPP = NTHREADS / KV;           // rows staged per pass
    constexpr int A_LD = BM / RPP;
    constexpr int B_LD = (BN + RPP - 1) / RPP;
    constexpr int TM = 64, TN = BN / 2;          // wave tile (2 x 2 waves)
    constexpr int MT = TM / 16, NT = TN / 16;

    __shared__ __attribute__((aligned(256))) T smem[2 * (BM + BN) * BK];
    auto As = [&](int buf) -> T* { return smem + buf * (BM + BN) * BK; };
    auto Bs = [&](int buf) -> T* { return smem + buf * (BM + BN) * BK + BM * BK; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int blk_m = tile / a.nblk_n, blk_n = tile - blk_m * a.nblk_n;
    const int m0 = blk_m * BM, n0 = blk_n * BN;

    const T* __restrict__ X = static_cast<const T*>(a.x);
    const T* __restrict__ Wt = static_cast<const T*>(a.w);

    const int kvec = tid % KV, prow = tid / KV;
    constexpr int ES = (int)sizeof(T);
    constexpr uint32_t OOB = 0x80000000u;          // beyond any descriptor: the load returns zeros

    // ---- operand addressing.
    // ALIGNED (C % 32 == 0: a K tile never straddles a filter tap): everything per-thread is loop invariant -- a
    // signed byte offset of the row's tap-(0,0) pixel, a bit per filter tap saying whether that tap lands inside
    // the image (and, for the stride-2 data gradient, on an even position), and the weight row offset.  Per K step
    // the tap / channel advance is SCALAR; padding and tile edges are an out-of-range buffer offset, so the loads
    // are branch-free: 3 VALU per activation load, none per weight load.
    // Otherwise (stem 7x7 with 8 channels, odd channel counts, > 32 taps, > 2 GiB tensors): generic 64-bit gather.
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, (int)a.w_bytes, 0x00020000);
    const int sh2 = (MODE != 0 && a.stride == 2) ? 1 : 0;

    int a_iy[A_LD], a_ix[A_LD], a_img[A_LD];       // generic path: pixel decomposition
    int a_base[A_LD];                               // fast path
    uint32_t a_mask[A_LD], b_base[B_LD];
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
        const int m = m0 + prow + j * RPP;
        a_base[j] = 0;
        a_mask[j] = 0;
        if (m < a.M) {
            const uint32_t b = fdiv((uint32_t)m, a.div_howo);
            const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
            const uint32_t yo = fdiv(rem, a.div_wo);
            const uint32_t xo = rem - yo * (uint32_t)a.Wo;
            if (MODE == 0) {
                a_iy[j] = (int)yo * a.stride - a.pad;
                a_ix[j] = (int)xo * a.stride - a.pad;
            } else {
                a_iy[j] = (int)yo + a.pad;
                a_ix[j] = (int)xo + a.pad;
            }
            a_img[j] = (int)b * a.Hi;
            if constexpr (ALIGNED) {
                const int by = MODE == 0 ? a_iy[j] : (a_iy[j] >> sh2), bx = MODE == 0 ? a_ix[j] : (a_ix[j] >> sh2);
                a_base[j] = (((a_img[j] + by) * a.Wi + bx) * a.ldx + kvec * VEC) * ES;
                uint32_t mk = 0;
                for (int r = 0, t = 0; r < a.R; ++r)
                    for (int q = 0; q < a.S; ++q, ++t) {
                        bool ok;
                        if (MODE == 0) {
                            const int ys = a_iy[j] + r * a.dil, xs = a_ix[j] + q * a.dil;
                            ok = ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
                        } else {
                            const int ty = a_iy[j] - r * a.dil, tx = a_ix[j] - q * a.dil;
                            ok = (sh2 == 0 || (((ty | tx) & 1) == 0)) && ty >= 0 && tx >= 0 &&
                                 ((ty >> sh2) < a.Hi) && ((tx >> sh2) < a.Wi);
                        }
                        mk |= ok ? (1u << t) : 0u;
                    }
                a_mask[j] = mk;
            }
        } else {
            a_iy[j] = -(1 << 28);
            a_ix[j] = -(1 << 28);
            a_img[j] = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
        const int row = prow + j * RPP, n = n0 + row;
        b_base[j] = (row < BN && n < a.N) ? (uint32_t)((n * a.Ktot + kvec * VEC) * ES) : OOB;
    }
    // scalar byte offset of filter tap (r, q) relative to tap (0, 0)
    auto tap_delta = [&](int r, int q) -> int {
        if (MODE == 0) return ((r * a.dil) * a.Wi + q * a.dil) * a.ldx * ES;
        return -((((r * a.dil) >> sh2) * a.Wi + ((q * a.dil) >> sh2)) * a.ldx) * ES;
    };

    uint4 a_reg[A_LD], b_reg[B_LD];
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

    auto load_tiles = [&](int kt, int tap_r, int tap_s, int c0) {
        if constexpr (ALIGNED) {
            const uint32_t tapbit = 1u << (tap_r * a.S + tap_s);
            const int soff = tap_delta(tap_r, tap_s) + c0 * ES;
#pragma unroll
            for (int j = 0; j < A_LD; ++j) {
                const uint32_t voff = (a_mask[j] & tapbit) ? (uint32_t)(a_base[j] + soff) : OOB;
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)voff, 0, 0);
                a_reg[j] = make_uint4(v.x, v.y, v.z, v.w);
            }
#pragma unroll
            for (int j = 0; j < B_LD; ++j) {
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)b_base[j], kt * BK * ES, 0);
                b_reg[j] = make_uint4(v.x, v.y, v.z, v.w);
            }
            return;
        }
        // ---- A operand (gathered activations)
        int r = tap_r, s = tap_s, c = c0 + kvec * VEC;
        bool kvalid = true;
        if (!ALIGNED) {
            const int k = kt * BK + kvec * VEC;
            kvalid = k < a.Ktot;
            const uint32_t tap = fdiv((uint32_t)k, a.div_c);
            c = k - (int)tap * a.C;
            r = (int)tap / a.S;
            s = (int)tap - r * a.S;
        }
#pragma unroll
        for (int j = 0; j < A_LD; ++j) {
            int ys, xs;
            bool ok = kvalid;
            if (MODE == 0) {
                ys = a_iy[j] + r * a.dil;
                xs = a_ix[j] + s * a.dil;
            } else {
                const int ty = a_iy[j] - r * a.dil, tx = a_ix[j] - s * a.dil;
                if (a.stride == 2) {
                    ok = ok && (((ty | tx) & 1) == 0);
                    ys = ty >> 1;
                    xs = tx >> 1;
                } else {
                    ys = ty;
                    xs = tx;
                }
            }
            ok = ok && ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
            if (ok) {
                const int64_t off = ((int64_t)(a_img[j] + ys) * a.Wi + xs) * a.ldx + c;
                a_reg[j] = *reinterpret_cast<const uint4*>(X + off);
            } else {
                a_reg[j] = make_uint4(0, 0, 0, 0);
            }
        }
        // ---- B operand (weights, K contiguous)
        const int kk = kt * BK + kvec * VEC;
#pragma unroll
        for (int j = 0; j < B_LD; ++j) {
            const int n = n0 + prow + j * RPP;
            const bool ok = (prow + j * RPP < BN) && n < a.N && (ALIGNED || kk < a.Ktot);
            if (ok)
                b_reg[j] = *reinterpret_cast<const uint4*>(Wt + (int64_t)n * a.Ktot + kk);
            else
                b_reg[j] = make_uint4(0, 0, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int j = 0; j < A_LD; ++j) {
            const int row = prow + j * RPP;
            *reinterpret_cast<uint4*>(As(buf) + row * BK + swz_chunk<T>(row, kvec) * VEC) = a_reg[j];
        }
#pragma unroll
        for (int j = 0; j < B_LD; ++j) {
            const int row = prow + j * RPP;
            if ((BN % RPP) == 0 || row < BN)
                *reinterpret_cast<uint4*>(Bs(buf) + row * BK + swz_chunk<T>(b_rho<NT>(row), kvec) * VEC) = b_reg[j];
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int KT = (a.Ktot + BK - 1) / BK;
    int tap_r = 0, tap_s = 0, c0 = 0;
    auto advance = [&]() {
        if (ALIGNED) {
            c0 += BK;
            if (c0 >= a.C) {
                c0 = 0;
                if (++tap_s == a.S) { tap_s = 0; ++tap_r; }
            }
        }
    };

    load_tiles(0, tap_r, tap_s, c0);
    store_tiles(0);
    __syncthreads();

    const int lr = lane & 15, lq = lane >> 4;
    int cur = 0;
    for (int kt = 0; kt < KT; ++kt) {
        const bool has_next = kt + 1 < KT;
        if (has_next) {
            advance();
            load_tiles(kt + 1, tap_r, tap_s, c0);
        }
        const T* as = As(cur) + (wm * TM) * BK;
        const T* bs = Bs(cur) + (wn * TN) * BK;
        if constexpr (sizeof(T) == 2) {
            mfma_bf16x8 bf[NT], af[MT];
#pragma unroll
            for (int i = 0; i < NT; ++i)
                bf[i] = *reinterpret_cast<const mfma_bf16x8*>(bs + b_row<NT>(i, lr) * BK + swz_chunk<T>(lr, lq) * 8);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int row = j * 16 + lr;
                af[j] = *reinterpret_cast<const mfma_bf16x8*>(as + row * BK + swz_chunk<T>(row, lq) * 8);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i], af[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                float bf[NT], af[MT];
#pragma unroll
                for (int i = 0; i < NT; ++i) bf[i] = bs[b_row<NT>(i, lr) * BK + swz_chunk<T>(lr, kk) * 4 + lq];
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const int row = j * 16 + lr;
                    af[j] = as[row * BK + swz_chunk<T>(row, kk) * 4 + lq];
                }
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[i], af[j], acc[i][j], 0, 0, 0);
            }
        }
        if (has_next) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // Cut the accumulators' live ranges here: without it hipcc keeps the MFMA results un-tied through the
    // branchy epilogue and re-copies all 64 AGPRs (v_accvgpr_mov + s_nop) in EVERY K step (-35 % throughput).
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(acc[i][j]));
    conv_epilogue<T, NT, MT, MODE>(acc, a, m0 + wm * TM, n0 + wn * TN, lr, lq);
}

// ------------------------------------------------------------------------------------------------
// fp32 tensors, products on the bf16 matrix cores: three-term split.
// The exact mode's v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16 rate.  Here every fp32 operand value x is split once,
// on its way from the staging registers into LDS, into hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (24 mantissa
// bits, each residual exact in fp32), LDS holds three bf16 planes per operand tile, and a 16 x 16 x 32 block is the six
// bf16 MFMAs whose terms are above 2^-26 of the product: lo*hi', hi*lo', mid*mid', mid*hi', hi*mid', hi*hi' (small terms
// first; every bf16 x bf16 product is exact in the fp32 accumulator).  96 MFMA cycles per block instead of 256; results at
// fp32 rounding level (NOT the reference's fp32 arithmetic bit for bit: DmlConvDesc.f32_split).
// One LDS buffer of 3 x (BM + BN) x 32 bf16 = 48 KB, two barriers per K step, global loads of the next tile in flight in
// registers meanwhile; 256-register budget = two workgroups per CU.  ALIGNED shapes only (C % 32 == 0).
// ------------------------------------------------------------------------------------------------
template <int BN, int MODE>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2))) void conv_igemm_x3_kernel(const ConvArgs a) {
    typedef float T;
    constexpr int BM = 128, ES = 4;
    constexpr int KV = BK / 4;                   // 16-byte chunks (4 floats) per tile row
    constexpr int RPP = NTHREADS / KV;           // rows staged per pass
    constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
    constexpr int TM = 64, TN = BN / 2, MT = TM / 16, NT = TN / 16;
    constexpr int PA = BM * BK, PB = BN * BK;    // bf16 elements per plane
    constexpr uint32_t OOB = 0x80000000u;
    __shared__ __attribute__((aligned(256))) bf16_t smem[3 * (PA + PB)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int blk_m = tile / a.nblk_n, blk_n = tile - blk_m * a.nblk_n;
    const int m0 = blk_m * BM, n0 = blk_n * BN;
    const int kvec = tid % KV, prow = tid / KV;

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, (int)a.w_bytes, 0x00020000);
    const int sh2 = (MODE != 0 && a.stride == 2) ? 1 : 0;
    int a_base[A_LD];
    uint32_t a_mask[A_LD], b_base[B_LD];
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
        const int m = m0 + prow + j * RPP;
        a_base[j] = 0;
        a_mask[j] = 0;
        if (m < a.M) {
            const uint32_t b = fdiv((uint32_t)m, a.div_howo);
            const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
            const uint32_t yo = fdiv(rem, a.div_wo);
            const uint32_t xo = rem - yo * (uint32_t)a.Wo;
            const int iy = MODE == 0 ? (int)yo * a.stride - a.pad : (int)yo + a.pad;
            const int ix = MODE == 0 ? (int)xo * a.stride - a.pad : (int)xo + a.pad;
            const int by = MODE == 0 ? iy : (iy >> sh2), bx = MODE == 0 ? ix : (ix >> sh2);
            a_base[j] = ((((int)b * a.Hi + by) * a.Wi + bx) * a.ldx + kvec * 4) * ES;
            uint32_t mk = 0;
            for (int r = 0, t = 0; r < a.R; ++r)
                for (int q = 0; q < a.S; ++q, ++t) {
                    bool ok;
                    if (MODE == 0) {
                        const int ys = iy + r * a.dil, xs = ix + q * a.dil;
                        ok = ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
                    } else {
                        const int ty = iy - r * a.dil, tx = ix - q * a.dil;
                        ok = (sh2 == 0 || (((ty | tx) & 1) == 0)) && ty >= 0 && tx >= 0 && ((ty >> sh2) < a.Hi) &&
                             ((tx >> sh2) < a.Wi);
                    }
                    mk |= ok ? (1u << t) : 0u;
                }
            a_mask[j] = mk;
        }
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
        const int row = prow + j * RPP, n = n0 + row;
        b_base[j] = (n < a.N) ? (uint32_t)((n * a.Ktot + kvec * 4) * ES) : OOB;
    }
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t a_reg[A_LD], b_reg[B_LD];
    int tap_r = 0, tap_s = 0, c0 = 0;
    const int KT = a.Ktot / BK;
    // loads of K step kt (kt >= KT: every lane out of range -- zeros, no memory access: keeps the loop branch-free), in three
    // parts so that each staging register can be refilled right after its split has been stored
    uint32_t ld_tapbit = 0, ld_boff = 0;
    int ld_soff = 0;
    bool ld_valid = false;
    auto tap_setup = [&](int kt) {
        ld_valid = kt < KT;
        ld_tapbit = ld_valid ? 1u << ((tap_r * a.S + tap_s) & 31) : 0u;
        ld_soff = (MODE == 0 ? ((tap_r * a.dil) * a.Wi + tap_s * a.dil) * a.ldx
                             : -((((tap_r * a.dil) >> sh2) * a.Wi + ((tap_s * a.dil) >> sh2)) * a.ldx)) * ES + c0 * ES;
        ld_boff = ld_valid ? (uint32_t)(kt * BK * ES) : 0u;
        c0 += BK;
        if (c0 >= a.C) {
            c0 = 0;
            if (++tap_s == a.S) { tap_s = 0; ++tap_r; }
        }
    };
    auto load_a = [&](int j) {
        if (j < A_LD) {
            const uint32_t voff = (a_mask[j] & ld_tapbit) ? (uint32_t)(a_base[j] + ld_soff) : OOB;
            a_reg[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)voff, 0, 0);
        }
    };
    auto load_b = [&](int j) {
        if (j < B_LD) b_reg[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)(ld_valid ? b_base[j] : OOB), (int)ld_boff, 0);
    };
    auto load_tiles = [&](int kt) {
        tap_setup(kt);
#pragma unroll
        for (int j = 0; j < A_LD; ++j) load_a(j);
#pragma unroll
        for (int j = 0; j < B_LD; ++j) load_b(j);
    };
    // x -> (hi, mid, lo), four values at a time, packed as bf16 pairs; the 8-byte piece is half a 16-byte bf16 chunk
    auto split_store = [&](const u32x4_t v, bf16_t* plane0, int plane_elems, int off) {
        const float x[4] = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
        uint32_t h[2], m[2], l[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
            const float r0 = x[2 * e] - __uint_as_float(h[e] << 16), r1 = x[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u);
            m[e] = pack_bf16x2(r0, r1);
            const float s0 = r0 - __uint_as_float(m[e] << 16), s1 = r1 - __uint_as_float(m[e] & 0xffff0000u);
            l[e] = pack_bf16x2(s0, s1);
        }
        *reinterpret_cast<uint2*>(plane0 + off) = make_uint2(h[0], h[1]);
        *reinterpret_cast<uint2*>(plane0 + plane_elems + off) = make_uint2(m[0], m[1]);
        *reinterpret_cast<uint2*>(plane0 + 2 * plane_elems + off) = make_uint2(l[0], l[1]);
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int j = 0; j < A_LD; ++j) {
            const int row = prow + j * RPP;
            split_store(a_reg[j], smem, PA, row * BK + swz_chunk<bf16_t>(row, kvec >> 1) * 8 + (kvec & 1) * 4);
        }
#pragma unroll
        for (int j = 0; j < B_LD; ++j) {
            const int row = prow + j * RPP;
            split_store(b_reg[j], smem + 3 * PA, PB, row * BK + swz_chunk<bf16_t>(b_rho<NT>(row), kvec >> 1) * 8 + (kvec & 1) * 4);
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    load_tiles(0);
    store_tiles();
    __syncthreads();
    load_tiles(1);                                  // stays in registers until it is split under the MFMAs of K step 0
    const int lr = lane & 15, lq = lane >> 4;
    const bf16_t* as = smem + (wm * TM) * BK;
    const bf16_t* bs = smem + 3 * PA + (wn * TN) * BK;
    for (int kt = 0; kt < KT; ++kt) {
        // all 24 fragments of this K step first (96 registers) ...
        mfma_bf16x8 af[3][MT], bf[3][NT];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int row = j * 16 + lr;
                af[p][j] = *reinterpret_cast<const mfma_bf16x8*>(as + p * PA + row * BK + swz_chunk<bf16_t>(row, lq) * 8);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
                bf[p][i] = *reinterpret_cast<const mfma_bf16x8*>(bs + p * PB + b_row<NT>(i, lr) * BK + swz_chunk<bf16_t>(lr, lq) * 8);
        }
        __syncthreads();                        // ... so that the one LDS buffer is free while the MFMAs run
        auto mm = [&](int pb, int pa) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[pb][i], af[pa][j], acc[i][j], 0, 0, 0);
        };
        // six MFMA groups (small terms first), the split + store of the NEXT tile's eight staged chunks in between: ~2.4 VALU /
        // LDS-write instructions per MFMA, which issue in the shadow of the 16-cycle matrix operations
        auto st_a = [&](int j) {
            if (j < A_LD) {
                const int row = prow + j * RPP;
                split_store(a_reg[j], smem, PA, row * BK + swz_chunk<bf16_t>(row, kvec >> 1) * 8 + (kvec & 1) * 4);
            }
        };
        auto st_b = [&](int j) {
            if (j < B_LD) {
                const int row = prow + j * RPP;
                split_store(b_reg[j], smem + 3 * PA, PB, row * BK + swz_chunk<bf16_t>(b_rho<NT>(row), kvec >> 1) * 8 + (kvec & 1) * 4);
            }
        };
        // each staging register is refilled (K step kt + 2) as soon as its split has been stored: the load has the rest of
        // this step and the next step's fragment reads to land
        tap_setup(kt + 2);
        mm(2, 0); st_a(0); st_a(1); load_a(0); load_a(1);             // lo(w) * hi(x)
        mm(1, 1); st_a(2); st_a(3); load_a(2); load_a(3);             // mid * mid
        mm(1, 0); st_b(0); st_b(1); load_b(0); load_b(1);             // mid * hi
        mm(0, 2); st_b(2); st_b(3); load_b(2); load_b(3);             // hi * lo
        mm(0, 1);                                                     // hi * mid
        mm(0, 0);                                                     // hi * hi
        // pin the interleaving: one MFMA, then up to three VALU and one LDS write, a global load every eighth
#pragma unroll
        for (int q = 0; q < 16 * NT * MT / 4; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            if (q % (2 * NT) == 2 * NT - 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(acc[i][j]));
    conv_epilogue<T, NT, MT, MODE>(acc, a, m0 + wm * TM, n0 + wn * TN, lr, lq);
}

// ------------------------------------------------------------------------------------------------
// bf16 forward / data-gradient kernel, LDS-DMA version (requires C % 32 == 0).
// Operand tiles go HBM -> LDS with buffer_load ... lds (no VGPR round trip, no ds_write): an NST-stage ring (3: 48 KB,
// three workgroups per CU), tiles issued NST-1 K-steps ahead, counted vmcnt waits and ONE barrier per K-step.  Zero padding / masked rows
// come from the buffer descriptor's bounds check (an out-of-range voffset writes zeros to LDS).  The LDS image
// is lane-linear, so the bank-conflict swizzle is applied to the per-lane SOURCE address.
// ------------------------------------------------------------------------------------------------

// BM = 128: 4 waves (2 x 2), three workgroups per CU.  BM = 256: 8 waves (4 x 2) on the same 64 x 64 wave tile -- the
// weight tile is shared by twice the rows, so a K step moves 24 KB into LDS for 2.1 MFLOP (85 FLOP/B against 64) -- two
// workgroups per CU (72 KB of LDS each, 128-register budget).
// TMW = 128 (with BM = 256): 4 waves (2 x 2) on a 128 x 64 WAVE tile -- 32 MFMAs per wave and K step against 12 KB of
// fragment reads (the 64 x 64 wave tile: 16 against 8 KB), half the barriers per FLOP; 128 accumulator registers, two
// workgroups per CU = two waves per SIMD.
template <int BN, int MODE, int NST, int WPE = 3, int BM = 128, int TMW = 64>
__global__ __launch_bounds__(BM / TMW * 128) __attribute__((amdgpu_waves_per_eu(WPE))) void conv_igemm_dma_kernel(const ConvArgs a, const uint32_t x_bytes,
                                                                  const uint32_t w_bytes) {
    typedef bf16_t T;
    constexpr int WAVES = BM / TMW * 2, NTH = WAVES * 64, LA = NST - 1;
    constexpr int STAGE = (BM + BN) * BK;          // elements per ring stage
    constexpr int TM = TMW, TN = BN / 2, MT = TM / 16, NT = TN / 16;
    constexpr int A_I = BM / 16 / WAVES, B_I = BN / 16 / WAVES;   // DMA instructions per wave per tile (1 KiB = 16 rows each)
    static_assert(B_I >= 1, "tile too narrow for this many waves");
    constexpr int NI = A_I + B_I;
    constexpr uint32_t OOB = 0x80000000u;

    __shared__ __attribute__((aligned(1024))) T smem[NST * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // whole tiles first (XCD-aware order), then the K-split parts of the remainder tiles
    int tile, kpart = 0, kparts = 1;
    if (a.tail_q > 1) {
        if ((int)blockIdx.x < a.tail_full) {
            tile = xcd_remap(blockIdx.x, a.tail_full);
        } else {
            const int part = (int)blockIdx.x - a.tail_full;
            tile = a.tail_full + part / a.tail_q;
            kpart = part - (tile - a.tail_full) * a.tail_q;
            kparts = a.tail_q;
        }
    } else {
        tile = xcd_remap(blockIdx.x, gridDim.x);
    }
    const int blk_m = tile / a.nblk_n, blk_n = tile - blk_m * a.nblk_n;
    const int m0 = blk_m * BM, n0 = blk_n * BN;

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.w), 0, (int)w_bytes, 0x00020000);

    // lane -> (row within a 16-row DMA piece, 16-byte chunk); source chunk carries the XOR swizzle
    const int prow = lane >> 2;
    const int lchunk = (lane & 3) ^ ((0x78 >> (((lane >> 4) & 3) * 2)) & 3);

    // per piece and lane: signed byte offset of the row's tap-(0,0) pixel (+ swizzled chunk) and one validity bit per
    // filter tap (image border, stride-2 parity of the data gradient) -- the per-K-step part is scalar (see
    // conv_igemm_kernel)
    const int sh2 = (MODE != 0 && a.stride == 2) ? 1 : 0;
    int a_base[A_I];
    uint32_t a_mask[A_I];
#pragma unroll
    for (int jj = 0; jj < A_I; ++jj) {
        const int m = m0 + (wave * A_I + jj) * 16 + prow;
        a_base[jj] = 0;
        a_mask[jj] = 0;
        if (m < a.M) {
            const uint32_t b = fdiv((uint32_t)m, a.div_howo);
            const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
            const uint32_t yo = fdiv(rem, a.div_wo);
            const uint32_t xo = rem - yo * (uint32_t)a.Wo;
            const int iy = MODE == 0 ? (int)yo * a.stride - a.pad : (int)yo + a.pad;
            const int ix = MODE == 0 ? (int)xo * a.stride - a.pad : (int)xo + a.pad;
            const int by = MODE == 0 ? iy : (iy >> sh2), bx = MODE == 0 ? ix : (ix >> sh2);
            a_base[jj] = ((((int)b * a.Hi + by) * a.Wi + bx) * a.ldx + lchunk * 8) * 2;
            uint32_t mk = 0;
            for (int r = 0, t = 0; r < a.R; ++r)
                for (int q = 0; q < a.S; ++q, ++t) {
                    bool ok;
                    if (MODE == 0) {
                        const int ys = iy + r * a.dil, xs = ix + q * a.dil;
                        ok = ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
                    } else {
                        const int ty = iy - r * a.dil, tx = ix - q * a.dil;
                        ok = (sh2 == 0 || (((ty | tx) & 1) == 0)) && ty >= 0 && tx >= 0 && ((ty >> sh2) < a.Hi) &&
                             ((tx >> sh2) < a.Wi);
                    }
                    mk |= ok ? (1u << t) : 0u;
                }
            a_mask[jj] = mk;
        }
    }
    uint32_t b_off[B_I];
#pragma unroll
    for (int jj = 0; jj < B_I; ++jj) {
        const int row = (wave * B_I + jj) * 16 + prow, n = n0 + row;
        const int bchunk = swz_chunk<T>(b_rho<NT>(row), lane & 3);      // weight rows: swizzle keyed on the MFMA row
        // tile-major weights [N / 64][K / 32][64][32]: the instruction's 16 rows x 64 bytes are one contiguous KB
        b_off[jj] = n >= a.N ? OOB
                    : a.w_tiled ? (uint32_t)(((int64_t)(n >> 6) * (a.Ktot / BK) * 2048 + (n & 63) * 32 + bchunk * 8) * 2)
                                : (uint32_t)(((int64_t)n * a.Ktot + bchunk * 8) * 2);
    }
    const uint32_t b_kstep = a.w_tiled ? 64u * BK * 2u : BK * 2u;       // bytes from one K step of a weight row to the next

    const int KTall = a.Ktot / BK;
    const int kbeg = (int)((int64_t)kpart * KTall / kparts), kend = (int)((int64_t)(kpart + 1) * KTall / kparts);
    int ir = 0, is = 0, ic0 = 0;       // filter tap / channel offset of the next tile to issue
    if (kbeg > 0) {
        const int per_tap = a.C / BK, tap = kbeg / per_tap;
        ic0 = (kbeg - tap * per_tap) * BK;
        ir = tap / a.S;
        is = tap - ir * a.S;
    }
    auto issue = [&](int kt, int stage) {
        T* sbase = smem + stage * STAGE;
        const uint32_t tapbit = 1u << (ir * a.S + is);
        const int soff = (MODE == 0 ? ((ir * a.dil) * a.Wi + is * a.dil) * a.ldx
                                    : -((((ir * a.dil) >> sh2) * a.Wi + ((is * a.dil) >> sh2)) * a.ldx)) * 2 + ic0 * 2;
#pragma unroll
        for (int jj = 0; jj < A_I; ++jj) {
            const uint32_t voff = (a_mask[jj] & tapbit) ? (uint32_t)(a_base[jj] + soff) : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(sbase + (wave * A_I + jj) * 16 * BK), 16, voff, 0, 0, 0);
        }
#pragma unroll
        for (int jj = 0; jj < B_I; ++jj) {    // OOB + K offset stays past the descriptor's range (tensors < 2^31 bytes)
            const uint32_t voff = b_off[jj] + (uint32_t)kt * b_kstep;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(sbase + BM * BK + (wave * B_I + jj) * 16 * BK), 16, voff, 0, 0, 0);
        }
        ic0 += BK;
        if (ic0 >= a.C) {
            ic0 = 0;
            if (++is == a.S) { is = 0; ++ir; }
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int KT = kend - kbeg;
#pragma unroll
    for (int t = 0; t < LA; ++t)
        if (t < KT) issue(kbeg + t, t);

    const int lr = lane & 15, lq = lane >> 4;
    for (int kt = 0; kt < KT; ++kt) {
        // tiles kt .. min(kt + LA - 1, KT - 1) are in flight; tile kt must have landed
        if (LA > 2 && kt + 2 < KT) wait_vmcnt<(LA > 2 ? 2 : 0) * NI>();
        else if (LA > 1 && kt + 1 < KT) wait_vmcnt<(LA > 1 ? 1 : 0) * NI>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + LA < KT) issue(kbeg + kt + LA, (kt + LA) % NST);
        const T* as = smem + (kt % NST) * STAGE + (wm * TM) * BK;
        const T* bs = smem + (kt % NST) * STAGE + BM * BK + (wn * TN) * BK;
        mfma_bf16x8 bf[NT], af[MT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
            bf[i] = *reinterpret_cast<const mfma_bf16x8*>(bs + b_row<NT>(i, lr) * BK + swz_chunk<T>(lr, lq) * 8);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int row = j * 16 + lr;
            af[j] = *reinterpret_cast<const mfma_bf16x8*>(as + row * BK + swz_chunk<T>(row, lq) * 8);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i], af[j], acc[i][j], 0, 0, 0);
    }
    // Cut the accumulators' live ranges here: without it hipcc keeps the MFMA results un-tied through the
    // branchy epilogue and re-copies all 64 AGPRs (v_accvgpr_mov + s_nop) in EVERY K step (-35 % throughput).
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(acc[i][j]));
    if (kparts > 1) {
        // K-split remainder tile: park this part's fp32 accumulators (lane-linear: one 4 KB row per (i, j)), publish,
        // and let the part that arrives last add all parts in part order -- deterministic -- and finish the tile.
        const int rt = tile - a.tail_full;
        // write-through (sc1) slab stores and sc1 loads instead of release / acquire fences: a release fence writes back
        // every dirty line of this XCD's L2 -- the other workgroups' output tiles included (first version: -2.3 % on the
        // whole step).  cdna_hip_programming.md, split-K seam: sc1 stores -> drained -> barrier -> relaxed ticket; the
        // last arriver reads with sc1 loads.
        typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t rs_ws = __builtin_amdgcn_make_buffer_rsrc(
            a.tail_ws + (int64_t)rt * kparts * (BM * BN), 0, kparts * BM * BN * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), rs_ws,
                                                       (kpart * BM * BN + ((i * MT + j) * NTH + tid) * 4) * 4, 0, 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem);            // the operand ring is free now
        if (tid == 0) {
            const int ticket = __hip_atomic_fetch_add(a.tail_cnt + rt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == kparts - 1)
                __hip_atomic_store(a.tail_cnt + rt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
            *flag = ticket;
        }
        __syncthreads();
        if (*flag != kparts - 1) return;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < kparts; ++p) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(
                        rs_ws, (p * BM * BN + ((i * MT + j) * NTH + tid) * 4) * 4, 0, 16);
                    acc[i][j] += __builtin_bit_cast(f32x4, v);
                }
        }
    }
    if constexpr (MT == 4) {
        conv_epilogue<T, NT, MT, MODE>(acc, a, m0 + wm * TM, n0 + wn * TN, lr, lq);
    } else {
        // 128-row wave tile: the epilogue's statistics / BN-backward partials are per DML_STAT_ROWS = 64 rows, so it runs
        // once per 64-row half (which also halves its register footprint)
#pragma unroll
        for (int h = 0; h < MT / 4; ++h) {
            f32x4 sub[NT][4];
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sub[i][j] = acc[i][h * 4 + j];
            conv_epilogue<T, NT, 4, MODE, false>(sub, a, m0 + wm * TM + h * 64, n0 + wn * TN, lr, lq);
        }
    }
}

// The library's run-time switches (conv_choice.h: ConvSwitches), read once: the library's one look at the environment.
static const conv_choice::ConvSwitches& conv_switches() {
    static const conv_choice::ConvSwitches s = {getenv("DML_CONV_V1") != nullptr, getenv("DML_CONV_BM256") ? atoi(getenv("DML_CONV_BM256")) : 1,
                                                getenv("DML_CONV_WS") ? atoi(getenv("DML_CONV_WS")) : 0};
    return s;
}

// ------------------------------------------------------------------------------------------------
// weight-gradient kernel: dw[n][kc] += sum_m dy[m][n] * x[src(m, tap(kc))][c(kc)]
// tile 128 (n) x 128 (kc), K loop over 32-pixel slabs, split over the pixel dimension.
// Both operands are "K-major" in memory (pixel rows, channel contiguous): the bf16 fragments are
// read with the gfx950 LDS transpose read ds_read_b64_tr_b16, the fp32 ones need no transpose.
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
    const void* x;
    const void* dy;
    float* dw;
    int B, Hi, Wi, C, ldx;
    int Ho, Wo, N, ldy;
    int R, S, stride, dil, pad;
    int M, Ktot;
    int nblk_n, nblk_k;
    int slab_tiles;   // K tiles (of 32 pixels) per split
    float* ws;        // optional split-K workspace [splits][N][Ktot]: plain stores instead of atomics
    FastDiv div_wo, div_howo, div_c;
    // f32_split == 2: fp16 hi / lo planes of both operands (DmlWgradDesc::x_planes ...)
    const void* x_planes;
    const void* dy_planes;
    const float* x_unscale;
    const float* dy_unscale;
    uint32_t x_plane_bytes, dy_plane_bytes;
};

template <typename T> struct WgLds;
template <> struct WgLds<float> { static constexpr int PITCH = 128 + 16; };    // floats; banks (kg*16 + i)
template <> struct WgLds<bf16_t> { static constexpr int PITCH = 128 + 8; };    // bf16

__device__ __forceinline__ bf16x4 lds_tr16_b64(const bf16_t* p) {
    // 16 lanes x 4 bf16 block transposed in hardware (ds_read_b64_tr_b16)
    typedef short v4i16 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4i16 __attribute__((address_space(3)))*)(p));
}

template <typename T>
__global__ __launch_bounds__(NTHREADS) void conv_wgrad_kernel(const WgradArgs a) {
    constexpr int TILE = 128;
    constexpr int VEC = Elem<T>::VEC;
    constexpr int CV = TILE / VEC;                // 16-byte vectors per tile row (16 bf16 / 32 f32)
    constexpr int RPP = NTHREADS / CV;            // rows per pass (16 / 8)
    constexpr int LD = BK / RPP;                  // loads per thread per operand (2 / 4)
    constexpr int PITCH = WgLds<T>::PITCH;
    constexpr int MT = 4, NT = 4;                 // wave tile 64 (n) x 64 (kc)

    __shared__ __attribute__((aligned(16))) T smem[2 * 2 * BK * PITCH];
    auto Ys = [&](int buf) -> T* { return smem + buf * 2 * BK * PITCH; };
    auto Xs = [&](int buf) -> T* { return smem + buf * 2 * BK * PITCH + BK * PITCH; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1;
    // 1-D grid, XCD-aware: every (n, kc) tile of one pixel slab runs on the same XCD, so the dy / x slabs are
    // fetched into that XCD's L2 once instead of once per XCD (PMC: 363 MB fetched per launch before, see DESIGN)
    const int ntile = a.nblk_n * a.nblk_k;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, tile_id = logical - split * ntile;
    const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
    const int n0 = blk_n * TILE, kc0 = blk_k * TILE;

    const T* __restrict__ X = static_cast<const T*>(a.x);
    const T* __restrict__ DY = static_cast<const T*>(a.dy);

    const int vcol = tid % CV, prow = tid / CV;
    // this thread's fixed filter tap / channel for the X operand
    const int kc = kc0 + vcol * VEC;
    const bool kc_ok = kc < a.Ktot;
    const uint32_t tap = fdiv((uint32_t)(kc_ok ? kc : 0), a.div_c);
    const int xc = (kc_ok ? kc : 0) - (int)tap * a.C;
    const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
    const int dyo = tr * a.dil - a.pad, dxo = ts * a.dil - a.pad;
    const int yn = n0 + vcol * VEC;
    const bool yn_ok = yn < a.N;

    const int tile_beg = split * a.slab_tiles;
    const int tiles_total = (a.M + BK - 1) / BK;
    const int tile_end = min(tiles_total, tile_beg + a.slab_tiles);

    const bool lin1x1 = a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0;
    uint4 y_reg[LD], x_reg[LD];
    auto load_tiles = [&](int t) {
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const int m = t * BK + prow + j * RPP;
            uint4 yv = make_uint4(0, 0, 0, 0), xv = make_uint4(0, 0, 0, 0);
            if (m < a.M) {
                if (yn_ok) yv = *reinterpret_cast<const uint4*>(DY + (int64_t)m * a.ldy + yn);
                if (kc_ok && lin1x1) {
                    xv = *reinterpret_cast<const uint4*>(X + (int64_t)m * a.ldx + xc);      // 1x1 stride 1: source pixel = m
                } else if (kc_ok) {
                    const uint32_t b = fdiv((uint32_t)m, a.div_howo);
                    const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
                    const uint32_t yo = fdiv(rem, a.div_wo);
                    const uint32_t xo = rem - yo * (uint32_t)a.Wo;
                    const int ys = (int)yo * a.stride + dyo, xs = (int)xo * a.stride + dxo;
                    if ((unsigned)ys < (unsigned)a.Hi && (unsigned)xs < (unsigned)a.Wi)
                        xv = *reinterpret_cast<const uint4*>(
                            X + ((int64_t)((int)b * a.Hi + ys) * a.Wi + xs) * a.ldx + xc);
                }
            }
            y_reg[j] = yv;
            x_reg[j] = xv;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const int row = prow + j * RPP;
            int off;
            if constexpr (sizeof(T) == 2) {
                // bf16: 16-column sub-tiles [col/16][k'][16] (1056-byte pitch), k rows stored with bits 2/3 swapped:
                // conflict-free for ds_read_b64_tr_b16 (2 x 32 lanes, 64 banks) and for these 16-byte writes
                const int prow_ = (row & 0x13) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 3);
                off = (vcol >> 1) * 528 + prow_ * 16 + (vcol & 1) * 8;
            } else {
                off = row * PITCH + vcol * VEC;
            }
            *reinterpret_cast<uint4*>(Ys(buf) + off) = y_reg[j];
            *reinterpret_cast<uint4*>(Xs(buf) + off) = x_reg[j];
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (tile_beg < tile_end) {
        load_tiles(tile_beg);
        store_tiles(0);
    }
    __syncthreads();

    const int lr = lane & 15, lq = lane >> 4;
    int cur = 0;
    for (int t = tile_beg; t < tile_end; ++t) {
        const bool has_next = t + 1 < tile_end;
        if (has_next) load_tiles(t + 1);
        const T* ys = Ys(cur) + (sizeof(T) == 2 ? wn * 4 * 528 : wn * 64);
        const T* xs = Xs(cur) + (sizeof(T) == 2 ? wk * 4 * 528 : wk * 64);
        if constexpr (sizeof(T) == 2) {
            // A[i = n][k = pixel]: lanes of a 16-group address the 4 x 16 block (rows k0..k0+3,
            // cols 16*i..) in 8-byte pieces: lane L -> row L/4, cols 4*(L%4)..; the hardware
            // returns to lane i the 4 k-values of column i.
            mfma_bf16x8 af[NT], bfr[MT];
            // k rows 8*lq + (lr>>2) (+4 for the second read) at their swapped positions inside a sub-tile
            const int p_lo = ((lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4)) * 16 + (lr & 3) * 4;
            const int p_hi = p_lo + 8 * 16;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const bf16x4 lo = lds_tr16_b64(ys + i * 528 + p_lo);
                const bf16x4 hi = lds_tr16_b64(ys + i * 528 + p_hi);
                bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                af[i] = __builtin_bit_cast(mfma_bf16x8, v);
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const bf16x4 lo = lds_tr16_b64(xs + j * 528 + p_lo);
                const bf16x4 hi = lds_tr16_b64(xs + j * 528 + p_hi);
                bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                bfr[j] = __builtin_bit_cast(mfma_bf16x8, v);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                float af[NT], bfr[MT];
#pragma unroll
                for (int i = 0; i < NT; ++i) af[i] = ys[(kk * 4 + lq) * PITCH + i * 16 + lr];
#pragma unroll
                for (int j = 0; j < MT; ++j) bfr[j] = xs[(kk * 4 + lq) * PITCH + j * 16 + lr];
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
        if (has_next) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // acc[i][j][q] = dw[n = n0 + wn*64 + i*16 + lq*4 + q][kc = kc0 + wk*64 + j*16 + lr]
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + wn * 64 + i * 16 + lq * 4 + q;
            if (n >= a.N) continue;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int k = kc0 + wk * 64 + j * 16 + lr;
                if (k < a.Ktot) {
                    if (a.ws != nullptr)
                        a.ws[((int64_t)split * a.N + n) * a.Ktot + k] = acc[i][j][q];
                    else
                        atomicAdd(a.dw + (int64_t)n * a.Ktot + k, acc[i][j][q]);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------
// fp32 weight gradient with the products on the bf16 matrix cores (three-term split, see conv_igemm_x3_kernel): the
// 128 x 128 tile / split-K scheme of conv_wgrad_kernel<float>, the fp32 operand tiles split into (hi, mid, lo) bf16 planes
// on their way from the staging registers into LDS -- in conv_wgrad_kernel<bf16_t>'s sub-tiled image, so that the
// fragments come out of ds_read_b64_tr_b16 -- and six MFMA groups per K step.  One LDS buffer (51 KB), two barriers per
// step, the next tile's split + store interleaved with the MFMAs, global loads a whole step ahead in registers.
// ------------------------------------------------------------------------------------------------
template <bool LIN>      // LIN: 1x1, stride 1, no padding -- pixel row m of x is output row m
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2))) void conv_wgrad_x3_kernel(
    const WgradArgs a, const uint32_t x_bytes, const uint32_t dy_bytes) {
    constexpr int TILE = 128, CV = TILE / 4, RPP = NTHREADS / CV, LD = BK / RPP;      // 32 float4 per row, 8 rows per pass, 4 loads
    constexpr int SUB = 528, PL = (TILE / 16) * SUB;                                   // bf16 elements per operand plane
    constexpr int MT = 4, NT = 4;
    constexpr uint32_t OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) bf16_t smem[6 * PL];
    bf16_t* const Ys = smem;                     // planes hi, mid, lo of dy
    bf16_t* const Xs = smem + 3 * PL;            // planes of x

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1;
    const int ntile = a.nblk_n * a.nblk_k;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, tile_id = logical - split * ntile;
    const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
    const int n0 = blk_n * TILE, kc0 = blk_k * TILE;
    // out-of-range rows / columns / taps read through the descriptors' range check: zeros, no branch, no access
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)dy_bytes, 0x00020000);
    const int vcol = tid % CV, prow = tid / CV;
    const int kc = kc0 + vcol * 4;
    const bool kc_ok = kc < a.Ktot;
    const uint32_t tap = fdiv((uint32_t)(kc_ok ? kc : 0), a.div_c);
    const int xc = (kc_ok ? kc : 0) - (int)tap * a.C;
    const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
    const int dyo = tr * a.dil - a.pad, dxo = ts * a.dil - a.pad;
    const int yn = n0 + vcol * 4;
    const bool yn_ok = yn < a.N;
    const int tile_beg = split * a.slab_tiles;
    const int tiles_total = (a.M + BK - 1) / BK;
    const int tile_end = min(tiles_total, tile_beg + a.slab_tiles);

    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t y_reg[LD], x_reg[LD];
    auto load_row = [&](int t, int j) {
        const int m = t * BK + prow + j * RPP;
        const bool mv = t < tile_end && m < a.M;
        uint32_t xo_b;
        bool xv = mv && kc_ok;
        if (LIN) {
            xo_b = ((uint32_t)m * (uint32_t)a.ldx + (uint32_t)xc) * 4u;
        } else {
            const uint32_t b = fdiv((uint32_t)m, a.div_howo);
            const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
            const uint32_t yo = fdiv(rem, a.div_wo);
            const uint32_t xo = rem - yo * (uint32_t)a.Wo;
            const int ys = (int)yo * a.stride + dyo, xs = (int)xo * a.stride + dxo;
            xv = xv && (unsigned)ys < (unsigned)a.Hi && (unsigned)xs < (unsigned)a.Wi;
            xo_b = ((uint32_t)(((int)b * a.Hi + ys) * a.Wi + xs) * (uint32_t)a.ldx + (uint32_t)xc) * 4u;
        }
        const uint32_t yo_b = ((uint32_t)m * (uint32_t)a.ldy + (uint32_t)yn) * 4u;
        y_reg[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_y, (int)((mv && yn_ok) ? yo_b : OOB), 0, 0);
        x_reg[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)(xv ? xo_b : OOB), 0, 0);
    };
    auto split_store = [&](const u32x4_t v, bf16_t* plane0, int off) {
        const float x[4] = {__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
        uint32_t h[2], m[2], l[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
            const float r0 = x[2 * e] - __uint_as_float(h[e] << 16), r1 = x[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u);
            m[e] = pack_bf16x2(r0, r1);
            const float s0 = r0 - __uint_as_float(m[e] << 16), s1 = r1 - __uint_as_float(m[e] & 0xffff0000u);
            l[e] = pack_bf16x2(s0, s1);
        }
        *reinterpret_cast<uint2*>(plane0 + off) = make_uint2(h[0], h[1]);
        *reinterpret_cast<uint2*>(plane0 + PL + off) = make_uint2(m[0], m[1]);
        *reinterpret_cast<uint2*>(plane0 + 2 * PL + off) = make_uint2(l[0], l[1]);
    };
    // conv_wgrad_kernel<bf16_t>'s image: 16-column sub-tiles [col / 16][k'][16], k rows with bits 2 / 3 swapped; this
    // thread's four columns are a quarter of a sub-tile row
    auto lds_off = [&](int j) {
        const int row = prow + j * RPP;
        const int prow_ = (row & 0x13) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 3);
        return (vcol >> 2) * SUB + prow_ * 16 + (vcol & 3) * 4;
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < LD; ++j) load_row(tile_beg, j);
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        split_store(y_reg[j], Ys, lds_off(j));
        split_store(x_reg[j], Xs, lds_off(j));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LD; ++j) load_row(tile_beg + 1, j);
    const int lr = lane & 15, lq = lane >> 4;
    const int p_lo = ((lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4)) * 16 + (lr & 3) * 4;
    const int p_hi = p_lo + 8 * 16;
    const bf16_t* ys = Ys + wn * 4 * SUB;
    const bf16_t* xs = Xs + wk * 4 * SUB;
    for (int t = tile_beg; t < tile_end; ++t) {
        mfma_bf16x8 af[3][NT], bfr[3][MT];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const bf16x4 lo = lds_tr16_b64(ys + p * PL + i * SUB + p_lo);
                const bf16x4 hi = lds_tr16_b64(ys + p * PL + i * SUB + p_hi);
                bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                af[p][i] = __builtin_bit_cast(mfma_bf16x8, v);
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const bf16x4 lo = lds_tr16_b64(xs + p * PL + j * SUB + p_lo);
                const bf16x4 hi = lds_tr16_b64(xs + p * PL + j * SUB + p_hi);
                bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                bfr[p][j] = __builtin_bit_cast(mfma_bf16x8, v);
            }
        }
        __syncthreads();
        auto mm = [&](int py, int px) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[py][i], bfr[px][j], acc[i][j], 0, 0, 0);
        };
        // each staging register is refilled (tile t + 2) as soon as its split has been stored: the load has the rest of this
        // step and the next step's fragment reads to land
        mm(2, 0); split_store(y_reg[0], Ys, lds_off(0)); split_store(x_reg[0], Xs, lds_off(0)); load_row(t + 2, 0);
        mm(0, 2); split_store(y_reg[1], Ys, lds_off(1)); split_store(x_reg[1], Xs, lds_off(1)); load_row(t + 2, 1);
        mm(1, 1); split_store(y_reg[2], Ys, lds_off(2)); split_store(x_reg[2], Xs, lds_off(2)); load_row(t + 2, 2);
        mm(1, 0); split_store(y_reg[3], Ys, lds_off(3)); split_store(x_reg[3], Xs, lds_off(3)); load_row(t + 2, 3);
        mm(0, 1);
        mm(0, 0);
#pragma unroll
        for (int q = 0; q < 64; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, LIN ? 3 : 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            if (q % 8 == 7) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __syncthreads();
    }
    // acc[i][j][q] = dw[n = n0 + wn*64 + i*16 + lq*4 + q][kc = kc0 + wk*64 + j*16 + lr]
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + wn * 64 + i * 16 + lq * 4 + q;
            if (n >= a.N) continue;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int k = kc0 + wk * 64 + j * 16 + lr;
                if (k < a.Ktot) {
                    if (a.ws != nullptr)
                        a.ws[((int64_t)split * a.N + n) * a.Ktot + k] = acc[i][j][q];
                    else
                        atomicAdd(a.dw + (int64_t)n * a.Ktot + k, acc[i][j][q]);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------
// fp32 weight gradient with the products on the fp16 matrix cores: both operands as two fp16 planes of the scaled tensors
// (dml_h2_split; DmlWgradDesc.x_planes / dy_planes).  conv_wgrad_kernel<bf16_t>'s 128 x 128 tile, sub-tiled LDS image and
// ds_read_b64_tr_b16 fragments, with four operand planes per stage and three MFMA groups per 32-pixel K step
// (dy_l x_h, dy_h x_l, dy_h x_h): 48 MFMAs per wave against 16 bytes x 8 loads per thread -- no VALU split in the loop, the
// planes were written once by the producer of the tensor.  Double-buffered LDS (68 KB: two workgroups per CU), loads of step
// t + 1 in registers while step t computes.  Same split-K / workspace scheme as the other weight-gradient kernels.
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// Weight gradient on fp16 planes, wave-specialised (the structure of conv_ws_kernel): three loader waves bring a K step -- 32
// pixels of dy [32][128] and of the gathered x [32][256], hi and lo plane each, 48 KB -- into a 3-stage LDS ring with LDS-DMA
// (whole 256 / 512-byte pixel rows per piece: the operands are pixel-major in memory), four consumer waves (2 x 2, wave tile
// 64 n x 128 kc = 32 accumulator fragments) read transposed fragments (ds_read_b64_tr_b16 on the row-major image, 16-byte chunk
// index XOR 2 (row & 7): conflict-free) and issue 96 MFMAs per K step.  Persistent workgroups walk the (output tile, pixel slab)
// list; slabs go to the workspace and wgrad_reduce_kernel folds them as for the other kernels.
// ------------------------------------------------------------------------------------------------
constexpr int WGW_NST = 3, WGW_NLD = 3;
constexpr int WGW_TN = 128, WGW_TK = 256;
constexpr int WGW_YROW = WGW_TN * 2, WGW_XROW = WGW_TK * 2;                  // bytes per pixel row and plane
constexpr int WGW_YPL = 32 * WGW_YROW, WGW_XPL = 32 * WGW_XROW;              // bytes per plane and stage
constexpr int WGW_SB = 2 * WGW_YPL + 2 * WGW_XPL;                            // [dy hi | dy lo | x hi | x lo] = 48 KB

template <bool LIN, int LW>
__device__ __forceinline__ void wgrad_ws_loader(const WgradArgs& a, const uint32_t x_bytes, const uint32_t dy_bytes, char* smem,
                                                uint32_t* ready, uint32_t* consumed, const int lane, const int nitems, const int ntile) {
    constexpr int NLD = WGW_NLD, NST = WGW_NST, NG = 24, MYG = NG / NLD;         // row groups: 8 of dy (4 rows), 16 of x (2 rows)
    constexpr uint32_t OOB = 0x80000000u;
    const u32x4_ws rs_x = ws_make_rsrc(a.x_planes, x_bytes + a.x_plane_bytes), rs_y = ws_make_rsrc(a.dy_planes, dy_bytes + a.dy_plane_bytes);
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    const int tiles_total = (a.M + BK - 1) / BK;
    uint32_t g = 0, pub = 0;
    for (int item = xcd_remap(blockIdx.x, gridDim.x); item < nitems; item += (int)gridDim.x) {      // (neighbouring items -- the tiles of one pixel slab -- on one XCD: they share dy and x rows in its L2)
        const int split = item / ntile, tile_id = item - split * ntile;
        const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
        const int n0 = blk_n * WGW_TN, kc0 = blk_k * WGW_TK;
        const int tile_beg = split * a.slab_tiles, tile_end = min(tiles_total, tile_beg + a.slab_tiles);
        const int m_end = min(a.M, tile_end * BK);
        int row[MYG], colb[MYG], dyo[MYG], dxo[MYG];
        bool cok[MYG];
#pragma unroll
        for (int q = 0; q < MYG; ++q) {
            const int gi = q * NLD + LW;
            if (gi < 8) {
                row[q] = gi * 4 + (lane >> 4);
                const int gch = (lane & 15) ^ (2 * (row[q] & 7));
                const int n = n0 + gch * 8;
                cok[q] = n < a.N;
                colb[q] = n * 2;
                dyo[q] = dxo[q] = 0;
            } else {
                row[q] = (gi - 8) * 2 + (lane >> 5);
                const int gch = (lane & 31) ^ (2 * (row[q] & 7));
                const int kc = kc0 + gch * 8;
                cok[q] = kc < a.Ktot;
                const uint32_t tap = fdiv((uint32_t)(cok[q] ? kc : 0), a.div_c);
                const int xc = (cok[q] ? kc : 0) - (int)tap * a.C;
                const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
                dyo[q] = tr * a.dil - a.pad;
                dxo[q] = ts * a.dil - a.pad;
                colb[q] = xc * 2;
            }
        }
        for (int t = tile_beg; t < tile_end; ++t) {
            if (g >= (uint32_t)NST) {
                const uint32_t need = g - NST + 1;
                bool drained = false;
                for (;;) {
                    uint32_t mn = ws_ld(consumed);
#pragma unroll
                    for (int w = 1; w < 4; ++w) mn = min(mn, ws_ld(consumed + w));
                    if (mn >= need) break;
                    if (!drained) {
                        wait_vmcnt<0>();
                        ws_st(ready + LW, g);
                        pub = g;
                        drained = true;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
            }
            const uint32_t sbase = lds0 + (g % NST) * WGW_SB;
#pragma unroll
            for (int q = 0; q < MYG; ++q) {
                const int gi = q * NLD + LW;
                const int m = t * BK + row[q];
                bool ok = cok[q] && m < m_end;
                uint32_t voff;
                if (gi < 8) {
                    voff = (uint32_t)m * (uint32_t)(a.ldy * 2) + (uint32_t)colb[q];
                    ws_dma16(rs_y, sbase + gi * 1024, ok ? voff : OOB, 0u);
                    ws_dma16(rs_y, sbase + WGW_YPL + gi * 1024, ok ? voff : OOB, a.dy_plane_bytes);
                } else {
                    if (LIN) {
                        voff = (uint32_t)m * (uint32_t)(a.ldx * 2) + (uint32_t)colb[q];
                    } else {
                        const uint32_t mm = ok ? (uint32_t)m : 0u;
                        const uint32_t b = fdiv(mm, a.div_howo);
                        const uint32_t rem = mm - b * (uint32_t)(a.Ho * a.Wo);
                        const uint32_t yo = fdiv(rem, a.div_wo);
                        const uint32_t xo = rem - yo * (uint32_t)a.Wo;
                        const int ys = (int)yo * a.stride + dyo[q], xs = (int)xo * a.stride + dxo[q];
                        ok = ok && (unsigned)ys < (unsigned)a.Hi && (unsigned)xs < (unsigned)a.Wi;
                        voff = (uint32_t)(((int)b * a.Hi + ys) * a.Wi + xs) * (uint32_t)(a.ldx * 2) + (uint32_t)colb[q];
                    }
                    const int xi = gi - 8;
                    ws_dma16(rs_x, sbase + 2 * WGW_YPL + xi * 1024, ok ? voff : OOB, 0u);
                    ws_dma16(rs_x, sbase + 2 * WGW_YPL + WGW_XPL + xi * 1024, ok ? voff : OOB, a.x_plane_bytes);
                }
            }
            ++g;
            if (g > 1u + pub) {
                wait_vmcnt<2 * MYG>();             // one stage of this wave's pieces in flight behind the one it publishes
                pub = g - 1;
                ws_st(ready + LW, pub);
            }
        }
    }
    wait_vmcnt<0>();
    ws_st(ready + LW, g);
}

template <bool LIN>
__global__ __launch_bounds__((4 + WGW_NLD) * 64) void conv_wgrad_ws_kernel(const WgradArgs a, const uint32_t x_bytes, const uint32_t dy_bytes,
                                                                          const int nitems) {
    constexpr int NST = WGW_NST, NLD = WGW_NLD, NT = 4, MT = 8;
    __shared__ __attribute__((aligned(1024))) char smem[NST * WGW_SB + 64];
    uint32_t* const ready = reinterpret_cast<uint32_t*>(smem + NST * WGW_SB);
    uint32_t* const consumed = ready + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 16) reinterpret_cast<uint32_t*>(smem + NST * WGW_SB)[tid] = 0;
    __syncthreads();
    const int ntile = a.nblk_n * a.nblk_k;
    if (wave >= 4) {
        const int lw = wave - 4;
        if (lw == 0) wgrad_ws_loader<LIN, 0>(a, x_bytes, dy_bytes, smem, ready, consumed, lane, nitems, ntile);
        if (lw == 1) wgrad_ws_loader<LIN, 1>(a, x_bytes, dy_bytes, smem, ready, consumed, lane, nitems, ntile);
        if (lw == 2) wgrad_ws_loader<LIN, 2>(a, x_bytes, dy_bytes, smem, ready, consumed, lane, nitems, ntile);
        return;
    }
    // ---------------------------------------------------------------------- consumer
    __builtin_amdgcn_s_setprio(3);
    const int wn = wave >> 1, wk = wave & 1;
    const int lr = lane & 15, lq = lane >> 4;
    const int tiles_total = (a.M + BK - 1) / BK;
    uint32_t g = 0, rflag = 0;
    auto wait_ready = [&](const uint32_t need) {
        while (rflag < need) {
            __builtin_amdgcn_s_sleep(1);
            uint32_t v = ws_ld(ready);
#pragma unroll
            for (int w = 1; w < NLD; ++w) v = min(v, ws_ld(ready + w));
            rflag = v;
        }
        asm volatile("" ::: "memory");
    };
    // transposed fragment = two ds_read_b64_tr_b16 (pixel rows r, r + 8 of the lane's row group) of four channels
    const int row_lo = (lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4);
    const int sw = 2 * (row_lo & 7), sub = ((lr & 3) & 1) * 8;
    int y_off[NT], x_off[MT];
#pragma unroll
    for (int i = 0; i < NT; ++i) y_off[i] = row_lo * WGW_YROW + (((wn * 8 + i * 2 + ((lr & 3) >> 1)) ^ sw) << 4) + sub;
#pragma unroll
    for (int j = 0; j < MT; ++j) x_off[j] = 2 * WGW_YPL + row_lo * WGW_XROW + (((wk * 16 + j * 2 + ((lr & 3) >> 1)) ^ sw) << 4) + sub;
    auto frag = [&](const char* p, const int rowb) -> mfma_f16x8 {
        const bf16x4 lo = lds_tr16_b64(reinterpret_cast<const bf16_t*>(p));
        const bf16x4 hi = lds_tr16_b64(reinterpret_cast<const bf16_t*>(p + 8 * rowb));
        const bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(mfma_f16x8, v);
    };
    for (int item = xcd_remap(blockIdx.x, gridDim.x); item < nitems; item += (int)gridDim.x) {      // (neighbouring items -- the tiles of one pixel slab -- on one XCD: they share dy and x rows in its L2)
        const int split = item / ntile, tile_id = item - split * ntile;
        const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
        const int n0 = blk_n * WGW_TN, kc0 = blk_k * WGW_TK;
        const int tile_beg = split * a.slab_tiles, tile_end = min(tiles_total, tile_beg + a.slab_tiles);
        const int KT = tile_end - tile_beg;
        f32x4 acc[NT][MT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mfma_f16x8 yh[NT], yhn[NT], yl[NT], xh[2], xl[2];
        uint32_t pl[NLD];
        if (KT > 0) {
            wait_ready(g + 1);
            const char* sb = smem + (g % NST) * WGW_SB;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                yh[i] = frag(sb + y_off[i], WGW_YROW);
                yl[i] = frag(sb + y_off[i] + WGW_YPL, WGW_YROW);
            }
            xh[0] = frag(sb + x_off[0], WGW_XROW);
            xl[0] = frag(sb + x_off[0] + WGW_XPL, WGW_XROW);
        }
        for (int kt = 0; kt < KT; ++kt) {
            const bool has_next = kt + 1 < KT;
            const char* sb = smem + (g % NST) * WGW_SB;
            const char* sn = has_next ? smem + ((g + 1) % NST) * WGW_SB : sb;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                // (round 5: the transposed fragment reads of the next column group sit BETWEEN this group's three MFMA quads, as in
                // conv_ws_kernel: a cluster of reads in front of twelve MFMAs outlasts the MFMA before it)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], yh[i], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 1 < MT) xh[(j + 1) & 1] = frag(sb + x_off[j + 1], WGW_XROW);
                else xh[0] = frag(sn + x_off[0], WGW_XROW);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[j & 1], yh[i], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 1 < MT) {
                    xl[(j + 1) & 1] = frag(sb + x_off[j + 1] + WGW_XPL, WGW_XROW);
                } else {
                    asm volatile("" ::: "memory");
                    ws_st(consumed + wave, g + 1);      // every read of stage g has been issued
                    xl[0] = frag(sn + x_off[0] + WGW_XPL, WGW_XROW);
                }
                if (j == 1) {
#pragma unroll
                    for (int w = 0; w < NLD; ++w) pl[w] = ws_ld(ready + w);
                }
                if (j == 3) {
                    rflag = pl[0];
#pragma unroll
                    for (int w = 1; w < NLD; ++w) rflag = min(rflag, pl[w]);
                    if (has_next) wait_ready(g + 2);
                }
                if (j >= 4 && j < 4 + NT) yhn[j - 4] = frag(sn + y_off[j - 4], WGW_YROW);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], yl[i], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                yl[i] = frag(sn + y_off[i] + WGW_YPL, WGW_YROW);
                yh[i] = yhn[i];
            }
            __builtin_amdgcn_sched_barrier(0);
            ++g;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(acc[i][j]));
        const float un = a.x_unscale[0] * a.dy_unscale[0];
        // the x fragment is the MFMA's row operand: acc[i][j][q] = dw[n = n0 + wn*64 + i*16 + lr][kc = kc0 + wk*128 + j*16 + lq*4 + q],
        // four consecutive kc per lane -> 16-byte slab stores (Ktot % 8 == 0)
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int n = n0 + wn * 64 + i * 16 + lr;
            if (n >= a.N) continue;
            float* wrow = a.ws + ((int64_t)split * a.N + n) * a.Ktot;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int k = kc0 + wk * 128 + j * 16 + lq * 4;
                if (k < a.Ktot) *reinterpret_cast<f32x4*>(wrow + k) = acc[i][j] * un;
            }
        }
    }
}

template <bool LIN>      // LIN: 1x1, stride 1, no padding -- pixel row m of x is output row m
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2))) void conv_wgrad_h2_kernel(
    const WgradArgs a, const uint32_t x_bytes, const uint32_t dy_bytes) {
    constexpr int TILE = 128, CV = TILE / 8, RPP = NTHREADS / CV, LD = BK / RPP;       // 16 vectors per row, 16 rows per pass, 2 loads
    constexpr int SUB = 528, PLN = (TILE / 16) * SUB;                                  // fp16 elements per operand plane and stage
    constexpr int MT = 4, NT = 4;
    constexpr uint32_t OOB = 0x80000000u;
    typedef _Float16 f16_t;
    __shared__ __attribute__((aligned(16))) f16_t smem[2 * 4 * PLN];                   // [buf][dy hi, dy lo, x hi, x lo]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1;
    const int ntile = a.nblk_n * a.nblk_k;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, tile_id = logical - split * ntile;
    const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
    const int n0 = blk_n * TILE, kc0 = blk_k * TILE;
    // descriptors span both planes; the lo plane is reached through the scalar offset
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x_planes), 0, (int)(x_bytes + a.x_plane_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy_planes), 0, (int)(dy_bytes + a.dy_plane_bytes), 0x00020000);
    const int vcol = tid % CV, prow = tid / CV;
    const int kc = kc0 + vcol * 8;
    const bool kc_ok = kc < a.Ktot;
    const uint32_t tap = fdiv((uint32_t)(kc_ok ? kc : 0), a.div_c);
    const int xc = (kc_ok ? kc : 0) - (int)tap * a.C;
    const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
    const int dyo = tr * a.dil - a.pad, dxo = ts * a.dil - a.pad;
    const int yn = n0 + vcol * 8;
    const bool yn_ok = yn < a.N;
    const int tile_beg = split * a.slab_tiles;
    const int tiles_total = (a.M + BK - 1) / BK;
    const int tile_end = min(tiles_total, tile_beg + a.slab_tiles);

    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t yh_r[LD], yl_r[LD], xh_r[LD], xl_r[LD];
    auto load_row = [&](int t, int j) {
        const int m = t * BK + prow + j * RPP;
        const bool mv = t < tile_end && m < a.M;
        uint32_t xo_b;
        bool xv = mv && kc_ok;
        if (LIN) {
            xo_b = ((uint32_t)m * (uint32_t)a.ldx + (uint32_t)xc) * 2u;
        } else {
            const uint32_t b = fdiv((uint32_t)m, a.div_howo);
            const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
            const uint32_t yo = fdiv(rem, a.div_wo);
            const uint32_t xo = rem - yo * (uint32_t)a.Wo;
            const int ys = (int)yo * a.stride + dyo, xs = (int)xo * a.stride + dxo;
            xv = xv && (unsigned)ys < (unsigned)a.Hi && (unsigned)xs < (unsigned)a.Wi;
            xo_b = ((uint32_t)(((int)b * a.Hi + ys) * a.Wi + xs) * (uint32_t)a.ldx + (uint32_t)xc) * 2u;
        }
        const uint32_t yo_b = ((uint32_t)m * (uint32_t)a.ldy + (uint32_t)yn) * 2u;
        const int yoff = (int)((mv && yn_ok) ? yo_b : OOB), xoff = (int)(xv ? xo_b : OOB);
        yh_r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_y, yoff, 0, 0);
        yl_r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_y, yoff, (int)a.dy_plane_bytes, 0);
        xh_r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff, 0, 0);
        xl_r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff, (int)a.x_plane_bytes, 0);
    };
    // conv_wgrad_kernel<bf16_t>'s image: 16-column sub-tiles [col / 16][k'][16], k rows with bits 2 / 3 swapped
    auto store_tiles = [&](int buf) {
        f16_t* base = smem + buf * 4 * PLN;
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const int row = prow + j * RPP;
            const int prow_ = (row & 0x13) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 3);
            const int off = (vcol >> 1) * SUB + prow_ * 16 + (vcol & 1) * 8;
            *reinterpret_cast<u32x4_t*>(base + off) = yh_r[j];
            *reinterpret_cast<u32x4_t*>(base + PLN + off) = yl_r[j];
            *reinterpret_cast<u32x4_t*>(base + 2 * PLN + off) = xh_r[j];
            *reinterpret_cast<u32x4_t*>(base + 3 * PLN + off) = xl_r[j];
        }
    };
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (tile_beg < tile_end) {
#pragma unroll
        for (int j = 0; j < LD; ++j) load_row(tile_beg, j);
        store_tiles(0);
    }
    __syncthreads();
    const int lr = lane & 15, lq = lane >> 4;
    const int p_lo = ((lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4)) * 16 + (lr & 3) * 4;
    const int p_hi = p_lo + 8 * 16;
    auto frag = [&](const f16_t* p) -> mfma_f16x8 {
        const bf16x4 lo = lds_tr16_b64(reinterpret_cast<const bf16_t*>(p + p_lo));
        const bf16x4 hi = lds_tr16_b64(reinterpret_cast<const bf16_t*>(p + p_hi));
        const bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(mfma_f16x8, v);
    };
    int cur = 0;
    for (int t = tile_beg; t < tile_end; ++t) {
        const bool has_next = t + 1 < tile_end;
        if (has_next) {
#pragma unroll
            for (int j = 0; j < LD; ++j) load_row(t + 1, j);
        }
        const f16_t* sb = smem + cur * 4 * PLN;
        mfma_f16x8 yh[NT], yl[NT], xh[MT], xl[MT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            yh[i] = frag(sb + (wn * 4 + i) * SUB);
            yl[i] = frag(sb + PLN + (wn * 4 + i) * SUB);
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            xh[j] = frag(sb + 2 * PLN + (wk * 4 + j) * SUB);
            xl[j] = frag(sb + 3 * PLN + (wk * 4 + j) * SUB);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yl[i], xh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yh[i], xl[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yh[i], xh[j], acc[i][j], 0, 0, 0);
        if (has_next) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    const float un = a.x_unscale[0] * a.dy_unscale[0];      // exact powers of two
    // acc[i][j][q] = dw[n = n0 + wn*64 + i*16 + lq*4 + q][kc = kc0 + wk*64 + j*16 + lr]
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + wn * 64 + i * 16 + lq * 4 + q;
            if (n >= a.N) continue;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int k = kc0 + wk * 64 + j * 16 + lr;
                if (k < a.Ktot) {
                    if (a.ws != nullptr)
                        a.ws[((int64_t)split * a.N + n) * a.Ktot + k] = acc[i][j][q] * un;
                    else
                        atomicAdd(a.dw + (int64_t)n * a.Ktot + k, acc[i][j][q] * un);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient for N <= 64 output channels (layer1's 3x3 and 1x1 convolutions, the stem, the 48- and
// 16-channel head convolutions): tile 64 (n) x 256 (kc), 4 waves side by side along kc (wave tile 64 x 64).  In the
// 128 x 128 kernel half of every MFMA row block is padding for these layers and two of the four waves idle; here all
// four compute.  Same LDS image (16-column sub-tiles read with ds_read_b64_tr_b16), same split-K / workspace scheme.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void conv_wgrad_n64_kernel(const WgradArgs a) {
    typedef bf16_t T;
    constexpr int TN = 64, TK = 256, VEC = 8;
    constexpr int SUB = 528;                       // elements per 16-column sub-tile (32 k rows x 16 + pad)
    constexpr int YS = (TN / 16) * SUB, XS = (TK / 16) * SUB;
    constexpr int NT = 4, MT = 4;

    __shared__ __attribute__((aligned(16))) T smem[2 * (YS + XS)];
    auto Ys = [&](int buf) -> T* { return smem + buf * (YS + XS); };
    auto Xs = [&](int buf) -> T* { return smem + buf * (YS + XS) + YS; };

    const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
    const int ntile = a.nblk_k;                    // one n tile
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, blk_k = logical - split * ntile;
    const int kc0 = blk_k * TK;

    const T* __restrict__ X = static_cast<const T*>(a.x);
    const T* __restrict__ DY = static_cast<const T*>(a.dy);

    // dy: 32 rows x 8 vectors = one 16-byte load per thread; x: 32 rows x 32 vectors = four per thread
    const int yv = tid & 7, yrow = tid >> 3;
    const int yn = yv * VEC;
    const bool yn_ok = yn < a.N;
    const int xv = tid & 31, xrow0 = tid >> 5;      // rows xrow0 + 8 j
    const int kc = kc0 + xv * VEC;
    const bool kc_ok = kc < a.Ktot;
    const uint32_t tap = fdiv((uint32_t)(kc_ok ? kc : 0), a.div_c);
    const int xc = (kc_ok ? kc : 0) - (int)tap * a.C;
    const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
    const int dyo = tr * a.dil - a.pad, dxo = ts * a.dil - a.pad;

    const int tile_beg = split * a.slab_tiles;
    const int tiles_total = (a.M + BK - 1) / BK;
    const int tile_end = min(tiles_total, tile_beg + a.slab_tiles);
    const bool lin1x1 = a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0;

    uint4 y_reg, x_reg[4];
    auto load_tiles = [&](int t) {
        {
            const int m = t * BK + yrow;
            y_reg = make_uint4(0, 0, 0, 0);
            if (m < a.M && yn_ok) y_reg = *reinterpret_cast<const uint4*>(DY + (int64_t)m * a.ldy + yn);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = t * BK + xrow0 + j * 8;
            uint4 xv4 = make_uint4(0, 0, 0, 0);
            if (m < a.M && kc_ok) {
                if (lin1x1) {
                    xv4 = *reinterpret_cast<const uint4*>(X + (int64_t)m * a.ldx + xc);
                } else {
                    const uint32_t b = fdiv((uint32_t)m, a.div_howo);
                    const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
                    const uint32_t yo = fdiv(rem, a.div_wo);
                    const uint32_t xo = rem - yo * (uint32_t)a.Wo;
                    const int ys = (int)yo * a.stride + dyo, xs = (int)xo * a.stride + dxo;
                    if ((unsigned)ys < (unsigned)a.Hi && (unsigned)xs < (unsigned)a.Wi)
                        xv4 = *reinterpret_cast<const uint4*>(X + ((int64_t)((int)b * a.Hi + ys) * a.Wi + xs) * a.ldx + xc);
                }
            }
            x_reg[j] = xv4;
        }
    };
    // sub-tile image [col/16][k'][16], k rows stored with bits 2/3 swapped (conflict-free for the transpose reads and
    // for these 16-byte writes) -- as in conv_wgrad_kernel
    auto row_pos = [](int row) { return (row & 0x13) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 3); };
    auto store_tiles = [&](int buf) {
        *reinterpret_cast<uint4*>(Ys(buf) + (yv >> 1) * SUB + row_pos(yrow) * 16 + (yv & 1) * 8) = y_reg;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<uint4*>(Xs(buf) + (xv >> 1) * SUB + row_pos(xrow0 + j * 8) * 16 + (xv & 1) * 8) = x_reg[j];
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (tile_beg < tile_end) {
        load_tiles(tile_beg);
        store_tiles(0);
    }
    __syncthreads();

    const int lr = lane & 15, lq = lane >> 4;
    const int p_lo = ((lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4)) * 16 + (lr & 3) * 4;
    const int p_hi = p_lo + 8 * 16;
    int cur = 0;
    for (int t = tile_beg; t < tile_end; ++t) {
        const bool has_next = t + 1 < tile_end;
        if (has_next) load_tiles(t + 1);
        const T* ys = Ys(cur);
        const T* xs = Xs(cur) + wk * 4 * SUB;
        mfma_bf16x8 af[NT], bfr[MT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const bf16x4 lo = lds_tr16_b64(ys + i * SUB + p_lo);
            const bf16x4 hi = lds_tr16_b64(ys + i * SUB + p_hi);
            bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            af[i] = __builtin_bit_cast(mfma_bf16x8, v);
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const bf16x4 lo = lds_tr16_b64(xs + j * SUB + p_lo);
            const bf16x4 hi = lds_tr16_b64(xs + j * SUB + p_hi);
            bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            bfr[j] = __builtin_bit_cast(mfma_bf16x8, v);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        if (has_next) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // acc[i][j][q] = dw[n = i*16 + lq*4 + q][kc = kc0 + wk*64 + j*16 + lr]
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = i * 16 + lq * 4 + q;
            if (n >= a.N) continue;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int k = kc0 + wk * 64 + j * 16 + lr;
                if (k < a.Ktot) {
                    if (a.ws != nullptr)
                        a.ws[((int64_t)split * a.N + n) * a.Ktot + k] = acc[i][j][q];
                    else
                        atomicAdd(a.dw + (int64_t)n * a.Ktot + k, acc[i][j][q]);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient, large tile: 256 (n) x 256 (kc) per 512-thread workgroup, 8 waves as 2 (n) x 4 (kc), wave
// tile 128 x 64 = 32 MFMAs per 32-pixel K step.  Why: the 128 x 128 kernel moves 16 KB through the CU's vector
// memory pipeline (64 B/clk) and 48 KB through LDS per 64 MFMAs -- both as busy as the matrix cores, so none of
// them gets past ~50 %; this tile halves both per MFMA.  One workgroup per CU; split-K over pixel slabs sized so
// that the grid is a multiple of the CU count.  Same LDS image as conv_wgrad_kernel (16-column sub-tiles read with
// ds_read_b64_tr_b16); the x fragment is the MFMA row operand here, so a lane ends up with 4 consecutive kc of
// one n and the split-K slab is written with 16-byte stores.  Operand tiles are written to LDS one K step ahead,
// right after the barrier (one register set, loads for step t+2 re-issued immediately).
// Addressing: buffer loads, 32-bit offsets advanced incrementally; tile edges and padding are out-of-range offsets.
// ------------------------------------------------------------------------------------------------
constexpr int WB_THREADS = 512;
constexpr int WB_SUB = 528;                 // elements per 16-column sub-tile (32 k rows x 16 + pad)
constexpr int WB_OP = 16 * WB_SUB;          // one operand, one stage (256 columns)

// DEPTH = 2: two K steps per barrier -- two register sets and 2 x 2 LDS buffers, so that a load has two K steps to land
// (twice the bytes in flight per CU: 64 KB; the one-workgroup-per-CU kernel is bound by what its 512 threads keep
// outstanding) and the barrier is paid once per 64 MFMAs of a wave.
// `logical`: this workgroup's index among the job's nblk_n * nblk_k * splits workgroups (tiles of one pixel slab adjacent)
template <int DEPTH>
__device__ __forceinline__ void wgrad_big_body(const WgradArgs& a, const uint32_t x_bytes, const uint32_t dy_bytes,
                                               const int logical, bf16_t* smem) {
    typedef bf16_t T;
    constexpr int TILE = 256, VEC = 8, RPP = 16, LD = 2;
    constexpr int NT = 8, MT = 4;                 // wave tile: 8 n-tiles x 4 kc-tiles of 16
    constexpr uint32_t OOB = 0x80000000u;

    auto Ys = [&](int buf, int h) -> T* { return smem + (buf * DEPTH + h) * 2 * WB_OP; };
    auto Xs = [&](int buf, int h) -> T* { return smem + (buf * DEPTH + h) * 2 * WB_OP + WB_OP; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 2, wk = wave & 3;
    const int ntile = a.nblk_n * a.nblk_k;
    const int split = logical / ntile, tile_id = logical - split * ntile;
    const int blk_n = tile_id % a.nblk_n, blk_k = tile_id / a.nblk_n;
    const int n0 = blk_n * TILE, kc0 = blk_k * TILE;

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)dy_bytes, 0x00020000);

    const int vcol = tid & 31, prow = tid >> 5;
    const int kc = kc0 + vcol * VEC;
    const bool kc_ok = kc < a.Ktot;
    const uint32_t tap = fdiv((uint32_t)(kc_ok ? kc : 0), a.div_c);
    const int xc = (kc_ok ? kc : 0) - (int)tap * a.C;
    const int tr = (int)tap / a.S, ts = (int)tap - tr * a.S;
    const int dyo = tr * a.dil - a.pad, dxo = ts * a.dil - a.pad;
    const int yn = n0 + vcol * VEC;
    const bool yn_ok = yn < a.N;

    const int tile_beg = split * a.slab_tiles;
    const int tiles_total = (a.M + BK - 1) / BK;
    const int tile_end = min(tiles_total, tile_beg + a.slab_tiles);
    const bool lin1x1 = a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0;

    // incremental per-row state: rows m = t*32 + prow + 16 j.  Rows past M need no test: their offsets fall
    // beyond the descriptors (dy: m*ldy >= M*ldy; x: image index >= B).
    uint32_t yoff[LD], xoff[LD];
    int px_b[LD], px_y[LD], px_x[LD];             // b*Hi, yo, xo of the general gather
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        const int m = tile_beg * BK + prow + j * RPP;
        yoff[j] = yn_ok ? (uint32_t)((m * a.ldy + yn) * 2) : OOB;
        xoff[j] = kc_ok ? (uint32_t)((m * a.ldx + xc) * 2) : OOB;          // 1x1 stride 1: source pixel = m
        const uint32_t b = fdiv((uint32_t)m, a.div_howo);
        const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
        const uint32_t yo = fdiv(rem, a.div_wo);
        px_b[j] = (int)b * a.Hi;
        px_y[j] = (int)yo;
        px_x[j] = (int)(rem - yo * (uint32_t)a.Wo);
    }
    const uint32_t ystep = (uint32_t)(BK * a.ldy * 2), xstep = (uint32_t)(BK * a.ldx * 2);

    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    uint4 y_reg[DEPTH][LD], x_reg[DEPTH][LD];
    // loads the NEXT tile in sequence into register set h (call once per K step, in tile order)
    auto load_next = [&](const int h) {
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const u32x4_t yv = __builtin_amdgcn_raw_buffer_load_b128(rs_y, (int)yoff[j], 0, 0);
            yoff[j] += ystep;
            uint32_t vo;
            if (lin1x1) {
                vo = xoff[j];
                xoff[j] += xstep;
            } else {
                const int ys = px_y[j] * a.stride + dyo, xs = px_x[j] * a.stride + dxo;
                const bool ok = kc_ok && ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
                const uint32_t pix = __umul24((uint32_t)(px_b[j] + ys), (uint32_t)a.Wi) + (uint32_t)xs;
                vo = ok ? (__umul24(pix, (uint32_t)(a.ldx * 2)) + (uint32_t)(xc * 2)) : OOB;
                px_x[j] += BK;
                while (px_x[j] >= a.Wo) {
                    px_x[j] -= a.Wo;
                    if (++px_y[j] == a.Ho) {
                        px_y[j] = 0;
                        px_b[j] += a.Hi;
                    }
                }
            }
            const u32x4_t xv = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)vo, 0, 0);
            y_reg[h][j] = make_uint4(yv.x, yv.y, yv.z, yv.w);
            x_reg[h][j] = make_uint4(xv.x, xv.y, xv.z, xv.w);
        }
    };
    auto store_tiles = [&](int buf, const int h) {
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const int row = prow + j * RPP;
            // 16-column sub-tiles [col/16][k'][16] (1056-byte pitch), k rows stored with bits 2/3 swapped:
            // conflict-free for ds_read_b64_tr_b16 and for these 16-byte writes
            const int prow_ = (row & 0x13) | (((row >> 3) & 1) << 2) | (((row >> 2) & 1) << 3);
            const int off = (vcol >> 1) * WB_SUB + prow_ * 16 + (vcol & 1) * 8;
            *reinterpret_cast<uint4*>(Ys(buf, h) + off) = y_reg[h][j];
            *reinterpret_cast<uint4*>(Xs(buf, h) + off) = x_reg[h][j];
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int h = 0; h < DEPTH; ++h)
        if (tile_beg + h < tile_end) load_next(h);
#pragma unroll
    for (int h = 0; h < DEPTH; ++h)
        if (tile_beg + h < tile_end) store_tiles(0, h);
#pragma unroll
    for (int h = 0; h < DEPTH; ++h)
        if (tile_beg + DEPTH + h < tile_end) load_next(h);
    __syncthreads();

    const int lr = lane & 15, lq = lane >> 4;
    // k rows 8*lq + (lr>>2) (+8 for the second read) at their swapped positions inside a sub-tile
    const int p_lo = ((lr >> 2) | ((lq & 1) << 2) | ((lq >> 1) << 4)) * 16 + (lr & 3) * 4;
    const int p_hi = p_lo + 8 * 16;
    int cur = 0;
    for (int t = tile_beg; t < tile_end; t += DEPTH) {
#pragma unroll
      for (int h = 0; h < DEPTH; ++h) {
        if (DEPTH > 1 && t + h >= tile_end) break;      // workgroup-uniform
        const T* ys = Ys(cur, h) + wn * 8 * WB_SUB;
        const T* xs = Xs(cur, h) + wk * 4 * WB_SUB;
        mfma_bf16x8 yf[NT], xf[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const bf16x4 lo = lds_tr16_b64(xs + j * WB_SUB + p_lo);
            const bf16x4 hi = lds_tr16_b64(xs + j * WB_SUB + p_hi);
            bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            xf[j] = __builtin_bit_cast(mfma_bf16x8, v);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const bf16x4 lo = lds_tr16_b64(ys + i * WB_SUB + p_lo);
            const bf16x4 hi = lds_tr16_b64(ys + i * WB_SUB + p_hi);
            bf16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            yf[i] = __builtin_bit_cast(mfma_bf16x8, v);
        }
        if (t + h + DEPTH < tile_end) {
            store_tiles(cur ^ 1, h);                            // tile t+h+DEPTH (in registers since the previous round)
            if (t + h + 2 * DEPTH < tile_end) load_next(h);     // tile t+h+2*DEPTH
        }
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int i = 0; i < NT; ++i)
                acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[j], yf[i], acc[j][i], 0, 0, 0);
      }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) asm volatile("" : "+v"(acc[j][i]));

    // acc[j][i][q] = dw[n = n0 + wn*128 + i*16 + lr][kc = kc0 + wk*64 + j*16 + lq*4 + q]
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int n = n0 + wn * 128 + i * 16 + lr;
        if (n >= a.N) continue;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int k = kc0 + wk * 64 + j * 16 + lq * 4;
            if (k >= a.Ktot) continue;            // Ktot is a multiple of 8: whole vectors
            if (a.ws != nullptr) {
                *reinterpret_cast<float4*>(a.ws + ((int64_t)split * a.N + n) * a.Ktot + k) =
                    make_float4(acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) atomicAdd(a.dw + (int64_t)n * a.Ktot + k + q, acc[j][i][q]);
            }
        }
    }
}

template <int DEPTH>
__global__ __launch_bounds__(WB_THREADS) void conv_wgrad_big_kernel(const WgradArgs a, const uint32_t x_bytes,
                                                                    const uint32_t dy_bytes) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * DEPTH * 2 * WB_OP];
    wgrad_big_body<DEPTH>(a, x_bytes, dy_bytes, xcd_remap(blockIdx.x, gridDim.x), smem);
}

// Several weight gradients in ONE launch.  A single 48 x 48 layer has 4-9 output tiles of 256 x 256, so filling 256 CUs
// takes ~28 pixel slabs per tile and every slab is a 256 KB fp32 partial that is written and read again by the fold
// kernel: 64 MB + 64 MB per layer whatever its size (PMC: 11.3 GB per step for a 0.24 GB result).  Weight gradients
// only feed the optimizer, so the plan launches the jobs of consecutive layers together: the same 256 workgroups then
// cover several layers with a few slabs each, and the slab traffic (and the launch count) drops by the group size.
constexpr int WG_MAX_JOBS = 12;
struct WgradGroup {
    int njobs;
    int start[WG_MAX_JOBS + 1];            // first workgroup of each job in the launch
    uint32_t xb[WG_MAX_JOBS], yb[WG_MAX_JOBS];
    WgradArgs job[WG_MAX_JOBS];
};
template <int DEPTH>
__global__ __launch_bounds__(WB_THREADS) void conv_wgrad_group_kernel(const WgradGroup g) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * DEPTH * 2 * WB_OP];
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    int j = 0;
    while (j + 1 < g.njobs && logical >= g.start[j + 1]) ++j;
    wgrad_big_body<DEPTH>(g.job[j], g.xb[j], g.yb[j], logical - g.start[j], smem);
}

// dw[n][rs][c < Cm] += sum_s ws[s * slab_stride][n][rs][c]   (fp32 atomics on the L2 are ~10x more expensive per byte than this)
// A small weight tensor with hundreds of splits stays parallel AND deterministic in two launches: with fold_only, blockIdx.y
// walks chunks of 16 splits and leaves each chunk's sum in the chunk's first slab (every thread reads and writes only its own
// element); the second launch then adds the chunk sums (slab_stride = 16) in order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(float* __restrict__ ws, float* __restrict__ dw, int splits, int64_t NRS,
                                                           int Cm, int Cp, int slab_stride, int fold_only) {
    const int64_t total = NRS * Cm;
    const int64_t plane = NRS * Cp;
    const int s0 = fold_only ? blockIdx.y * 16 : 0, s1 = fold_only ? min(splits, s0 + 16) : splits;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t src = i;
        if (Cm != Cp) {
            const int64_t t = i / Cm;
            src = t * Cp + (i - t * Cm);
        }
        float acc = 0.f;
        #pragma unroll 8
        for (int sidx = s0; sidx < s1; ++sidx) acc += ws[(int64_t)sidx * slab_stride * plane + src];
        if (fold_only) ws[(int64_t)s0 * plane + src] = acc;
        else dw[i] += acc;
    }
}

struct ReduceGroup {
    int njobs;
    const float* ws[WG_MAX_JOBS];
    float* dw[WG_MAX_JOBS];
    int splits[WG_MAX_JOBS], Cm[WG_MAX_JOBS], Cp[WG_MAX_JOBS];
    int64_t NRS[WG_MAX_JOBS];
};
// blockIdx.y = job: dw_j[n][rs][c < Cm] += sum_s ws_j[s][n][rs][c]
__global__ __launch_bounds__(256) void wgrad_reduce_group_kernel(const ReduceGroup g) {
    const int j = blockIdx.y;
    const float* __restrict__ ws = g.ws[j];
    float* __restrict__ dw = g.dw[j];
    const int Cm = g.Cm[j], Cp = g.Cp[j], splits = g.splits[j];
    const int64_t total = g.NRS[j] * Cm, plane = g.NRS[j] * Cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t src = i;
        if (Cm != Cp) {
            const int64_t t = i / Cm;
            src = t * Cp + (i - t * Cm);
        }
        float acc = 0.f;
#pragma unroll 4
        for (int sidx = 0; sidx < splits; ++sidx) acc += ws[sidx * plane + src];
        dw[i] += acc;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side.  Which kernel takes a descriptor, with which tiling and grid, is decided in conv_choice.h (pure host code, testable
// without a GPU); here the kernel arguments are filled from the descriptor plus that choice, and one switch launches.
// ------------------------------------------------------------------------------------------------
static_assert(cc::BK == BK && cc::NTHREADS == NTHREADS && cc::WS_MT == WS_MT && cc::WS_STAT_ROWS == WS_STAT_ROWS &&
                  cc::WS_NLD == WS_PLANES_NLD && cc::WB_THREADS == WB_THREADS && cc::WGW_TN == WGW_TN && cc::WGW_TK == WGW_TK &&
                  cc::WGW_NLD == WGW_NLD && cc::WG_MAX_JOBS == WG_MAX_JOBS,
              "conv_choice.h describes the kernels of this file");

// The kernel arguments of a launch: every field of the descriptor that is in effect, the rest zero, and the chosen tiling.
static ConvArgs conv_args(const DmlConvDesc* d, const cc::ConvChoice& c) {
    ConvArgs a{};
    a.x = d->x; a.w = d->w; a.y = d->y; a.bias = d->bias; a.stats = d->stats;
    a.B = d->B; a.Hi = d->Hi; a.Wi = d->Wi; a.C = d->C; a.ldx = d->ldx;
    a.Ho = d->Ho; a.Wo = d->Wo; a.N = d->N; a.ldy = d->ldy;
    a.R = d->R; a.S = d->S; a.stride = d->stride; a.dil = d->dil; a.pad = d->pad; a.pad_x = cc::conv_pad_x(*d);
    a.M = cc::conv_m(*d);
    a.Ktot = cc::conv_ktot(*d);
    a.y_f32 = d->y_f32; a.accum = d->accum;
    a.nblk_m = c.nblk_m; a.nblk_n = c.nblk_n;
    a.div_wo = make_fastdiv((uint32_t)d->Wo);
    a.div_howo = make_fastdiv((uint32_t)(d->Ho * d->Wo));
    a.div_c = make_fastdiv((uint32_t)d->C);
    a.x_bytes = c.x_bytes; a.w_bytes = c.w_bytes;
    a.w_tiled = d->w_tiled ? 1 : 0;
    a.f32_split = cc::conv_f32_split(*d);
    if (cc::conv_has_planes(*d)) {
        a.x_planes = d->x_planes; a.w_planes = d->w_planes; a.x_unscale = d->x_unscale; a.w_unscale = d->w_unscale;
        a.x_plane_bytes = (uint32_t)(d->x_plane_stride * 2); a.w_plane_bytes = (uint32_t)(d->w_plane_stride * 2);
    }
    if (d->acc32) { a.acc32 = d->acc32; a.acc32_ld = d->acc32_ld; }
    if (d->res_dz) { a.res_dz = d->res_dz; a.res_mask = d->res_mask; a.res_ld = d->res_ld; }
    a.tail_full = c.tail_full; a.tail_q = c.tail_q;
    // ws_min_tiles, tail_ws_elems_, tail_cnt_len_: read by nobody (conv_choice.h looks at the descriptor); set so that the argument block
    // of a launch holds defined values in every member
    a.ws_min_tiles = d->ws_min_tiles;
    if (cc::conv_has_tail(*d)) {
        a.tail_ws = d->tail_ws; a.tail_cnt = d->tail_counters;
        a.tail_ws_elems_ = d->tail_ws_elems; a.tail_cnt_len_ = d->tail_counters_len;
    }
    if (d->post_scale) {
        a.post_scale = d->post_scale; a.post_shift = d->post_shift; a.post_mean = d->post_mean; a.post_res = d->post_res;
        a.post_ldres = d->post_ldres; a.post_relu = d->post_relu;
    }
    if (d->bnr_partials) {
        a.bnr_y = d->bnr_y; a.bnr_mask = d->bnr_mask; a.bnr_mean = d->bnr_mean; a.bnr_invstd = d->bnr_invstd;
        a.bnr_partials = d->bnr_partials; a.bnr_ldy = d->bnr_ldy; a.bnr_relu = d->bnr_relu;
        if (d->dtype == DML_F32) a.bnr_gmax = d->bnr_gmax;
        a.bnr_inc = d->bnr_inc != 0 ? 1 : 0;
    }
    a.nt_out = c.nt_out;
    if (d->sub_grid) { a.sub_grid = 1; a.sub_y = d->sub_y; a.sub_x = d->sub_x; }
    return a;
}

template <typename T, int MODE>
void launch_conv(const cc::ConvChoice& c, const ConvArgs& a, hipStream_t st) {
    const dim3 grid(c.grid), block(c.block);
    switch (c.family) {
    case cc::CONV_RING:
        if constexpr (sizeof(T) == 2) {
            if (c.bm == 256)
                hipLaunchKernelGGL((conv_igemm_dma_kernel<128, MODE, 3, 2, 256, 128>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
            else if (c.bn == 128)
                hipLaunchKernelGGL((conv_igemm_dma_kernel<128, MODE, 3>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
            else
                hipLaunchKernelGGL((conv_igemm_dma_kernel<64, MODE, 3>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
        }
        break;
    case cc::CONV_X3:
        if constexpr (sizeof(T) == 4 && MODE != 2) {
            if (c.bn == 128) hipLaunchKernelGGL((conv_igemm_x3_kernel<128, MODE>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((conv_igemm_x3_kernel<64, MODE>), grid, block, 0, st, a);
        }
        break;
    default:
        if constexpr (MODE != 2) {
            if (c.aligned) {
                if (c.bn == 128) hipLaunchKernelGGL((conv_igemm_kernel<T, 128, true, MODE>), grid, block, 0, st, a);
                else if (c.bn == 64) hipLaunchKernelGGL((conv_igemm_kernel<T, 64, true, MODE>), grid, block, 0, st, a);
                else hipLaunchKernelGGL((conv_igemm_kernel<T, 32, true, MODE>), grid, block, 0, st, a);
            } else {
                if (c.bn == 128) hipLaunchKernelGGL((conv_igemm_kernel<T, 128, false, MODE>), grid, block, 0, st, a);
                else if (c.bn == 64) hipLaunchKernelGGL((conv_igemm_kernel<T, 64, false, MODE>), grid, block, 0, st, a);
                else hipLaunchKernelGGL((conv_igemm_kernel<T, 32, false, MODE>), grid, block, 0, st, a);
            }
        }
        break;
    }
}

// everything of WgradArgs but the tiling (nblk_n, nblk_k, slab_tiles) and the workspace
static void fill_wgrad_args(WgradArgs& a, const DmlWgradDesc* d, const bool planes) {
    a.x = d->x; a.dy = d->dy; a.dw = d->dw;
    a.B = d->B; a.Hi = d->Hi; a.Wi = d->Wi; a.C = d->C; a.ldx = d->ldx;
    a.Ho = d->Ho; a.Wo = d->Wo; a.N = d->N; a.ldy = d->ldy;
    a.R = d->R; a.S = d->S; a.stride = d->stride; a.dil = d->dil; a.pad = d->pad;
    a.M = d->B * d->Ho * d->Wo;
    a.Ktot = d->R * d->S * d->C;
    a.div_wo = make_fastdiv((uint32_t)d->Wo);
    a.div_howo = make_fastdiv((uint32_t)(d->Ho * d->Wo));
    a.div_c = make_fastdiv((uint32_t)d->C);
    a.x_planes = planes ? d->x_planes : nullptr; a.dy_planes = planes ? d->dy_planes : nullptr;
    a.x_unscale = planes ? d->x_unscale : nullptr; a.dy_unscale = planes ? d->dy_unscale : nullptr;
    a.x_plane_bytes = planes ? (uint32_t)(d->x_plane_stride * 2) : 0u;
    a.dy_plane_bytes = planes ? (uint32_t)(d->dy_plane_stride * 2) : 0u;
}

}  // namespace

// Rows of the GEMM covered by one statistics partial (DmlConvDesc.stats / bnr_partials) of THIS launch: 48 where the
// wave-specialised kernel takes it, DML_STAT_ROWS otherwise.  The caller sizes the partial buffers with it and passes it on to
// dml_bn_finalize_rows / dml_bn_moments_rows (the BN-backward finalize only needs the group count).
extern "C" int dml_conv_stat_rows(const DmlConvDesc* d) {
    cc::ConvChoice c;
    cc::conv_choose(d, conv_switches(), &c);
    return c.stat_rows;
}

extern "C" int dml_conv_igemm(const DmlConvDesc* d, void* stream) {
    cc::ConvChoice c;
    const int rc = cc::conv_choose(d, conv_switches(), &c);
    if (rc) return rc;
    const ConvArgs a = conv_args(d, c);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c.family == cc::CONV_WS) {
        launch_conv_ws(c, a, st);
    } else if (c.elem_bytes == 2) {
        if (c.mode == 2) launch_conv<bf16_t, 2>(c, a, st);
        else if (c.mode == 1) launch_conv<bf16_t, 1>(c, a, st);
        else launch_conv<bf16_t, 0>(c, a, st);
    } else {
        if (c.mode == 1) launch_conv<float, 1>(c, a, st);
        else launch_conv<float, 0>(c, a, st);
    }
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_conv_wgrad(const DmlWgradDesc* d, void* stream) {
    cc::WgradChoice c;
    const int rc = cc::wgrad_choose(d, &c);
    if (rc) return rc;
    WgradArgs a;
    fill_wgrad_args(a, d, c.planes);
    a.nblk_n = c.nblk_n; a.nblk_k = c.nblk_k; a.slab_tiles = c.slab_tiles;
    a.ws = c.use_ws ? d->ws : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(c.grid), block(c.block);
    switch (c.family) {
    case cc::WGRAD_BIG:
        hipLaunchKernelGGL(conv_wgrad_big_kernel<WGRAD_DEPTH>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes);
        break;
    case cc::WGRAD_WS:
        if (c.lin) hipLaunchKernelGGL(conv_wgrad_ws_kernel<true>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes, c.nitems);
        else hipLaunchKernelGGL(conv_wgrad_ws_kernel<false>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes, c.nitems);
        break;
    case cc::WGRAD_H2:
        if (c.lin) hipLaunchKernelGGL(conv_wgrad_h2_kernel<true>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes);
        else hipLaunchKernelGGL(conv_wgrad_h2_kernel<false>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes);
        break;
    case cc::WGRAD_N64:
        hipLaunchKernelGGL(conv_wgrad_n64_kernel, grid, block, 0, st, a);
        break;
    case cc::WGRAD_X3:
        if (c.lin) hipLaunchKernelGGL(conv_wgrad_x3_kernel<true>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes);
        else hipLaunchKernelGGL(conv_wgrad_x3_kernel<false>, grid, block, 0, st, a, c.x_bytes, c.dy_bytes);
        break;
    default:
        if (c.elem_bytes == 2) hipLaunchKernelGGL(conv_wgrad_kernel<bf16_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(conv_wgrad_kernel<float>, grid, block, 0, st, a);
        break;
    }
    for (int i = 0; i < c.nreduce; ++i) {
        const cc::ReduceLaunch& r = c.reduce[i];
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(r.grid_x, r.grid_y), dim3(r.block), 0, st, d->ws, d->dw, r.splits, c.nrs, c.cm, d->C,
                           r.slab_stride, r.fold_only);
    }
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_conv_wgrad_group_eligible(const DmlWgradDesc* d) { return cc::wgrad_big_eligible(d, true) ? 1 : 0; }

// Weight gradients of several layers in one launch (conv_wgrad_group_kernel) + one fold launch.  Every job must pass
// dml_conv_wgrad_group_eligible; the descriptors' own ws / ws_elems / splitk fields are ignored: the shared workspace
// `ws` is partitioned by wgrad_group_choose.
extern "C" int dml_conv_wgrad_group(const DmlWgradDesc* const* descs, int n, float* ws, int64_t ws_elems, void* stream) {
    cc::WgradGroupChoice c;
    const int rc = cc::wgrad_group_choose(descs, n, ws, ws_elems, &c);
    if (rc) return rc;
    WgradGroup g;
    ReduceGroup r;
    g.njobs = r.njobs = n;
    g.start[0] = 0;
    for (int j = 0; j < n; ++j) {
        const DmlWgradDesc* d = descs[j];
        WgradArgs& a = g.job[j];
        fill_wgrad_args(a, d, false);
        a.nblk_n = c.nblk_n[j]; a.nblk_k = c.nblk_k[j]; a.slab_tiles = c.slab_tiles[j];
        a.ws = ws + c.ws_off[j];
        g.xb[j] = c.x_bytes[j]; g.yb[j] = c.dy_bytes[j];
        g.start[j + 1] = c.start[j + 1];
        r.ws[j] = a.ws; r.dw[j] = d->dw; r.splits[j] = c.splitk[j]; r.Cm[j] = c.cm[j]; r.Cp[j] = d->C;
        r.NRS[j] = c.nrs[j];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(conv_wgrad_group_kernel<WGRAD_DEPTH>, dim3(c.grid), dim3(c.block), 0, st, g);
    hipLaunchKernelGGL(wgrad_reduce_group_kernel, dim3(c.rgrid_x, c.rgrid_y), dim3(c.rblock), 0, st, r);
    DML_LAUNCH_CHECK();
    return 0;
}
