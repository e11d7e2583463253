// Implicit-GEMM convolution on MFMA for gfx950 (MI355X): the WAVE-SPECIALISED forward / data-gradient kernel with its row epilogues.
// One kernel template, compiled in two translation units because its instantiations are the slowest code of the library to build:
// conv_ws.hip instantiates the one-plane (bf16) launches and the two-plane forward, conv_ws_dgrad.hip the two-plane data gradients.
// conv_igemm.hip has the overview and the host side, conv_device.h the shared epilogue and the LDS-DMA helpers.
#pragma once
#include "conv_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// bf16 forward / data-gradient kernel, WAVE-SPECIALISED version (round 4; tools/probe_ws_gemm.hip is its GEMM-only probe,
// profiles/r04_ws_probe_*.txt the measurements behind every choice below).
// What bounded the ring kernel (conv_igemm.hip): every wave both issues its share of the K step's buffer_load ... lds instructions and
// consumes the step -- a wave issues in order, so the 84-170 cycles the texture addresser takes to accept each of its four
// DMA instructions are cycles in which it issues no MFMA, and three co-resident workgroups only partly fill the holes
// (profiles/r03_dma_phases.txt).  Here the two jobs belong to different waves of one workgroup per CU:
//   * NLD LOADER waves own the vector-memory path.  Loader l issues pieces l, l + NLD, ... (1 KB = 16 tile rows x 64 B each)
//     of every K step into an NST-stage LDS ring, keeps D stages in flight behind the one it publishes (counted vmcnt) and
//     announces "stage landed" through a counter in LDS.  A single wave gets one DMA instruction accepted per ~100 cycles,
//     the addresser takes one per ~30 from several waves: three to four loaders saturate it (1 loader 455, 2: 906, 3: 997
//     TFLOP/s on layer3's 3x3).  The DMA instruction is inline asm: hipcc must not see an LDS-DMA in flight, or it drains
//     vmcnt(0) before each of the loader's own LDS accesses (the flag polls).
//   * 4 CONSUMER waves (one per SIMD) never touch vector memory inside the K loop: poll the counter (the poll for step
//     k + 1 is issued in the middle of step k's MFMAs), read fragments, issue MFMAs back to back.  The fragments of step
//     k + 1 are fetched under the MFMAs of step k, register by register as they become free (A fragment j right after the
//     four MFMAs that used it; the weight fragments and the last A fragment alternate between two register sets).
//   * No s_barrier in the K loop; the ring decouples the two sides.  WAR: a consumer announces "every read of stage g has
//     been ISSUED" (DS executes one wave's operations in order, so the flag write lands after them); a loader overwrites a
//     stage only when all four consumers have announced it.
//   * Tile = (144 MW) x (64 NW) pixels x channels on 144 x 64 WAVE tiles (36 MFMAs per wave and K step against 13 KB of
//     fragment reads; the 64 x 64 wave tile of the ring kernel: 16 against 8 KB).  144 rows because the maps of this network
//     at 16 images are 36 864 / 147 456 / 589 824 pixels: 256 CUs x 144 rows x {1, 4, 16} -- one 144 x 256 tile per CU fills the
//     chip exactly where 128-row tiles leave a quarter of a round (layer3: 576 tiles on 768 slots) and 256 x 256 tiles 44 %
//     of it.  One workgroup per CU; workgroups are persistent and walk the tile list (m fastest: the CUs work on the same
//     weight rows at the same time), the loaders run ahead into the next tile while the consumers store the finished one.
//   * BatchNorm partial statistics / BN-backward partial sums come per 48 rows (three groups per wave tile): the epilogue is
//     conv_epilogue on 48-row sub-tiles, and the finalize kernels take the group height (dml_conv_stat_rows).
// Weights must be the tile-major copy (w_tiled).  MODE as conv_igemm_dma_kernel.
// ------------------------------------------------------------------------------------------------
// fp32 output of a 48 x 64 sub-tile as WHOLE 256-byte rows: straight from the accumulators a store instruction writes, per pixel
// row, four 16-byte pieces 32 bytes apart (the lane's channel runs, frag_chan) -- 16 rows x 4 pieces per instruction, and the
// chip takes a 144 x 256 fp32 tile per CU (37.7 MB per launch) in 14-16 us, every K loop waiting behind it.  Staged through
// 12 KB of LDS (row-major, 16-byte chunk index XOR row: conflict-free both ways) every store instruction -- and every read
// of the accumulate / residual operands -- covers four pixel rows x 256 contiguous bytes: 5-6 us (profiles/r04_h2_epilogue.txt).
// BatchNorm statistics come from the accumulators as before (conv_epilogue, STATS_ONLY); accumulate and the stores happen on the
// row side (launches with a bias or the inference epilogue post_* keep conv_epilogue).  `stage`: this wave's own 12 KB.
// BatchNorm partial statistics of a WHOLE 144 x 64 wave tile of the two-plane forward kernel: (sum, M2 about the tile mean) per channel over
// its 144 rows, from the accumulators, before the row epilogue stores them sub-tile by sub-tile.  Round 6: with 48-row groups the
// cross-lane reductions (a DPP row sum per channel and sub-tile, twice) made the statistics 15-28 % of the short-K 1x1 forward
// launches (tools/bench_h2.py with and without `stats`: 1x1 256 -> 1024 at 48 x 48 94.9 vs 80.1 us, 64 -> 256 at 192 x 192 177.6 vs
// 128.4); per wave tile they are a third as many, and the finalize kernels fold a third of the partial rows.
// acc3[h][i][jj] = rows mw0 + 48 h + 16 jj + (lane & 15), channels nw0 + frag_chan<4>(i, lane >> 4) .. + 3
template <int NT, int NS>
__device__ __forceinline__ void ws_tile_stats(const f32x4 (&acc3)[NS][NT][3], const ConvArgs& a, const int mw0, const int nw0,
                                              const int lr, const int lq) {
    static_assert(NT == 4, "64-channel wave tile");
    constexpr int TM = NS * 48;
    const int cnt = min(TM, max(0, a.M - mw0));
    if (cnt <= 0) return;
    const float inv = 1.0f / (float)cnt;
    float* sg = a.stats + (int64_t)(mw0 / TM) * a.N * 2;
    float S[NT][4], Q[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                const bool v = (mw0 + h * 48 + jj * 16 + lr) < a.M;
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] += v ? acc3[h][i][jj][q] : 0.f;
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = row16_sum(s[q]);
        float m2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                const bool v = (mw0 + h * 48 + jj * 16 + lr) < a.M;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float dlt = acc3[h][i][jj][q] - s[q] * inv;
                    m2[q] += v ? dlt * dlt : 0.f;
                }
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            S[i][q] = s[q];
            Q[i][q] = row16_sum(m2[q]);
        }
    }
    // one store instruction per wave: lane (lq, lr = 2 i + h) writes the (sum, M2) pairs of channels 2 h, 2 h + 1 of tile i (conv_epilogue)
    if (lr < 2 * NT && nw0 + NT * 16 <= a.N) {
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

template <int NT, int MODE, bool OPS = true>      // OPS = false: launches with epilogue operands go to conv_epilogue_rows_ops
__device__ __forceinline__ void conv_epilogue_rows(f32x4 (&acc)[NT][3], const ConvArgs& a, const int mw0, const int nw0,
                                                   const int lane, char* stage, char* mstage, const bool do_stats = true) {
    static_assert(NT == 4, "64-channel wave tile");
    const int lr = lane & 15, lq = lane >> 4;
    if (MODE == 0 && a.stats != nullptr && do_stats) conv_epilogue<float, NT, 3, MODE, false, true>(acc, a, mw0, nw0, lr, lq);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int row = j * 16 + lr, chunk = frag_chan<NT>(i, lq) >> 2;
            *reinterpret_cast<f32x4*>(stage + row * 256 + ((chunk ^ (row & 15)) << 4)) = acc[i][j];
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the wave's own writes, read back by other lanes
    const int c0 = nw0 + (lane & 15) * 4;
    if (c0 >= a.N) return;                                       // (a last, half-empty 128-wide block)
    // the accumulate operand: the gradient's earlier value (accum), or the identity branch's share of it -- the block output's
    // gradient res_dz under its ReLU mask (DmlConvDesc.res_*, one mask byte per four channels)
    const bool resm = OPS && MODE == 1 && a.res_dz != nullptr;
    const bool has_old = OPS && (a.accum != 0 || resm);
    const bool bnr = OPS && MODE == 1 && a.bnr_partials != nullptr;
    float* const yb = static_cast<float*>(a.y);
    if (!OPS || (!has_old && !bnr)) {
        // all twelve LDS reads first (into the registers the sub-tile's accumulators just left), then twelve stores back to back.
        // (One path with the accumulate operand selected per element made every store wait vmcnt(0) -- stores count there too on
        // gfx950 -- i.e. for the store before it: 36 serialised round trips per tile, as slow as the scattered stores this function
        // replaces; hence separate code paths on wave-uniform branches.)
        float4 o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int r = k * 4 + (lane >> 4);
            o[k] = *reinterpret_cast<const float4*>(stage + r * 256 + (((lane & 15) ^ (r & 15)) << 4));
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int m = mw0 + k * 4 + (lane >> 4);
            if (m < a.M) st16f(yb + (int64_t)(MODE == 1 ? ws_out_row(a, (uint32_t)m) : (uint32_t)m) * a.ldy + c0, o[k].x, o[k].y, o[k].z, o[k].w,
                               (a.nt_out & 1) != 0);
        }
        return;
    }
    // With an accumulate operand (the gradient has earlier producers) and / or the BatchNorm-backward sums of the tensor being
    // written (DmlConvDesc.bnr_*: sum g, sum g * xhat per 48 rows and channel, g = dz * [ReLU mask bit] -- what dml_bn_bwd_reduce
    // would compute from the stored tensor, without its pass over dz and y): groups of four rows, the operand loads of the NEXT
    // group issued before this group's stores, so that waiting for them does not wait for the stores.
    auto body = [&](auto ho, auto bn) {
        constexpr bool HO = decltype(ho)::value, BNR = decltype(bn)::value;
        float4 old[2][4], yv[2][4];
        float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1, mu = r1, is = r1;
        uint32_t gmx = 0;
        if (BNR) {
            mu = *reinterpret_cast<const float4*>(a.bnr_mean + c0);
            is = *reinterpret_cast<const float4*>(a.bnr_invstd + c0);
        }
        // ReLU masks of the sub-tile (one byte per four channels, low nibble): lane L < 48 fetches row L's 16 mask bytes -- this wave's
        // 64 channels -- of each mask with ONE 16-byte load, packs them (identity-branch mask: low nibble, BatchNorm mask: high
        // nibble) and parks the 768 bytes in the wave's mask area behind the ring; the row loop reads its byte back.  Per-lane byte
        // loads were one VMEM instruction per mask and four rows -- 24 of the ~60 of a sub-tile -- and the texture addresser pays
        // per instruction, not per byte.
        const bool use_rm = HO && resm, use_bm = BNR && a.bnr_relu != 0;
        // byte of row (4 c + (lane >> 4)), chunk (lane & 15) = mstage[64 c + lane]: one base, compile-time offsets (computed here, from
        // a lane index the optimiser cannot see through -- hoisted to the head of the kernel the twelve row offsets get spilled, and a
        // scratch reload inside the row loop waits vmcnt(0), i.e. for every store in flight)
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        const char* const mrd = mstage + lane_m;
        if (use_rm || use_bm) {
            if (lane < WS_STAT_ROWS) {
                const int m = mw0 + lane;
                uint4 rv = make_uint4(0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu), bv = rv;
                if (m < a.M) {
                    const int64_t mo = (int64_t)ws_out_row(a, (uint32_t)m) * (a.N >> 2) + (nw0 >> 2);
                    if (use_rm) rv = *reinterpret_cast<const uint4*>(a.res_mask + mo);
                    if (use_bm) bv = *reinterpret_cast<const uint4*>(a.bnr_mask + mo);
                }
                uint4 pk;
                pk.x = (rv.x & 0x0f0f0f0fu) | ((bv.x & 0x0f0f0f0fu) << 4);
                pk.y = (rv.y & 0x0f0f0f0fu) | ((bv.y & 0x0f0f0f0fu) << 4);
                pk.z = (rv.z & 0x0f0f0f0fu) | ((bv.z & 0x0f0f0f0fu) << 4);
                pk.w = (rv.w & 0x0f0f0f0fu) | ((bv.w & 0x0f0f0f0fu) << 4);
                *reinterpret_cast<uint4*>(mstage + lane * 16) = pk;
            }
        }
        auto load_ops = [&](const int g4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int m = mw0 + (g4 * 4 + u) * 4 + (lane >> 4);
                old[g4 & 1][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                yv[g4 & 1][u] = old[g4 & 1][u];
                if (m < a.M) {
                    const int64_t pm = (int64_t)ws_out_row(a, (uint32_t)m);
                    if (HO) {
                        if (resm) old[g4 & 1][u] = *reinterpret_cast<const float4*>(static_cast<const float*>(a.res_dz) + pm * a.res_ld + c0);
                        else old[g4 & 1][u] = *reinterpret_cast<const float4*>(yb + pm * a.ldy + c0);
                    }
                    if (BNR) yv[g4 & 1][u] = *reinterpret_cast<const float4*>(static_cast<const float*>(a.bnr_y) + pm * a.bnr_ldy + c0);
                }
            }
        };
        load_ops(0);
#pragma unroll
        for (int g4 = 0; g4 < 3; ++g4) {
            if (g4 + 1 < 3) load_ops(g4 + 1);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = (g4 * 4 + u) * 4 + (lane >> 4), m = mw0 + r;
                if (m >= a.M) continue;
                float4 o = *reinterpret_cast<const float4*>(stage + r * 256 + (((lane & 15) ^ (r & 15)) << 4));
                uint32_t pkb = 0xffu;
                if (use_rm || use_bm) pkb = *reinterpret_cast<const uint8_t*>(mrd + (g4 * 4 + u) * 64);
                if (HO) {
                    float4 t = old[g4 & 1][u];
                    if (resm) {
                        t.x = (pkb & 1u) ? t.x : 0.f; t.y = (pkb & 2u) ? t.y : 0.f; t.z = (pkb & 4u) ? t.z : 0.f; t.w = (pkb & 8u) ? t.w : 0.f;
                    }
                    o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
                }
                st16f(yb + (int64_t)ws_out_row(a, (uint32_t)m) * a.ldy + c0, o.x, o.y, o.z, o.w, (a.nt_out & 1) != 0);
                if (BNR) {
                    const uint32_t bits = pkb >> 4;
                    const float4 y4 = yv[g4 & 1][u];
                    const float g0 = (bits & 1u) ? o.x : 0.f, g1 = (bits & 2u) ? o.y : 0.f, g2 = (bits & 4u) ? o.z : 0.f,
                                g3 = (bits & 8u) ? o.w : 0.f;
                    r1.x += g0; r1.y += g1; r1.z += g2; r1.w += g3;
                    r2.x += g0 * (y4.x - mu.x) * is.x; r2.y += g1 * (y4.y - mu.y) * is.y;
                    r2.z += g2 * (y4.z - mu.z) * is.z; r2.w += g3 * (y4.w - mu.w) * is.w;
                    gmx = max(max(gmx, __float_as_uint(g0) & 0x7fffffffu), max(__float_as_uint(g1) & 0x7fffffffu,
                              max(__float_as_uint(g2) & 0x7fffffffu, __float_as_uint(g3) & 0x7fffffffu)));
                }
            }
        }
        if (BNR) {
            // the four lane groups (lane >> 4) hold the same four channels: fold, then lanes 0 .. 15 write their channels' pairs
            float v[8] = {r1.x, r2.x, r1.y, r2.y, r1.z, r2.z, r1.w, r2.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] += __shfl_xor(v[e], 16, 64);
                v[e] += __shfl_xor(v[e], 32, 64);
            }
            if (lane < 16 && mw0 < a.M) {
                float* pp = a.bnr_partials + ((int64_t)(mw0 / WS_STAT_ROWS) * a.N + c0) * 2;
                st16f(pp, v[0], v[1], v[2], v[3], false);
                st16f(pp + 4, v[4], v[5], v[6], v[7], false);
            }
            if (a.bnr_gmax != nullptr) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) gmx = max(gmx, (uint32_t)__shfl_xor((int)gmx, o, 64));
                if (lane == 0 && gmx != 0)
                    atomicMax(reinterpret_cast<uint32_t*>(a.bnr_gmax) + ((blockIdx.x * 16u + (uint32_t)(mw0 / WS_STAT_ROWS) + (uint32_t)(nw0 >> 6)) & 1023u), gmx);
            }
        }
    };
    if constexpr (OPS) {
        if (bnr) {
            if (has_old) body(std::true_type{}, std::true_type{});
            else body(std::false_type{}, std::true_type{});
        } else {
            body(std::true_type{}, std::false_type{});
        }
    }
}

// conv_epilogue_rows for a WHOLE wave tile (NS 48-row sub-tiles) of a data gradient WITH epilogue operands (identity-branch gradient /
// accumulate, fused BatchNorm-backward sums): one software pipeline over all 12 NS row quads instead of one per sub-tile.  The operand
// loads of a launch like the data gradient of 1x1 1024 -> 256 (dz and y in, dx out: 490 MB) ran at 4 TB/s = the bytes a CU had in
// flight (two groups of four row quads per wave) over the loaded HBM latency, and every sub-tile began with an exposed round trip
// (its masks and its first group).  Here every row quad has its own operand registers (a ring of 12, indices compile-time in the
// unrolled quad loop), the loads run WS_EPI_P quads ahead ACROSS the sub-tile boundaries of the rolled sub-tile loop, and the masks
// of sub-tile h + 1 are fetched during sub-tile h.
constexpr int WS_EPI_P = 8;
template <int I, int N, class F>
__device__ __forceinline__ void ws_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ws_static_for<I + 1, N>(f);
    }
}
template <int NT, int NS, bool HO, bool BNR>
__device__ __forceinline__ void conv_epilogue_rows_ops(f32x4 (&acc3)[NS][NT][3], const ConvArgs& a, const int mwt, const int nw0,
                                                       const int lane_in, char* stage0, char* stage1, char* mstage) {
    static_assert(NT == 4, "64-channel wave tile");
    constexpr int P = WS_EPI_P;
    static_assert(P >= 1 && P <= 11, "ring of 12 row quads");
    typedef unsigned int u32x4_b __attribute__((ext_vector_type(4)));
    constexpr uint32_t OOB = 0x80000000u;
    // (a lane index the optimiser cannot see through: hoisted out of the tile loop, the per-quad addresses below get spilled)
    int lane = lane_in;
    asm volatile("" : "+v"(lane));
    // Every global access of the quad loop is a BUFFER access with the tensor's byte size as range: rows beyond M read zeros and
    // their stores are dropped by the address unit, an access that must not happen gets an offset 2^31 bytes further (all these
    // tensors are below 2^31 bytes, conv_ws_planes_eligible).  No branch around any memory instruction, so the loop is straight-line
    // code whose vmcnt waits the compiler counts exactly; under `if (m < M)` / `if (h + 1 < NS)` branches it must assume the
    // fewest instructions behind a load and ends up draining the queue.
    const int c0 = nw0 + (lane & 15) * 4;
    const uint32_t coff = c0 < a.N ? (uint32_t)c0 * 4u : OOB;
    const bool resm = a.res_dz != nullptr;
    const uint32_t y_row = (uint32_t)a.ldy * 4u;
    const uint32_t o_row = resm ? (uint32_t)a.res_ld * 4u : y_row, b_row = (uint32_t)a.bnr_ldy * 4u, m_row = (uint32_t)(a.N >> 2);
    const bool use_rm = HO && resm, use_bm = BNR && a.bnr_relu != 0;
    // (sub_grid: the launch's rows are a parity class of tensors with four times as many pixels, ws_out_row; a row beyond M maps
    // beyond every range)
    const uint32_t prow_n = ws_out_rows(a);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)(prow_n * y_row), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(
        resm ? const_cast<void*>(a.res_dz) : a.y, 0, HO ? (int)(prow_n * o_row) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(
        BNR ? const_cast<void*>(static_cast<const void*>(a.bnr_y)) : a.y, 0, BNR ? (int)(prow_n * b_row) : 0, 0x00020000);
    // (a mask that is not in use: a zero-sized range -- the loads return zeros without touching memory -- and constant bits instead)
    const __amdgpu_buffer_rsrc_t rs_rm = __builtin_amdgcn_make_buffer_rsrc(
        use_rm ? const_cast<void*>(static_cast<const void*>(a.res_mask)) : a.y, 0, use_rm ? (int)(prow_n * m_row) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_bm = __builtin_amdgcn_make_buffer_rsrc(
        use_bm ? const_cast<void*>(static_cast<const void*>(a.bnr_mask)) : a.y, 0, use_bm ? (int)(prow_n * m_row) : 0, 0x00020000);
    const int ngroups = (a.M + WS_STAT_ROWS - 1) / WS_STAT_ROWS;
    const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc(
        BNR ? static_cast<void*>(a.bnr_partials) : a.y, 0, BNR ? (int)((uint32_t)ngroups * (uint32_t)a.N * 8u) : 0, 0x00020000);
    const uint32_t nomask = use_bm ? 0u : 0xfu;
    u32x4_b old[12], yv[12];
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu;
    if (BNR && c0 < a.N) {
        mu = *reinterpret_cast<const float4*>(a.bnr_mean + c0);
        is = *reinterpret_cast<const float4*>(a.bnr_invstd + c0);
    }
    // ReLU masks of a sub-tile: lane L fetches row L's 16 mask bytes (this wave's 64 channels) of each mask; lanes < 48 park them,
    // packed (identity-branch mask: low nibble, BatchNorm mask: high nibble), in the wave's mask area (as conv_epilogue_rows);
    // the masks of sub-tile h + 1 are fetched during sub-tile h
    u32x4_b rv, bv;
    auto load_masks = [&](const int h) {
        const uint32_t mo = ws_out_row(a, (uint32_t)(mwt + h * WS_STAT_ROWS + lane)) * m_row + (uint32_t)(nw0 >> 2);
        rv = __builtin_amdgcn_raw_buffer_load_b128(rs_rm, mo, 0, 0);
        bv = __builtin_amdgcn_raw_buffer_load_b128(rs_bm, mo, 0, 0);
    };
    // operands of row quad Q of the wave tile (rows mwt + 4 Q + (lane >> 4)) into its ring slot
    auto load_quad = [&](auto Qc) {
        constexpr int Q = decltype(Qc)::value, slot = Q % 12;
        if constexpr (Q < 12 * NS) {
            const uint32_t m = ws_out_row(a, (uint32_t)(mwt + Q * 4 + (lane >> 4)));
            if (HO) old[slot] = __builtin_amdgcn_raw_buffer_load_b128(rs_o, m * o_row + coff, 0, 0);
            if (BNR) yv[slot] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, m * b_row + coff, 0, 0);
        }
    };
    // accumulators -> LDS rows: sub-tiles 0 and 1 at once (two staging areas: the slots of the tile's last TWO K stages), sub-tile 2
    // into area 0 when sub-tile 0 has been read -- 48 accumulator registers live under the operand ring instead of 96
    auto stage_acc = [&](f32x4 (&sub)[NT][3], char* st) {
        const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int row = j * 16 + lr, chunk = frag_chan<NT>(i, lq) >> 2;
                *reinterpret_cast<f32x4*>(st + row * 256 + ((chunk ^ (row & 15)) << 4)) = sub[i][j];
            }
    };
    stage_acc(acc3[0], stage0);
    if constexpr (NS == 3) stage_acc(acc3[1], stage1);
    __builtin_amdgcn_sched_barrier(0);      // (the ring's first loads after the staging: 96 accumulator registers are free by then)
    load_masks(0);
    ws_static_for<0, P>(load_quad);
    uint32_t gmx = 0;
    // (the sub-tile loop unrolled: rolled, the ring slots still in flight at its back edge get copied from register to register there,
    // and every copy waits for its load -- the queue drained once per sub-tile)
    ws_static_for<0, NS>([&](auto hc) {
        constexpr int h = decltype(hc)::value;
        asm volatile("" : "+v"(lane));      // (per-quad LDS offsets recomputed per sub-tile, not kept live across sub-tiles)
        const int mw0 = mwt + h * WS_STAT_ROWS;
        const char* const stage = (h & 1) ? stage1 : stage0;
        {
            u32x4_b pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = (rv[e] & 0x0f0f0f0fu) | ((bv[e] & 0x0f0f0f0fu) << 4);
            if (lane < WS_STAT_ROWS) *reinterpret_cast<u32x4_b*>(mstage + lane * 16) = pk;
            if constexpr (h + 1 < NS) load_masks(h + 1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the wave's own writes, read back by other lanes
        float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1;
        auto quad = [&](auto qc) {
            constexpr int q = decltype(qc)::value;
            __builtin_amdgcn_sched_barrier(0);      // quads in program order: the ring slots are what bounds the registers
            // the loads that run P quads ahead (into the slot quad q + P - 12 left P quads ago)
            load_quad(std::integral_constant<int, h * 12 + q + P>{});
            const int r = q * 4 + (lane >> 4);
            const uint32_t m = ws_out_row(a, (uint32_t)(mw0 + r));
            float4 o = *reinterpret_cast<const float4*>(stage + r * 256 + (((lane & 15) ^ (r & 15)) << 4));
            const uint32_t pkb = *reinterpret_cast<const uint8_t*>(mstage + lane + q * 64);
            const float4 inc = o;          // (the convolution's own share of the gradient: DmlConvDesc.bnr_inc)
            if (HO) {
                float4 t = make_float4(__uint_as_float(old[q][0]), __uint_as_float(old[q][1]), __uint_as_float(old[q][2]),
                                       __uint_as_float(old[q][3]));
                if (resm) {
                    t.x = (pkb & 1u) ? t.x : 0.f; t.y = (pkb & 2u) ? t.y : 0.f; t.z = (pkb & 4u) ? t.z : 0.f; t.w = (pkb & 8u) ? t.w : 0.f;
                }
                o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
            }
            const u32x4_b ov = {__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)};
            // (non-temporal whatever nt_out says: one store instruction on every path -- data gradients with operands write 38-600 MB)
            __builtin_amdgcn_raw_buffer_store_b128(ov, rs_y, m * y_row + coff, 0, 2);
            if (BNR) {
                // (rows beyond M: their accumulators are zero -- the loaders fill such rows with zeros -- and so are the operands)
                const uint32_t bits = (pkb >> 4) | nomask;
                const float4 y4 = make_float4(__uint_as_float(yv[q][0]), __uint_as_float(yv[q][1]), __uint_as_float(yv[q][2]),
                                              __uint_as_float(yv[q][3]));
                const float g0 = (bits & 1u) ? o.x : 0.f, g1 = (bits & 2u) ? o.y : 0.f, g2 = (bits & 4u) ? o.z : 0.f,
                            g3 = (bits & 8u) ? o.w : 0.f;
                // (the sums over this launch's own share where the caller says so -- only an accumulating launch has another share)
                const bool use_inc = HO && a.bnr_inc != 0;
                const float s0 = use_inc ? ((bits & 1u) ? inc.x : 0.f) : g0, s1 = use_inc ? ((bits & 2u) ? inc.y : 0.f) : g1,
                            s2 = use_inc ? ((bits & 4u) ? inc.z : 0.f) : g2, s3 = use_inc ? ((bits & 8u) ? inc.w : 0.f) : g3;
                r1.x += s0; r1.y += s1; r1.z += s2; r1.w += s3;
                r2.x += s0 * (y4.x - mu.x) * is.x; r2.y += s1 * (y4.y - mu.y) * is.y;
                r2.z += s2 * (y4.z - mu.z) * is.z; r2.w += s3 * (y4.w - mu.w) * is.w;
                gmx = max(max(gmx, __float_as_uint(g0) & 0x7fffffffu), max(__float_as_uint(g1) & 0x7fffffffu,
                          max(__float_as_uint(g2) & 0x7fffffffu, __float_as_uint(g3) & 0x7fffffffu)));
                asm volatile("" : "+v"(gmx), "+v"(r1.x), "+v"(r2.x));      // (here, not at the end of the sub-tile with 48 values kept live for it)
            }
        };
        ws_static_for<0, 12>(quad);
        __builtin_amdgcn_sched_barrier(0);
        if (BNR) {
            // the four lane groups (lane >> 4) hold the same four channels: fold, then lanes 0 .. 15 write their channels' pairs
            float v[8] = {r1.x, r2.x, r1.y, r2.y, r1.z, r2.z, r1.w, r2.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] += __shfl_xor(v[e], 16, 64);
                v[e] += __shfl_xor(v[e], 32, 64);
            }
            const uint32_t po = (lane < 16 && mw0 < a.M && c0 < a.N) ? ((uint32_t)(mw0 / WS_STAT_ROWS) * (uint32_t)a.N + (uint32_t)c0) * 8u : OOB;
            const u32x4_b p0 = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            const u32x4_b p1 = {__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])};
            __builtin_amdgcn_raw_buffer_store_b128(p0, rs_p, po, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(p1, rs_p, po + 16u, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this sub-tile's reads of its staging area and of the masks
        static_assert(NS == 1 || NS == 3, "one or three sub-tiles per wave tile");
        if constexpr (NS == 3 && h == 0) stage_acc(acc3[2], stage0);
    });
    if (BNR && a.bnr_gmax != nullptr) {      // max |g| of the wave tile, for the plane scale of dy (dml_h2_bound_bn_bwd)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gmx = max(gmx, (uint32_t)__shfl_xor((int)gmx, o, 64));
        if (lane == 0 && gmx != 0)
            atomicMax(reinterpret_cast<uint32_t*>(a.bnr_gmax) + ((blockIdx.x * 16u + (uint32_t)(mwt / WS_STAT_ROWS) + (uint32_t)(nw0 >> 6)) & 1023u), gmx);
    }
}

// The same through 2 KB of LDS that belong to the wave alone (the 144 x 256 configuration leaves 10 KB beside its ring): chunks of
// 16 rows x 32 channels, a store instruction = 8 rows x 128 contiguous bytes (whole cache lines).  No consumer barrier and no held-back
// ring slot: with the staging area inside the ring (conv_epilogue_rows) the loaders prefetch one stage less across the tile boundary
// and the consumers wait for each other -- 8-10 % of a launch with four tiles of eight K steps per CU (profiles/r04_h2_ablations.txt).
// DS operations of one wave execute in order: chunk q + 1 is written right behind the reads of chunk q, whose data the stores then
// wait for with the newer writes still outstanding.  Forward launches only: a version with the data gradients' epilogue operands
// (accumulate, fused BN-backward sums) had four rows of operand loads in flight per lane against the eight of conv_epilogue_rows, and
// those epilogues are bound by exactly that (+2 % on the step's data gradients); both versions in one kernel spill 300 bytes per lane.
template <int NT, int MODE>
__device__ __forceinline__ void conv_epilogue_rows8(f32x4 (&acc)[NT][3], const ConvArgs& a, const int mw0, const int nw0,
                                                    const int lane, char* stage, const bool do_stats = true) {
    static_assert(NT == 4 && MODE == 0, "64-channel wave tile, forward launches");
    const int lr = lane & 15, lq = lane >> 4;
    if (a.stats != nullptr && do_stats) conv_epilogue<float, NT, 3, MODE, false, true>(acc, a, mw0, nw0, lr, lq);
    const int rr = lane >> 3, cc = lane & 7;                     // row side: row within 8, 16-byte chunk within the 128-byte half row
    float* const yb = static_cast<float*>(a.y);
    // chunk q = (fragment j = q >> 1, channel half = q & 1): tiles i = 2 half, 2 half + 1 of fragment j
    auto wr = [&](auto qc) {
        constexpr int q = decltype(qc)::value, j = q >> 1, hf = q & 1;
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
            *reinterpret_cast<f32x4*>(stage + lr * 128 + (((lq * 2 + ii) ^ (lr & 7)) << 4)) = acc[2 * hf + ii][j];
    };
    auto rd = [&](float4 (&o)[2]) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = k * 8 + rr;
            o[k] = *reinterpret_cast<const float4*>(stage + r * 128 + ((cc ^ (r & 7)) << 4));
        }
        asm volatile("" ::: "memory");
    };
    float4 o[2][2];
    auto chunk = [&](auto qc) {
        constexpr int q = decltype(qc)::value, j = q >> 1, hf = q & 1;
        if constexpr (q + 1 < 6) wr(std::integral_constant<int, (q + 1 < 6 ? q + 1 : 0)>{});      // behind the reads of chunk q (in-order DS)
        const int c0 = nw0 + hf * 32 + cc * 4;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int m = mw0 + j * 16 + k * 8 + rr;
            if (m < a.M && c0 < a.N)
                st16f(yb + (int64_t)m * a.ldy + c0, o[q & 1][k].x, o[q & 1][k].y, o[q & 1][k].z, o[q & 1][k].w, (a.nt_out & 1) != 0);
        }
        if constexpr (q + 1 < 6) rd(o[(q + 1) & 1]);
    };
    wr(std::integral_constant<int, 0>{});
    rd(o[0]);
    chunk(std::integral_constant<int, 0>{});
    chunk(std::integral_constant<int, 1>{});
    chunk(std::integral_constant<int, 2>{});
    chunk(std::integral_constant<int, 3>{});
    chunk(std::integral_constant<int, 4>{});
    chunk(std::integral_constant<int, 5>{});
}

// (accumulators in the accumulator register file through inline-asm MFMAs were tried in round 5: hipcc splits the 256 registers of a
// two-waves-per-SIMD kernel 128 / 128, the 144 accumulators of the 144 x 64 wave tile do not fit, and the K loop did not get faster:
// 888 -> 944 us on the ASPP 3x3, profiles/r05_h2_kloop_ablations.txt)

// Tile walk.  One plane: row blocks fastest (the workgroups of an XCD share weight rows).  Two planes: column blocks fastest --
// the 32 workgroups of an XCD then hold 32 / nblk_n neighbouring row blocks x all their column blocks AT THE SAME TIME and the
// activation rows are fetched over the fabric once, not once per column block (row blocks fastest: the column blocks of a row
// block run rounds apart; PMC: 1x1 256 -> 1024 at 48 x 48 read its input 4.2 x).
template <int PL>
__device__ __forceinline__ int ws_tile_m(const int tile, const ConvArgs& a) {
    return PL == 2 ? tile / a.nblk_n : tile % a.nblk_m;
}
template <int PL>
__device__ __forceinline__ int ws_tile_n(const int tile, const ConvArgs& a) {
    return PL == 2 ? tile % a.nblk_n : tile / a.nblk_m;
}

// ring stages: six in one-plane (bf16) launches, three on two planes (51 KB stages)
constexpr int ws_ring_stages(const int PL) { return PL == 1 ? WS_NST : 3; }

// loader wave LW of NLD: compile-time piece ownership (no branches in the issue loop)
// PL = 2: every operand tile is two planes (hi, lo fp16 of the scaled fp32 tensor); a stage = [A hi | A lo | B hi | B lo]
template <int MW, int NW, int MODE, int NLD, int LW, int PL, int MT = WS_MT>
__device__ __forceinline__ void conv_ws_loader(const ConvArgs& a, const uint32_t x_bytes, const uint32_t w_bytes, char* smem,
                                               uint32_t* ready, uint32_t* consumed, const int lane, const int ntiles,
                                               const int first_tile) {
    typedef bf16_t T;
    constexpr int NCW = MW * NW, NT = 4;
    constexpr int BM = 16 * MT * MW, BN = 64 * NW;
    constexpr int PA = BM / 16, PB = BN / 16, NP = PL * (PA + PB);
    constexpr int SB = PL * (BM + BN) * BK * 2;
    constexpr int MYP = (NP - LW + NLD - 1) / NLD;
    constexpr int NST = ws_ring_stages(PL), D = PL == 1 ? WS_D : 1;
    constexpr uint32_t OOB = 0x80000000u;
    static_assert(D * MYP <= 63, "vmcnt is a 6-bit counter");
    // (PL = 2: the descriptors span both planes; the lo plane is reached through the scalar offset)
    const u32x4_ws rs_x = ws_make_rsrc(PL == 1 ? a.x : a.x_planes, PL == 1 ? x_bytes : x_bytes + a.x_plane_bytes),
                   rs_w = ws_make_rsrc(PL == 1 ? a.w : a.w_planes, PL == 1 ? w_bytes : w_bytes + a.w_plane_bytes);
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    const int prow = lane >> 2;
    const int lchunk = (lane & 3) ^ ((0x78 >> (((lane >> 4) & 3) * 2)) & 3);
    const int sh2 = (MODE != 0 && a.stride == 2) ? 1 : 0;
    const int KT = a.Ktot / BK;
    uint32_t g = 0, pub = 0;               // K steps issued / published as landed
    int base[MYP];
    uint32_t mask[MYP];
    int prev_blk_m = -1;
    for (int tile = first_tile; tile < ntiles; tile += (int)gridDim.x) {
        const int blk_m = ws_tile_m<PL>(tile, a), blk_n = ws_tile_n<PL>(tile, a);
        const int m0 = blk_m * BM, n0 = blk_n * BN;
        // per owned piece and lane: A -- signed byte offset of the row's tap-(0,0) pixel (+ swizzled chunk) and one validity
        // bit per filter tap; B -- byte offset into the tile-major weights at K step 0 (see conv_igemm_dma_kernel).  The A part
        // only depends on the row block: a workgroup whose tiles share it (grid = row blocks: N > 256) sets it up once.
        const bool new_rows = blk_m != prev_blk_m;
        prev_blk_m = blk_m;
#pragma unroll
        for (int q = 0; q < MYP; ++q) {
            const int p = q * NLD + LW;             // piece of the stage: [PL x PA activation pieces | PL x PB weight pieces]
            if (p < PL * PA) {
                if (!new_rows) continue;
                base[q] = 0;
                mask[q] = 0;
                const int m = m0 + (p % PA) * 16 + prow;
                if (m < a.M) {
                    const uint32_t b = fdiv((uint32_t)m, a.div_howo);
                    const uint32_t rem = (uint32_t)m - b * (uint32_t)(a.Ho * a.Wo);
                    const uint32_t yo = fdiv(rem, a.div_wo);
                    const uint32_t xo = rem - yo * (uint32_t)a.Wo;
                    const int iy = MODE == 0 ? (int)yo * a.stride - a.pad : (int)yo + a.pad;
                    const int ix = MODE == 0 ? (int)xo * a.stride - a.pad_x : (int)xo + a.pad_x;
                    const int by = MODE == 0 ? iy : (iy >> sh2), bx = MODE == 0 ? ix : (ix >> sh2);
                    base[q] = ((((int)b * a.Hi + by) * a.Wi + bx) * a.ldx + lchunk * 8) * 2;
                    uint32_t mk = 0;
                    for (int r = 0, t = 0; r < a.R; ++r)
                        for (int s = 0; s < a.S; ++s, ++t) {
                            bool ok;
                            if (MODE == 0) {
                                const int ys = iy + r * a.dil, xs = ix + s * a.dil;
                                ok = ((unsigned)ys < (unsigned)a.Hi) && ((unsigned)xs < (unsigned)a.Wi);
                            } else {
                                const int ty = iy - r * a.dil, tx = ix - s * a.dil;
                                ok = (sh2 == 0 || (((ty | tx) & 1) == 0)) && ty >= 0 && tx >= 0 && ((ty >> sh2) < a.Hi) &&
                                     ((tx >> sh2) < a.Wi);
                            }
                            mk |= ok ? (1u << t) : 0u;
                        }
                    mask[q] = mk;
                }
            } else {
                const int row = ((p - PL * PA) % PB) * 16 + prow, n = n0 + row;
                const int bchunk = swz_chunk<T>(b_rho<NT>(row & 63), lane & 3);
                base[q] = n < a.N ? (int)((((int64_t)(n >> 6) * KT) * 2048 + (n & 63) * 32 + bchunk * 8) * 2) : (int)OOB;
            }
        }
        // (K order: every workgroup walks K from step 0.  The workgroups of an XCD share one L2 and -- on the m-fastest tile walk -- the
        // same weight rows; letting each start at its own K step, to spread their simultaneous requests over the L2 channels, LOSES:
        // the weight working set of the moment grows from one K step to the whole matrix and falls out of the 4 MB L2 (ASPP 3x3
        // 278 -> 389 us in bf16, 732 -> 870 us on two planes; gpurun_out/r04 h2_krot).)
        // Two planes: K walks 64-channel groups outermost and the filter taps inside a group.  The workgroups of an XCD hold
        // neighbouring row blocks and move through K together, so at any moment they read ONE channel group of one contiguous
        // row range (+- the halo) whatever the tap: ~1 MB that stays in the XCD's 4 MB L2 across the nine taps.  With the taps
        // outermost a tap sweeps all C channels of that range (4.7 MB at C = 256) before the next tap comes back to the same
        // lines, and every tap was a miss (PMC: 3x3 256 -> 256 at 48 x 48 fetched 4.4 x its algorithmic bytes, the decoder's
        // data gradient 12.6 x).  64 channels = the two K steps that share a 128-byte line.
        constexpr bool TAPIN = PL == 2;
        const int ksteps_c = a.C / BK;
        int ir = 0, is = 0, ic0 = 0, cg0 = 0;
        for (int kt = 0; kt < KT; ++kt) {
            if (g >= (uint32_t)NST) {
                // the stage this K step overwrites must have been read by every consumer wave
                const uint32_t need = g - NST + 1;
                bool drained = false;
                for (;;) {
                    uint32_t mn = ws_ld(consumed);
#pragma unroll
                    for (int w = 1; w < NCW; ++w) mn = min(mn, ws_ld(consumed + w));
                    if (mn >= need) break;
                    if (!drained) {
                        // ring full, nothing to issue: let everything in flight land and publish it now instead of D issues
                        // later -- with the shallow ring of the two-plane mode (3 stages) the consumers otherwise only ever
                        // see one stage ahead
                        wait_vmcnt<0>();
                        ws_st(ready + LW, g);
                        pub = g;
                        drained = true;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
            }
            const uint32_t sbase = lds0 + (g % NST) * SB;
            const uint32_t tapbit = 1u << (ir * a.S + is);
            const int ktw = TAPIN ? (ir * a.S + is) * ksteps_c + ic0 / BK : kt;      // the K step's tile in the (tap-major) weight copy
            const int soff = (MODE == 0 ? ((ir * a.dil) * a.Wi + is * a.dil) * a.ldx
                                        : -((((ir * a.dil) >> sh2) * a.Wi + ((is * a.dil) >> sh2)) * a.ldx)) * 2 + ic0 * 2;
#pragma unroll
            for (int q = 0; q < MYP; ++q) {
                const int p = q * NLD + LW;
                if (p < PL * PA) {
                    const uint32_t voff = (mask[q] & tapbit) ? (uint32_t)(base[q] + soff) : OOB;
                    ws_dma16(rs_x, sbase + p * 1024, voff, p < PA ? 0u : a.x_plane_bytes);
                } else {
                    ws_dma16(rs_w, sbase + p * 1024, (uint32_t)base[q],
                             (uint32_t)ktw * 4096u + ((p - PL * PA) < PB ? 0u : a.w_plane_bytes));
                }
            }
            ic0 += BK;
            if (TAPIN) {
                if (ic0 >= a.C || ic0 >= cg0 + 64) {             // this tap's share of the channel group is done
                    ic0 = cg0;
                    if (++is == a.S) {
                        is = 0;
                        if (++ir == a.R) { ir = 0; cg0 += 64; ic0 = cg0; }
                    }
                }
            } else if (ic0 >= a.C) {
                ic0 = 0;
                if (++is == a.S) { is = 0; ++ir; }
            }
            ++g;
            if (g > (uint32_t)D + pub) {
                wait_vmcnt<D * MYP>();             // at most D stages of this wave's pieces in flight: stage g - 1 - D has landed
                pub = g - D;
                ws_st(ready + LW, pub);
            }
        }
    }
    wait_vmcnt<0>();
    ws_st(ready + LW, g);
}

// EPI (two planes, data gradient): 0 no epilogue operand, 1 accumulate / identity-branch gradient, 2 fused BatchNorm-backward sums,
// 3 both -- ONE epilogue per instantiation (all of them behind run-time branches in one kernel: 144 accumulators live at a four-way
// fork, 400-700 bytes of scratch per lane)
template <int MW, int NW, int MODE, int NLD, int PL, int MT, int EPI>
__device__ __forceinline__ void conv_ws_body(const ConvArgs& a, const uint32_t x_bytes, const uint32_t w_bytes) {
    typedef bf16_t T;
    static_assert(MW * NW == 4, "four consumer waves, one per SIMD");
    static_assert(MT % 3 == 0 && MT >= 3, "48-row sub-tiles (statistics groups, row epilogue)");
    constexpr int NCW = MW * NW, NT = 4, NST = ws_ring_stages(PL);
    constexpr int BM = 16 * MT * MW, BN = 64 * NW;
    constexpr int SB = PL * (BM + BN) * BK * 2;
    // two planes, 144 x 256: 2 KB of private staging per consumer wave behind the flags (conv_epilogue_rows8); the 288 x 128
    // configuration has no room for it and stages in the slot of the tile's last K stage (conv_epilogue_rows)
    // (forward only: nearly every data gradient of a plan carries epilogue operands -- accumulate, fused BN-backward sums -- whose
    // loads want the deeper row groups of conv_epilogue_rows, and both epilogues in one kernel spill 300 bytes per lane)
    constexpr bool PRIV_STAGE = PL == 2 && MW == 1 && MODE == 0;
    // two planes, 192 x 64 (MW = 4, MT = 3: the 64-channel layers; 48 x 64 wave tiles): its ring is 3 x 32 KB, so the row epilogue's
    // 12 KB per wave sit BESIDE the ring in both directions -- no held-back slot, no consumer barrier (conv_epilogue_rows)
    constexpr bool PRIV_ROWS = PL == 2 && MW == 4;
    constexpr int ROWS_STAGE = PRIV_ROWS ? WS_STAT_ROWS * 256 : 0;
    // (two planes, data gradient: 768 bytes per consumer wave for the ReLU masks of a 48-row sub-tile, conv_epilogue_rows)
    constexpr int MASK_STAGE = (PL == 2 && !PRIV_STAGE) ? WS_STAT_ROWS * 16 : 0;
    __shared__ __attribute__((aligned(1024))) char smem[NST * SB + 64 + (PRIV_STAGE ? NCW * 2048 : NCW * (MASK_STAGE + ROWS_STAGE))];
    static_assert(sizeof(smem) <= 160 * 1024, "LDS of one CU");
    uint32_t* const ready = reinterpret_cast<uint32_t*>(smem + NST * SB);          // [NLD] stages landed, per loader
    uint32_t* const consumed = ready + 4;                                          // [4] stages whose reads were issued

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 16) reinterpret_cast<uint32_t*>(smem + NST * SB)[tid] = 0;
    __syncthreads();

    const int ntiles = a.nblk_m * a.nblk_n;
    const int first_tile = xcd_remap(blockIdx.x, gridDim.x);      // this workgroup walks first_tile, + grid, + 2 grid, ...
    const int KT = a.Ktot / BK;

    if (wave >= NCW) {
        const int lw = wave - NCW;
        if (lw == 0) conv_ws_loader<MW, NW, MODE, NLD, 0, PL, MT>(a, x_bytes, w_bytes, smem, ready, consumed, lane, ntiles, first_tile);
        if (NLD > 1 && lw == 1) conv_ws_loader<MW, NW, MODE, NLD, (NLD > 1 ? 1 : 0), PL, MT>(a, x_bytes, w_bytes, smem, ready, consumed, lane, ntiles, first_tile);
        if (NLD > 2 && lw == 2) conv_ws_loader<MW, NW, MODE, NLD, (NLD > 2 ? 2 : 0), PL, MT>(a, x_bytes, w_bytes, smem, ready, consumed, lane, ntiles, first_tile);
        if (NLD > 3 && lw == 3) conv_ws_loader<MW, NW, MODE, NLD, (NLD > 3 ? 3 : 0), PL, MT>(a, x_bytes, w_bytes, smem, ready, consumed, lane, ntiles, first_tile);
        return;
    }

    // ---------------------------------------------------------------------- consumer
    __builtin_amdgcn_s_setprio(3);      // the MFMA waves ahead of the loader wave that shares their SIMD (+0.15 % on the step)
    const int wm = wave / NW, wn = wave % NW;
    const int lr = lane & 15, lq = lane >> 4;
    constexpr bool priv = PRIV_STAGE || PRIV_ROWS;      // the epilogue stages beside the ring: a tile's last stage is released like any other
    uint32_t g = 0, rflag = 0, tiles_done = 0;
    uint32_t* const edone = consumed + 4;                  // [4] tiles whose last fragment reads were issued, per consumer wave
    auto read_ready = [&]() -> uint32_t {
        uint32_t v = ws_ld(ready);
#pragma unroll
        for (int w = 1; w < NLD; ++w) v = min(v, ws_ld(ready + w));
        return v;
    };
    auto wait_ready = [&](const uint32_t need) {
        while (rflag < need) {
            __builtin_amdgcn_s_sleep(1);
            rflag = read_ready();
        }
        asm volatile("" ::: "memory");
    };
    constexpr int A_PLANE = BM * BK * 2, B_PLANE = BN * BK * 2;      // bytes from the hi plane to the lo plane inside a stage
    constexpr bool EPI_OPS = PL == 2 && MODE == 1 && !PRIV_STAGE;
    static_assert(EPI == 0 || EPI_OPS, "epilogue operands: two-plane data gradients");
    constexpr bool hold2 = EPI != 0 && !priv;

    for (int tile = first_tile; tile < ntiles; tile += (int)gridDim.x) {
        const int blk_m = ws_tile_m<PL>(tile, a), blk_n = ws_tile_n<PL>(tile, a);
        // fragment byte offsets inside a stage (hi plane; the lo plane is BM / BN rows further).  Recomputed per tile from a lane
        // index the optimiser cannot see through: hoisted out of the tile loop these 13 registers stay live across the epilogue,
        // where the 144 accumulator registers leave no room for them (spills, and a scratch reload waits vmcnt(0) -- for every
        // store issued before it).
        int lr_k = lr, lq_k = lq;
        asm volatile("" : "+v"(lr_k), "+v"(lq_k));
        int a_off[MT], b_off[NT];
        // (the chunk swizzle of a 64-byte bf16 / fp16 row looks at row bits 2-3 only: fragment j sits j KB behind fragment 0 -- written
        // that way, the nine offsets are ONE register and immediates)
        static_assert(BK * 2 * 16 == 1024, "16 rows of 64 bytes per fragment");
        const int a_off0 = (wm * (16 * MT) + lr_k) * (BK * 2) + swz_chunk<T>(lr_k & 15, lq_k) * 16;
#pragma unroll
        for (int j = 0; j < MT; ++j) a_off[j] = a_off0 + j * 1024;
#pragma unroll
        for (int i = 0; i < NT; ++i) b_off[i] = PL * BM * BK * 2 + (wn * 64 + b_row<NT>(i, lr_k)) * (BK * 2) + swz_chunk<T>(lr_k, lq_k) * 16;
        // accumulators by 48-row sub-tile: ACC(i, j) = acc3[j / 3][i][j % 3], so that the epilogue takes a sub-tile by reference
        f32x4 acc3[MT / 3][NT][3];
#define ACC(i, j) acc3[(j) / 3][i][(j) % 3]
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) ACC(i, j) = (f32x4){0.f, 0.f, 0.f, 0.f};

        if constexpr (PL == 1) {
            mfma_bf16x8 bfA[NT], bfB[NT], af[MT], alA, alB;       // af[MT - 1] unused: the last A fragment alternates alA / alB
            wait_ready(g + 1);                                      // first K step of the tile: exposed once per tile
            {
                const char* sb = smem + (g % NST) * SB;
#pragma unroll
                for (int i = 0; i < NT; ++i) bfA[i] = *reinterpret_cast<const mfma_bf16x8*>(sb + b_off[i]);
#pragma unroll
                for (int j = 0; j < MT - 1; ++j) af[j] = *reinterpret_cast<const mfma_bf16x8*>(sb + a_off[j]);
                alA = *reinterpret_cast<const mfma_bf16x8*>(sb + a_off[MT - 1]);
            }
            // one K step: MFMAs of step g from (bc, af, alc); the fragments of step g + 1 into (bn, af, aln) as registers free up
            auto step = [&](mfma_bf16x8 (&bc)[NT], mfma_bf16x8 (&bn)[NT], mfma_bf16x8& alc, mfma_bf16x8& aln, const bool has_next) {
                asm volatile("" ::: "memory");
                ws_st(consumed + wave, g + 1);         // every read of stage g has been issued (DS runs a wave's operations in order)
                const char* sn = smem + ((g + 1) % NST) * SB;
                if (has_next) {
                    wait_ready(g + 2);
#pragma unroll
                    for (int i = 0; i < NT; ++i) bn[i] = *reinterpret_cast<const mfma_bf16x8*>(sn + b_off[i]);
                    aln = *reinterpret_cast<const mfma_bf16x8*>(sn + a_off[MT - 1]);
                }
#pragma unroll
                for (int j = 0; j < MT - 1; ++j) {
#pragma unroll
                    for (int i = 0; i < NT; ++i) ACC(i, j) = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[i], af[j], ACC(i, j), 0, 0, 0);
                    if (has_next) af[j] = *reinterpret_cast<const mfma_bf16x8*>(sn + a_off[j]);
                    if (j == (MT - 1) / 2) rflag = read_ready();      // the next step's poll, answered under the MFMAs
                }
#pragma unroll
                for (int i = 0; i < NT; ++i) ACC(i, MT - 1) = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[i], alc, ACC(i, MT - 1), 0, 0, 0);
                ++g;
            };
            int kt = 0;
            for (; kt + 1 < KT; kt += 2) {
                step(bfA, bfB, alA, alB, true);
                step(bfB, bfA, alB, alA, kt + 2 < KT);
            }
            if (kt < KT) step(bfA, bfB, alA, alB, false);
        } else {
            // two fp16 planes per operand: x s = xh + xl, w t = wh + wl; per 16 x 16 x 32 block the three products wh xh, wh xl,
            // wl xh (the dropped wl xl is below 2^-22 of the block) -- 108 MFMAs per K step against 26 fragment reads.
            // Every fragment is in flight one row group (12 MFMAs, ~200 cycles) before its first use: the activation pair of
            // group j + 1 is read ahead of group j's MFMAs (two register slots; 9 groups per step, so the slot of group 0
            // alternates from step to step: P), the hi weight fragments of step k + 1 under groups 5.. of step k (two sets,
            // alternating), the lo weight fragments -- used LAST in every group -- right after step k's final MFMAs, under the
            // first eight of step k + 1.  __builtin_amdgcn_sched_barrier pins that order: left to itself hipcc sinks each
            // read to just before its use and waits lgkmcnt(0) there, nine exposed LDS latencies per step (measured: 1.45 us per
            // step against 0.72 of MFMA issue).
            // (two groups ahead -- three slots, waits at lgkmcnt 3-6 instead of 1-2 -- measured +-0 on the step, 76.64 vs 76.56 ms over
            // five interleaved pairs: the latency of the fragment reads is covered at one group already; what they cost is issue slots,
            // profiles/r05_h2_kloop_ablations.txt)
            mfma_f16x8 bhA[NT], bhB[NT], bl[NT], ah[2], al[2];
            uint32_t pl[NLD];
#define WS_FRAG(p) (*reinterpret_cast<const mfma_f16x8*>(p))
            wait_ready(g + 1);                                      // first K step of the tile: exposed once per tile
            {
                const char* sb = smem + (g % NST) * SB;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    bhA[i] = WS_FRAG(sb + b_off[i]);
                    bl[i] = WS_FRAG(sb + b_off[i] + B_PLANE);
                }
                ah[0] = WS_FRAG(sb + a_off[0]);
                al[0] = WS_FRAG(sb + a_off[0] + A_PLANE);
            }
            auto step = [&](auto pc, mfma_f16x8 (&bc)[NT], mfma_f16x8 (&bn)[NT], const bool has_next, const bool rel) {
                constexpr int P = decltype(pc)::value;
                const char* sb = smem + (g % NST) * SB;
                // (last step of the tile: the "next" reads fall on this stage again and are never used)
                const char* sn = has_next ? smem + ((g + 1) % NST) * SB : sb;
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    // (positions inside the step: row group 1 / 4 / 5.. of the nine of a 144-row wave tile, 0 / 1 / 2 of a 48-row one)
                    constexpr int JP = MT >= 9 ? 1 : 0, JW = MT >= 9 ? 4 : 1, JB = MT >= 9 ? 5 : MT - 1;
                    // The non-MFMA instructions of a row group SPREAD between its three MFMA quads instead of clustered in front of
                    // them: a wave issues in order, and a cluster of five or six of them (two fragment reads, waits, hazard nops)
                    // outlasts the 16 cycles of the MFMA before it -- the ablations put 25-30 % of the K loop on the fragment reads
                    // although the LDS itself is busy a fifth of the time (profiles/r05_h2_kloop_ablations.txt).
                    // fragment slots: this group's and the one of the group read ahead (two slots, alternating from step to step with
                    // P because MT is odd)
                    const int CUR = (j + P) & 1, NXT = (j + 1 + P) & 1;
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < NT; ++i) ACC(i, j) = __builtin_amdgcn_mfma_f32_16x16x32_f16(bc[i], ah[CUR], ACC(i, j), 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (j + 1 < MT) {
                        ah[NXT] = WS_FRAG(sb + a_off[j + 1]);
                    } else {
                        asm volatile("" ::: "memory");
                        ah[NXT] = WS_FRAG(sn + a_off[0]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < NT; ++i) ACC(i, j) = __builtin_amdgcn_mfma_f32_16x16x32_f16(bc[i], al[CUR], ACC(i, j), 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (j + 1 < MT) {
                        al[NXT] = WS_FRAG(sb + a_off[j + 1] + A_PLANE);
                    } else {
                        asm volatile("" ::: "memory");
                        // every read of stage g has been issued (the tile's LAST stage is announced after the epilogue, which
                        // stages the output rows in its slot)
                        if (rel || priv) ws_st(consumed + wave, g + 1);
                        al[NXT] = WS_FRAG(sn + a_off[0] + A_PLANE);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < NT; ++i) ACC(i, j) = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[i], ah[CUR], ACC(i, j), 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (j == JP) {     // the next step's poll, answered under the MFMAs
#pragma unroll
                        for (int w = 0; w < NLD; ++w) pl[w] = ws_ld(ready + w);
                    }
                    if (j == JW) {
                        rflag = pl[0];
#pragma unroll
                        for (int w = 1; w < NLD; ++w) rflag = min(rflag, pl[w]);
                        if (has_next) wait_ready(g + 2);
                    }
                    if (MT >= 9) {                      // the next step's hi weight fragments, one per row group
                        if (j >= JB && j < JB + NT) bn[j - JB] = WS_FRAG(sn + b_off[j - JB]);
                    } else if (j == JB) {
#pragma unroll
                        for (int i = 0; i < NT; ++i) bn[i] = WS_FRAG(sn + b_off[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < NT; ++i) bl[i] = WS_FRAG(sn + b_off[i] + B_PLANE);
                __builtin_amdgcn_sched_barrier(0);
                ++g;
            };
            // (a data gradient with epilogue operands holds back the slots of its last TWO K stages: conv_epilogue_rows_ops)
            int kt = 0;
            for (; kt + 1 < KT; kt += 2) {
                step(std::integral_constant<int, 0>{}, bhA, bhB, true, !(hold2 && kt + 2 == KT));
                step(std::integral_constant<int, 1>{}, bhB, bhA, kt + 2 < KT, kt + 2 < KT && !(hold2 && kt + 3 == KT));
            }
            if (kt < KT) step(std::integral_constant<int, 0>{}, bhA, bhB, false, false);
        }
        // cut the accumulators' live ranges (see conv_igemm_kernel), then the shared epilogue per 48-row group
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(ACC(i, j)));
        if constexpr (PL == 2) {
            const float un = a.x_unscale[0] * a.w_unscale[0];      // exact powers of two
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) ACC(i, j) *= un;
        }
        // (three explicit copies: hipcc does not unroll a loop around the inlined epilogue, and a run-time index into acc
        // sends all 36 accumulator fragments through scratch memory -- 37 MB written and read back per launch, +25 us)
        char* rows_stage = nullptr;
        if (PRIV_STAGE) rows_stage = smem + NST * SB + 64 + wave * 2048;
        if (PRIV_ROWS) rows_stage = smem + NST * SB + 64 + NCW * MASK_STAGE + wave * ROWS_STAGE;
        if (PL == 2 && !priv) {
            // the slot of the tile's last K step becomes the staging area of conv_epilogue_rows (12 KB per wave): every consumer
            // wave must have issued its last fragment reads first
            ++tiles_done;
            asm volatile("" ::: "memory");
            ws_st(edone + wave, tiles_done);
            for (;;) {
                uint32_t mn = ws_ld(edone);
#pragma unroll
                for (int w = 1; w < NCW; ++w) mn = min(mn, ws_ld(edone + w));
                if (mn >= tiles_done) break;
                __builtin_amdgcn_s_sleep(1);
            }
            asm volatile("" ::: "memory");
            rows_stage = smem + ((g - 1) % NST) * SB + wave * (WS_STAT_ROWS * 256);
        }
        // One copy of the epilogue code, run three times on acc[.][0..2] with the accumulators rotated down by a sub-tile in
        // between (2 x 96 register moves): three inlined copies -- what a compile-time sub-tile index costs; a run-time index into
        // acc would send all of it through scratch memory -- made these kernels 10-19 K instructions, more than the instruction
        // cache two CUs share.
        // forward, 144-row wave tiles: the BatchNorm statistics of the whole wave tile at once (ws_tile_stats)
        constexpr bool TILE_STATS = PL == 2 && MODE == 0 && MT == 9;
        if constexpr (TILE_STATS) {
            if (a.stats != nullptr) ws_tile_stats<NT, MT / 3>(acc3, a, blk_m * BM + wm * (16 * MT), blk_n * BN + wn * 64, lr, lq);
        }
        if constexpr (EPI != 0)
            conv_epilogue_rows_ops<NT, MT / 3, (EPI & 1) != 0, (EPI & 2) != 0>(
                acc3, a, blk_m * BM + wm * (16 * MT), blk_n * BN + wn * 64, lane, rows_stage,
                priv ? rows_stage : smem + ((g - 2) % NST) * SB + wave * (WS_STAT_ROWS * 256), smem + NST * SB + 64 + wave * MASK_STAGE);
#pragma clang loop unroll(disable)
        for (int h = 0; h < (EPI != 0 ? 0 : MT / 3); ++h) {
            const int mw0 = blk_m * BM + wm * (16 * MT) + h * WS_STAT_ROWS, nw0 = blk_n * BN + wn * 64;
            if constexpr (PL == 1) conv_epilogue<bf16_t, NT, 3, MODE, false>(acc3[0], a, mw0, nw0, lr, lq);
            else if (MODE == 0 && (a.bias != nullptr || a.post_scale != nullptr)) {
                conv_epilogue<float, NT, 3, MODE, false>(acc3[0], a, mw0, nw0, lr, lq);      // (inference epilogue, bias: scattered stores)
            } else if (PRIV_STAGE) {
                if constexpr (PRIV_STAGE) conv_epilogue_rows8<NT, MODE>(acc3[0], a, mw0, nw0, lane, rows_stage, !TILE_STATS);
            } else {
                conv_epilogue_rows<NT, MODE, !EPI_OPS>(acc3[0], a, mw0, nw0, lane, rows_stage, smem + NST * SB + 64 + wave * MASK_STAGE,
                                                       !TILE_STATS);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // its reads of the staging area, before the next group's writes
            }
            if constexpr (MT == 9) {
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        acc3[0][i][j] = acc3[1][i][j];
                        acc3[1][i][j] = acc3[2][i][j];
                        // (keeps the loop a loop: the optimiser must not see through the rotation and re-specialise the three trips)
                        asm volatile("" : "+v"(acc3[0][i][j]), "+v"(acc3[1][i][j]));
                    }
            } else {
                static_assert(MT == 9 || MT == 3, "accumulator rotation of the sub-tile loop");
            }
        }
#undef ACC
        if (PL == 2 && !priv) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ws_st(consumed + wave, g);                  // the tile's last stage: its slot is free again
        }
    }
}

template <int MW, int NW, int MODE, int NLD, int PL = 1, int MT = WS_MT, int EPI = 0>
__global__ __launch_bounds__((MW * NW + NLD) * 64) void conv_ws_kernel(const ConvArgs a, const uint32_t x_bytes, const uint32_t w_bytes) {
    conv_ws_body<MW, NW, MODE, NLD, PL, MT, EPI>(a, x_bytes, w_bytes);
}

// two-plane instantiations of the wave-specialised kernel (ConvChoice::pl == 2)
// Each including translation unit owns the instantiations of ONE mode and says which in CONV_WS_PLANES_MODE (0: forward, conv_ws.hip;
// 1: data gradient, conv_ws_dgrad.hip): naming the other's would compile the library's slowest kernels a second time, silently.
#ifndef CONV_WS_PLANES_MODE
#error "define CONV_WS_PLANES_MODE before including conv_ws.h"
#endif
template <int MODE, int EPI>
void launch_ws_planes(const cc::ConvChoice& c, const ConvArgs& a, hipStream_t st) {
    static_assert(MODE == CONV_WS_PLANES_MODE, "two-plane instantiations of this mode belong to the other translation unit");
    constexpr int NLD = WS_PLANES_NLD;
    const dim3 grid(c.grid), block(c.block);
    if (c.mw == 1 && c.mt == 3) {      // 48 x 256 tiles: forward launches only
        if constexpr (MODE == 0 && EPI == 0)
            hipLaunchKernelGGL((conv_ws_kernel<1, 4, 0, NLD, 2, 3, 0>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
    } else if (c.mw == 4)
        hipLaunchKernelGGL((conv_ws_kernel<4, 1, MODE, NLD, 2, 3, EPI>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
    else if (c.mw == 1)
        hipLaunchKernelGGL((conv_ws_kernel<1, 4, MODE, NLD, 2, WS_MT, EPI>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
    else
        hipLaunchKernelGGL((conv_ws_kernel<2, 2, MODE, NLD, 2, WS_MT, EPI>), grid, block, 0, st, a, c.kx_bytes, c.kw_bytes);
}

}  // namespace
