// Which kernel takes a convolution descriptor, and with which tiling: validation and choice of dml_conv_igemm, dml_conv_stat_rows,
// dml_conv_wgrad and dml_conv_wgrad_group as pure host code -- integer arithmetic on a descriptor, no HIP, no allocation, no
// pointer dereferenced (pointers are looked at for nullness, alignment and equality only).  conv_igemm.hip fills the kernel
// arguments from the descriptor plus the choice and switches over it (the wave-specialised kernel's switch is the launcher of
// conv_ws.hip, declared in conv_device.h); tests/tools/conv_choice_dump.cpp prints it without a GPU.
// The measurement notes beside each rule are the record of why the rule is what it is.
#pragma once
#include <cstdint>

#include "../../include/dmlnet_hip.h"

namespace conv_choice {

constexpr int CUS = 256;                 // compute units of the MI355X: one round of workgroups
constexpr int BK = 32;                   // K tile (channels of one tap) of every kernel; pixel tile of the weight gradients
constexpr int NTHREADS = 256;
constexpr int WS_MT = 9;                 // 16-row fragments per wave tile of the wave-specialised kernel (144 rows)
constexpr int WS_STAT_ROWS = 48;         // rows per statistics group of that kernel
constexpr int WS_NLD = 3;                // its loader waves (bf16 and two-plane instantiations alike)
constexpr int WB_THREADS = 512;          // workgroup of the 256 x 256 weight-gradient kernel
constexpr int WGW_TN = 128, WGW_TK = 256, WGW_NLD = 3;      // output tile and loader waves of the wave-specialised weight gradient
constexpr int WG_MAX_JOBS = 12;          // jobs of one grouped weight-gradient launch

// The library's run-time switches (read once from the environment by conv_igemm.hip).  Tests select kernel families through them.
//   DML_CONV_V1     set: bf16 launches on the register-staged kernel instead of the LDS-DMA ones
//   DML_CONV_BM256  256-row tiles of the LDS-DMA kernel: 0 never, 1 the rule in conv_choose (default), 2 every eligible layer,
//                   >= 64 the K threshold of the rule
//   DML_CONV_WS     non-zero: bf16 launches on conv_ws_kernel wherever conv_ws_eligible allows (default 0)
struct ConvSwitches {
    bool v1;
    int bm256, ws;
};

static inline int mul32(const int a, const int b) { return (int)((uint32_t)a * (uint32_t)b); }      // the int product, wrapping
static inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// bytes of an activation operand [B][Hi][Wi] x C channels at pitch ld with es-byte elements (extent of its buffer descriptor)
static inline int64_t operand_bytes(const int B, const int Hi, const int Wi, const int ld, const int C, const int es) {
    return (((int64_t)mul32(B, Hi) * Wi - 1) * ld + C) * es;
}
static inline int blocks_for(const int64_t work_items, const int block, const int max_blocks = 256 * 8) {      // (grid_for of common.h)
    int64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// ------------------------------------------------------------------------------------------------
// forward / data gradient
// ------------------------------------------------------------------------------------------------
enum ConvFamily {
    CONV_REG = 0,      // conv_igemm_kernel<T, BN, ALIGNED, MODE>: register-staged
    CONV_RING,         // conv_igemm_dma_kernel<BN, MODE, 3, WPE, BM, TMW>: LDS-DMA ring
    CONV_WS,           // conv_ws_kernel<MW, NW, MODE, 3, PL, MT, EPI>: wave-specialised, persistent
    CONV_X3            // conv_igemm_x3_kernel<BN, MODE>: three-term split
};

struct ConvChoice {
    int family;
    int elem_bytes;                   // T: 2 = bf16_t, 4 = float
    int mode;                         // MODE: 0 forward, 1 data gradient, 2 data gradient adding DmlConvDesc::acc32
    int bn, aligned;                  // REG: BN, ALIGNED; RING and X3: BN
    int bm, tmw, wpe;                 // RING
    int mw, nw, pl, mt, epi;          // WS
    int nblk_m, nblk_n, tail_full, tail_q, nt_out;      // ConvArgs fields of the same names
    uint32_t x_bytes, w_bytes;        // ConvArgs::x_bytes / w_bytes (0: an operand of 2^31 bytes or more)
    uint32_t kx_bytes, kw_bytes;      // RING and WS: the kernel's own x_bytes / w_bytes arguments
    int grid, block;
    int stat_rows;                    // rows of the GEMM per statistics partial (dml_conv_stat_rows); valid whatever conv_choose returns
};

// what conv_args puts into the launch: fields of the descriptor that are only in effect together with others
static inline int conv_m(const DmlConvDesc& d) { return mul32(mul32(d.B, d.Ho), d.Wo); }
static inline int conv_ktot(const DmlConvDesc& d) { return mul32(mul32(d.R, d.S), d.C); }
static inline int conv_f32_split(const DmlConvDesc& d) { return d.dtype == DML_F32 ? d.f32_split : 0; }
static inline bool conv_has_planes(const DmlConvDesc& d) { return conv_f32_split(d) == 2 && d.x_planes && d.w_planes; }
static inline bool conv_has_tail(const DmlConvDesc& d) { return d.tail_ws && d.tail_counters && d.tail_ws_elems > 0 && d.tail_counters_len > 0; }
static inline int conv_pad_x(const DmlConvDesc& d) { return d.pad_w_set ? d.pad_w : d.pad; }

static inline int64_t conv_x_bytes(const DmlConvDesc& d, const int es) { return operand_bytes(d.B, d.Hi, d.Wi, d.ldx, d.C, es); }
static inline int64_t conv_w_bytes(const DmlConvDesc& d, const int es) { return (int64_t)d.N * conv_ktot(d) * es; }

// bf16: may this launch run on the LDS-DMA kernels?  K tiles inside one tap, N > 32, tensors addressable with a 31-bit byte offset
static inline bool conv_dma_eligible(const DmlConvDesc& d, const ConvSwitches& sw, const int64_t xb, const int64_t wb) {
    return !sw.v1 && (d.C % BK) == 0 && d.R * d.S <= 32 && d.N > 32 && xb < (1ll << 31) && wb < (1ll << 31);
}

// ... and among them on conv_ws_kernel?
static inline bool conv_ws_eligible(const DmlConvDesc& d, const ConvSwitches& sw, const int64_t xb, const int64_t wb) {
    // bf16 plans: OPT-IN (DML_CONV_WS=1).  Per launch it wins where K is long (rule below), but in the train step the persistent
    // 150 KB-of-LDS workgroups keep the side stream's weight-gradient workgroups off the CUs they hold and static tile lists
    // cannot rebalance around them: whole step 391.5 / 392.2 images/s with it, 395.3 / 394.9 without (two interleaved pairs,
    // profiles/r04_ab_ws.txt).  The two-plane fp32 mode (conv_ws_planes_eligible) always runs on it.
    // (forward-only for the long-K launches, where nothing runs beside the main stream, measured +0.1...0.4 % on the step -- and moved
    // the bf16 plan's rounding (48-row statistics groups) enough to redraw the chaotic 30-step trajectory of
    // tests/test_gpu_training_equivalence.py past its bar; not worth a different default)
    if ((!sw.ws && d.ws_min_tiles <= 0) || !d.w_tiled || (d.C % BK) != 0 || d.R * d.S > 32 || (d.N % 128) != 0) return false;
    if (xb >= (1ll << 31) || wb >= (1ll << 31)) return false;
    // long K loops only: a consumer wave runs its tile's epilogue itself, with nothing of the same workgroup to cover it, and
    // below ~32 K steps per tile that costs more than the K loop gains (tools/bench_ws.py, profiles/r04_bench_ws_2.txt: K = 256
    // with four tiles per workgroup 42.5 vs 31.6 us, K = 512 120 vs 89; K = 1024 28.6 vs 32.0, K = 2304 52.9 vs 60.5, K = 4608
    // 158 vs 207, K = 18432 284 vs 372).  ws_min_tiles > 0 (tests) lifts the rule.
    if (d.ws_min_tiles <= 0 && d.R * d.S * d.C < 1024) return false;
    // a persistent workgroup per CU: the tile list must fill most of the chip
    const int bn = (d.N % 256) == 0 ? 256 : 128, bm = (d.N % 256) == 0 ? 144 : 288;
    const int64_t ntiles = ((int64_t)conv_m(d) + bm - 1) / bm * (d.N / bn);
    return ntiles >= (d.ws_min_tiles > 0 ? d.ws_min_tiles : 192);
}
// two planes, forward: 48 x 256 tiles instead of 144 x 256 for launches that leave most of the chip empty (also decides the rows per
// statistics partial)
static inline bool ws_planes_short(const DmlConvDesc& d, const int mode) {
    return mode == 0 && (d.N % 256) == 0 && ((conv_m(d) + 143) / 144) * (d.N / 256) * 2 <= 256;
}
// rows of the GEMM per BatchNorm statistics partial of a two-plane FORWARD launch: the whole 144-row wave tile (ws_tile_stats) except on
// the 48-row wave tiles (64 output channels, short tiles)
static inline int ws_planes_stat_rows(const DmlConvDesc& d, const int mode) {
    if (mode != 0) return 48;
    return (d.N == 64 || ws_planes_short(d, mode)) ? 48 : 144;
}
// the same kernel on two fp16 planes per operand (fp32 tensors, f32_split == 2): every shape it can address -- the alternative
// is the three-term split kernel at a third of its rate
static inline bool conv_ws_planes_eligible(const DmlConvDesc& d, const int mode) {
    if (mode == 0 && d.accum) return false;      // (an accumulating FORWARD launch: no plan issues one; the forward epilogue has no such path)
    if (!conv_has_planes(d) || !d.x_unscale || !d.w_unscale) return false;
    // (plane strides the kernel argument holds: a larger one would wrap in x_plane_bytes)
    if (d.x_plane_stride >= (1ll << 30) || d.w_plane_stride >= (1ll << 30)) return false;
    // (N = 320: the decoder's data gradient.  N = 64 -- layer1's 3x3 and the 256 -> 64 1x1 -- runs the 288 x 128 configuration with
    // half of every tile empty: zero weight rows through the descriptor's range check, no stores; still ahead of the three-term
    // kernel those layers took before: whole step +0.4 %, two interleaved pairs)
    if ((d.C % BK) != 0 || d.R * d.S > 32 || (d.N % 64) != 0) return false;
    if (mode == 1 && conv_ktot(d) < 2 * BK) return false;      // (conv_epilogue_rows_ops stages in the slots of a tile's last two K stages)
    // whole 16-byte vectors of the fp32 output and of every epilogue operand (conv_epilogue_rows); the inference epilogue's operands
    // are in effect with post_scale only
    const bool post = d.post_scale != nullptr;
    if ((d.ldy & 3) != 0 || (post && d.post_res != nullptr && (d.post_ldres & 3) != 0) ||
        ((addr(d.y) | addr(d.bias) | (post ? addr(d.post_res) | addr(d.post_scale) | addr(d.post_shift) | addr(d.post_mean) : 0)) & 15) != 0)
        return false;
    return conv_x_bytes(d, 2) + (uint32_t)(d.x_plane_stride * 2) < (1ll << 31) && conv_w_bytes(d, 2) + (uint32_t)(d.w_plane_stride * 2) < (1ll << 31);
}

// Tiles of the partially filled last round, split along K (DmlConvDesc::tail_*): when the remainder is at most half a round of the
// CUs, q = CUs / remainder parts per tile give every CU the same share -- at least 6 K steps per part, at most 8 parts, and only
// within the capacities of the caller's workspace and counters.  max_full: most whole-round tiles for which the split is still
// taken (0: no limit).  Returns q (1: no split) and the first split tile in *full.
static inline int tail_split(const DmlConvDesc& d, const int ntiles, const int tile_rows, const int max_full, int* full_out) {
    *full_out = 0;
    if (!conv_has_tail(d)) return 1;
    const int full = ntiles / CUS * CUS, rem = ntiles - full;
    if (full < CUS || (max_full > 0 && full > max_full) || rem <= 0 || rem > CUS / 2) return 1;
    int q = CUS / rem;
    if (q > 8) q = 8;
    const int KTall = conv_ktot(d) / BK;
    while (q > 1 && KTall / q < 6) --q;
    if (q <= 1 || (int64_t)rem * q * tile_rows * 128 > d.tail_ws_elems || rem > d.tail_counters_len) return 1;
    *full_out = full;
    return q;
}

// the kernel, tiling and grid of a descriptor that passed validation: T = bf16_t (es 2) or float (es 4), MODE = mode
static inline int conv_choose_kernel(const DmlConvDesc& d, const ConvSwitches& sw, const int es, const int mode, const bool ws_ok,
                              const bool planes_ok, ConvChoice* c) {
    const int M = conv_m(d), Ktot = conv_ktot(d), N = d.N;
    const int64_t xb = conv_x_bytes(d, es), wb = conv_w_bytes(d, es);
    const bool small = xb < (1ll << 31) && wb < (1ll << 31);
    c->elem_bytes = es;
    c->mode = mode;
    c->x_bytes = small ? (uint32_t)xb : 0u;
    c->w_bytes = small ? (uint32_t)wb : 0u;
    const bool aligned = (d.C % BK) == 0 && d.R * d.S <= 32 && small;
    c->nblk_m = (M + 127) / 128;
    c->tail_full = 0;
    c->tail_q = 1;
    // non-temporal epilogue stores for outputs that do not fit the L2 anyway (st16); smaller ones are better left there for
    // their consumer (1x1 1024 -> 256 at 48 x 48, 19 MB: 45.3 us plain, 46.9 non-temporal).
    // the partial statistics (64 B per wave instruction) follow only where they are many: beside non-temporal outputs,
    // 19 MB of plain partial stores bring the stalls back (192 x 192, 64 -> 256: 158 us, 126 with both non-temporal; all
    // plain 141), while 4.7 MB do better plain (48 x 48, 256 -> 1024: 41.1 against 45.4 us)
    const bool nt_y = (int64_t)M * N * (int64_t)es >= (32ll << 20);
    const bool nt_p = nt_y && (int64_t)((M + 63) / 64) * N * 8 >= (8ll << 20);
    c->nt_out = (nt_y ? 1 : 0) | (nt_p ? 2 : 0);
    // LDS-DMA kernel: bf16, K tiles inside one tap, tensors addressable with a 31-bit byte offset.  With a 3-stage
    // ring (48 KB of LDS) and the 168-register budget three workgroups fit a CU like the register-staged kernel, and
    // it is the default for every eligible shape: whole train step 362.4 vs 356.4 images/s (three interleaved A/B
    // runs; a 4-stage ring on the largest grids only: 360.2).  In isolation the two kernels are within +-5 % of each
    // other (tools/bench_conv.py); the register-staged kernel stays for fp32, unaligned channel counts (stem, final
    // conv) and N <= 32.
    if (es == 2 && conv_dma_eligible(d, sw, xb, wb)) {
        c->kx_bytes = (uint32_t)xb;
        c->kw_bytes = (uint32_t)wb;
        // wave-specialised kernel (conv_ws_kernel): one persistent workgroup per CU on 144-row tiles, tile-major weights,
        // N a multiple of 128, enough tiles to fill the chip.  Same-box microbenchmarks against the ring kernel below
        // (profiles/r04_ws_probe_3.txt vs r04_ws_probe_1_shipped.txt): layer3 3x3 67.5 -> 43.6 us, 1x1 1024 -> 256
        // 37.6 -> 24.2, 1x1 256 -> 1024 38.4 -> 31.0, ASPP 3x3 385 -> 325-357, decoder 3x3 886 -> 825-870.
        if (ws_ok) {
            const bool wide = (N % 256) == 0;
            const int bm = wide ? 144 : 288;
            c->family = CONV_WS;
            c->mw = wide ? 1 : 2; c->nw = wide ? 4 : 2; c->pl = 1; c->mt = WS_MT; c->epi = 0;
            c->nblk_m = (M + bm - 1) / bm;
            c->nblk_n = N / (wide ? 256 : 128);
            const int ntiles = c->nblk_m * c->nblk_n;
            c->grid = ntiles < CUS ? ntiles : CUS;
            c->block = (4 + WS_NLD) * 64;
            return 0;
        }
        c->family = CONV_RING;
        c->block = NTHREADS;
        // grids that leave most of the chip idle (batch-1 inference, the anomaly model's down-scaled inputs): halve the
        // tile width to double the workgroup count; per-FLOP the 128 x 64 tile is 15-25 % slower, so only below 200
        // workgroups (1024 x 2048 bs 1: 235 -> 250 images/s, 5-scale open-set evaluation 92 -> 97.5 frames/s; the
        // training grids are all larger)
        const bool narrow = c->nblk_m * ((N + 127) / 128) < 200;
        // 256-row tiles pay where the K loop is long (3x3 convolutions over >= 256 channels: layer4 / ASPP / decoder),
        // with the K-split tail balancing their few tiles: in isolation ASPP 3x3 389 -> 343 us (1014 TFLOP/s), layer4
        // 3x3 202 -> 176 us, decoder 3x3 1003 -> 922 us.  On the short-K 1x1 layers three
        // workgroups of four waves hide latency better than two of eight (whole step -1.8 % with 256-row tiles
        // everywhere).  DML_CONV_BM256: 0 = never, 1 = this rule (default), 2 = every eligible layer,
        // >= 64 = the K threshold of the rule
        // In the plan (serial profile, r02 v3 -> v5): ASPP forward 1.14 -> 0.98 ms, ASPP data gradients 1.12 -> 1.01,
        // decoder forward 0.95 -> 0.86, layer4 3x3 -0.05; but layer3's 3x3 (K = 2304, only 288 tiles of 256 rows) LOSES
        // 0.24 ms over its 44 launches -- one 72-step tile per CU at two waves per SIMD -- hence the tile-count clause.
        const int tiles256 = ((M + 255) / 256) * (N / 128);
        const bool long_k = sw.bm256 >= 64 ? Ktot >= sw.bm256 : (Ktot >= 4608 || (Ktot >= 2304 && tiles256 >= 512));
        // The 256-row tile runs as 4 waves on 128 x 64 WAVE tiles (conv_igemm_dma_kernel<..., 256, 128>: 32 MFMAs per wave and
        // K step against 12 KB of fragment reads, half the barriers per FLOP); the 8-wave variant on 64 x 64 wave tiles it
        // replaced in round 3 (decoder 3x3 data gradient 1.064 -> 0.957 ms, whole step 385.3 -> 388.3 images/s) is gone.
        const bool rows256 = (sw.bm256 == 2 || (sw.bm256 != 0 && long_k)) && N >= 128 && !narrow && N % 128 == 0;
        c->bm = rows256 ? 256 : 128; c->tmw = rows256 ? 128 : 64; c->wpe = rows256 ? 2 : 3;
        if (rows256) {
            // whole tiles on the first multiple of 256 workgroups, the remainder split along K
            c->nblk_m = (M + 255) / 256;
            c->bn = 128;
        } else {
            c->bn = (N > 64 && !narrow) ? 128 : 64;
        }
        c->nblk_n = (N + c->bn - 1) / c->bn;
        const int ntiles = c->nblk_m * c->nblk_n;
        // (128-row tiles: only where the whole rounds are at most six -- beyond that the last round is a small share of the launch)
        if (c->bn == 128) c->tail_q = tail_split(d, ntiles, c->bm, rows256 ? 0 : 6 * CUS, &c->tail_full);
        c->grid = c->tail_q > 1 ? c->tail_full + (ntiles - c->tail_full) * c->tail_q : ntiles;
        return 0;
    }
    if (d.w_tiled) return DML_EUNSUPPORTED;      // tile-major weights: only the LDS-DMA kernels above read them
    if (es == 4 && planes_ok) {
        // fp32 tensors, products of two fp16 planes per operand on the matrix cores (DmlConvDesc.x_planes ...)
        const bool wide = (N % 256) == 0;
        // 64 output channels (layer1's 3x3, the 256 -> 64 1x1, the data gradients of the 64 -> 256 1x1): 192 x 64 tiles on four
        // 48 x 64 wave tiles.  On the 288 x 128 configuration half of every tile -- MFMAs and DMA pieces -- was empty
        // (r04: 0.16-0.17 of the class's own bound).  Same box, old -> new: 3x3 64 -> 64 at 192 x 192 forward 347 -> 286 us, 1x1
        // 256 -> 64 244 -> 185, 1x1 128 -> 64 190 -> 132; whole step +0.8 % (profiles/r05_ab_n64.txt)
        const bool n64 = N == 64;
        // Forward launches that leave most of the chip empty on 144-row tiles (batch-1 inference at 1024 x 2048: 57 row blocks on
        // layer3 / layer4 / ASPP; the small maps of the tests): 48 x 256 tiles -- three times the workgroups, each with a third
        // of the MFMAs per K step behind the same weight pieces.  (Round 6; 1024 x 2048 batch 1: see profiles/r06_infer_short_tiles.txt)
        const bool shortm = ws_planes_short(d, mode);
        const int bm = wide ? (shortm ? 48 : 144) : (n64 ? 192 : 288);
        c->family = CONV_WS;
        c->pl = 2;
        c->mw = wide ? 1 : (n64 ? 4 : 2); c->nw = wide ? 4 : (n64 ? 1 : 2);
        c->mt = (shortm || (n64 && !wide)) ? 3 : WS_MT;
        // data gradients: one instantiation per set of epilogue operands (conv_epilogue_rows_ops)
        c->epi = mode == 1 ? ((d.accum != 0 || d.res_dz != nullptr) ? 1 : 0) | (d.bnr_partials != nullptr ? 2 : 0) : 0;
        c->nblk_m = (M + bm - 1) / bm;
        c->nblk_n = wide ? N / 256 : (n64 ? 1 : (N + 127) / 128);      // (a last 128-wide block may be half empty: zero rows, no stores)
        const int ntiles = c->nblk_m * c->nblk_n;
        c->grid = ntiles < CUS ? ntiles : CUS;
        c->block = (4 + WS_NLD) * 64;
        c->kx_bytes = (uint32_t)conv_x_bytes(d, 2);
        c->kw_bytes = (uint32_t)conv_w_bytes(d, 2);
        return 0;
    }
    c->block = NTHREADS;
    if (es == 4 && conv_f32_split(d) && aligned && N > 32) {      // (f32_split == 2 launches the planes kernel did not take: three-term split)
        c->family = CONV_X3;
        c->bn = N > 64 ? 128 : 64;
    } else {
        if (mode == 2) return DML_EUNSUPPORTED;      // acc32: LDS-DMA kernels only (bf16, C % 32 == 0, N > 32)
        c->family = CONV_REG;
        c->bn = N > 64 ? 128 : (N > 32 ? 64 : 32);
        c->aligned = aligned ? 1 : 0;
    }
    c->nblk_n = (N + c->bn - 1) / c->bn;
    c->grid = c->nblk_m * c->nblk_n;
    return 0;
}

// Validation of a dml_conv_igemm descriptor and the choice of its launch.  0, or the DML_E* code dml_conv_igemm returns for it;
// c->stat_rows is set either way (DML_STAT_ROWS unless one of the wave-specialised kernels would take the launch).
static inline int conv_choose(const DmlConvDesc* dp, const ConvSwitches& sw, ConvChoice* c) {
    *c = ConvChoice{};
    c->stat_rows = DML_STAT_ROWS;
    if (!dp) return DML_EINVAL;
    const DmlConvDesc& d = *dp;
    // the two persistent kernels, which count their statistics groups in their own wave tiles
    const bool planes_ok = d.dtype == DML_F32 && conv_ws_planes_eligible(d, d.mode);
    bool ws_ok = false;
    if (d.dtype == DML_BF16) {
        const int64_t xb = conv_x_bytes(d, 2), wb = conv_w_bytes(d, 2);
        ws_ok = conv_dma_eligible(d, sw, xb, wb) && conv_ws_eligible(d, sw, xb, wb);
    }
    if (planes_ok) c->stat_rows = ws_planes_stat_rows(d, d.mode);
    else if (ws_ok) c->stat_rows = WS_STAT_ROWS;

    if (!d.x || !d.w || !d.y) return DML_EINVAL;
    if (d.dtype != DML_F32 && d.dtype != DML_BF16) return DML_EINVAL;
    const int vec = d.dtype == DML_BF16 ? 8 : 4;
    if (d.C % vec || d.ldx % vec) return DML_EALIGN;
    if (d.mode != 0 && d.mode != 1) return DML_EINVAL;
    if (d.mode == 1 && d.stride != 1 && d.stride != 2) return DML_EUNSUPPORTED;
    if (d.B <= 0 || d.Ho <= 0 || d.Wo <= 0 || d.N <= 0 || d.R <= 0 || d.S <= 0) return DML_EINVAL;
    if ((int64_t)d.B * d.Ho * d.Wo >= (1ll << 31)) return DML_EINVAL;
    if (d.stats && d.bias) return DML_EINVAL;
    const int f32_split = conv_f32_split(d);
    if (f32_split < 0 || f32_split > 2) return DML_EINVAL;
    if (conv_has_planes(d)) {
        if (!d.x_unscale || !d.w_unscale || d.x_plane_stride <= 0 || d.w_plane_stride <= 0 ||
            d.x_plane_stride >= (1ll << 30) || d.w_plane_stride >= (1ll << 30))
            return DML_EINVAL;
        if ((addr(d.x_planes) & 15) || (addr(d.w_planes) & 15) || (d.x_plane_stride & 7) || (d.w_plane_stride & 7)) return DML_EALIGN;
    }
    if (d.w_tiled && (d.dtype != DML_BF16 || d.C % BK || d.N % 64)) return DML_EUNSUPPORTED;
    if (d.acc32) {
        // fp32 staging of a gradient with several producers: the 16-byte-vector bf16 path of the data gradient only
        if (d.mode != 1 || d.dtype != DML_BF16 || d.y_f32 || d.accum || d.res_dz || d.bnr_partials) return DML_EINVAL;
        if (d.N % 8 || d.ldy % 8 || d.acc32_ld % 4 || (addr(d.y) & 15) || (addr(d.acc32) & 15) || d.N <= 32) return DML_EALIGN;
    }
    if (d.res_dz) {
        // masked residual gradient in the epilogue: the 16-byte-vector bf16 path of the data gradient only
        // (fp32: the two-plane kernel's row epilogue, 4-channel mask bytes; checked against the launch below)
        if (d.mode != 1 || d.y_f32 || d.accum || !d.res_mask) return DML_EINVAL;
        if (d.dtype == DML_BF16) {
            if (d.N % 8 || d.ldy % 8 || d.res_ld % 8 || (addr(d.y) & 15) || (addr(d.res_dz) & 15) || d.N <= 32) return DML_EALIGN;
            if ((d.N & 63) == 0 && (addr(d.res_mask) & 7)) return DML_EALIGN;      // 8-byte mask rows
        } else if (d.N % 64 || d.res_ld % 4 || ((addr(d.res_dz) | addr(d.res_mask)) & 15)) {
            return DML_EALIGN;      // (16 mask bytes per pixel row and 64 channels are one load)
        }
    }
    if (conv_has_tail(d) && (addr(d.tail_ws) & 15)) return DML_EALIGN;
    if (d.post_scale) {
        if (d.mode != 0 || !d.post_shift || !d.post_mean || d.stats || d.bias || d.accum || d.y_f32) return DML_EINVAL;
        if (d.post_res && (d.post_ldres % vec || (addr(d.post_res) & 15))) return DML_EALIGN;
    }
    if (d.bnr_partials) {
        // fused BN-backward reduce: data-gradient mode; bf16 result stored as 16-byte vectors, 8-channel mask bytes -- or fp32 on the
        // two-plane kernel (checked below, once the launch is described), 4-channel mask bytes
        if (d.mode != 1 || d.y_f32 || !d.bnr_y || !d.bnr_mean || !d.bnr_invstd || (d.bnr_relu && !d.bnr_mask)) return DML_EINVAL;
        if (d.dtype == DML_BF16) {
            if (d.N % 8 || d.ldy % 8 || d.bnr_ldy % 8 || (addr(d.y) & 15) || (addr(d.bnr_y) & 15) || (addr(d.bnr_partials) & 15) || d.N <= 32)
                return DML_EUNSUPPORTED;
            if (d.bnr_relu && (d.N & 63) == 0 && (addr(d.bnr_mask) & 7)) return DML_EALIGN;
        } else {
            if (d.N % 64 || d.bnr_ldy % 4) return DML_EUNSUPPORTED;
            if (((addr(d.bnr_y) | addr(d.bnr_partials) | addr(d.bnr_mean) | addr(d.bnr_invstd) | (d.bnr_relu ? addr(d.bnr_mask) : 0)) & 15) != 0)
                return DML_EALIGN;
        }
    }
    // (only the two-plane row epilogue with both operand sets knows the increment: an accumulating fp32 launch)
    if (d.bnr_partials && d.bnr_inc != 0 && (!d.accum || d.dtype != DML_F32 || d.res_dz)) return DML_EUNSUPPORTED;
    if (d.sub_grid) {
        // a parity class of a stride-2 data gradient: stride-1 geometry on dY's grid, the two-plane kernel's row epilogues only
        if (d.mode != 1 || d.stride != 1 || d.dil != 1 || d.Hi != d.Ho || d.Wi != d.Wo || (unsigned)d.sub_y > 1u || (unsigned)d.sub_x > 1u ||
            d.dtype != DML_F32)
            return DML_EINVAL;
        if ((int64_t)4 * d.B * d.Ho * d.Wo * (int64_t)d.ldy * 4 >= (1ll << 31)) return DML_EUNSUPPORTED;
    }
    const bool own_geometry = d.sub_grid || conv_pad_x(d) != d.pad;
    if (own_geometry && (d.dtype == DML_BF16 || d.acc32)) return DML_EUNSUPPORTED;
    if (d.acc32) return conv_choose_kernel(d, sw, 2, 2, ws_ok, false, c);
    if (d.dtype == DML_BF16) return conv_choose_kernel(d, sw, 2, d.mode, ws_ok, false, c);
    // fp32: only the two-plane kernel writes the BN-backward sums / adds the masked identity-branch gradient / maps a sub-grid
    if ((d.bnr_partials || d.res_dz || own_geometry) && !planes_ok) return DML_EUNSUPPORTED;
    // x == x_planes: the caller keeps this operand as fp16 planes ONLY (no fp32 tensor behind `x`).  Every other fp32 kernel would
    // read the planes as floats: refuse instead of falling back
    if (d.f32_split == 2 && d.x_planes && d.x == d.x_planes && !planes_ok) return DML_EUNSUPPORTED;
    return conv_choose_kernel(d, sw, 4, d.mode, false, planes_ok, c);
}

// ------------------------------------------------------------------------------------------------
// weight gradient
// ------------------------------------------------------------------------------------------------
enum WgradFamily {
    WGRAD_BIG = 0,      // conv_wgrad_big_kernel<WGRAD_DEPTH>: 256 x 256 output tiles
    WGRAD_WS,           // conv_wgrad_ws_kernel<LIN>: wave-specialised on planes, 128 x 256 tiles, persistent
    WGRAD_H2,           // conv_wgrad_h2_kernel<LIN>: planes, 128 x 128 tiles
    WGRAD_N64,          // conv_wgrad_n64_kernel: bf16, 64 x 256 tiles
    WGRAD_X3,           // conv_wgrad_x3_kernel<LIN>: three-term split
    WGRAD_PLAIN         // conv_wgrad_kernel<T>
};

struct ReduceLaunch {      // one wgrad_reduce_kernel launch
    int grid_x, grid_y, block, splits, slab_stride, fold_only;
};

struct WgradChoice {
    int family;
    int lin;                          // LIN: 1x1, stride 1, no padding
    int elem_bytes;                   // PLAIN: T
    bool planes;                      // the fp16 planes of the descriptor are in effect (WgradArgs::x_planes ...)
    bool use_ws;                      // WgradArgs::ws = the descriptor's workspace (false: atomics)
    int tiles, cm;                    // pixel tiles of 32; un-padded input channels of dw
    int nblk_n, nblk_k, splitk, slab_tiles;
    int grid, block;
    uint32_t x_bytes, dy_bytes;       // BIG, WS, H2, X3: the kernel's extent arguments
    int nitems;                       // WS
    int64_t nrs;                      // N * R * S
    int nreduce;
    ReduceLaunch reduce[2];
};

static inline int64_t wgrad_m(const DmlWgradDesc& d) { return (int64_t)d.B * d.Ho * d.Wo; }
static inline int wgrad_ktot(const DmlWgradDesc& d) { return mul32(mul32(d.R, d.S), d.C); }
static inline int64_t wgrad_x_bytes(const DmlWgradDesc& d, const int es) { return operand_bytes(d.B, d.Hi, d.Wi, d.ldx, d.C, es); }
static inline int64_t wgrad_dy_bytes(const DmlWgradDesc& d, const int es) { return ((wgrad_m(d) - 1) * d.ldy + d.N) * es; }

// May this bf16 job run on the 256 x 256-tile kernel?  Whole 256-channel output tiles, everything addressable with 31-bit byte
// offsets and 24-bit pixel indices.  Measured (tools/bench_conv.py wgrad, incl. the reduce pass, vs the 128 x 128 kernel):
// decoder 3x3 320->256 @192^2 970 vs 727 TFLOP/s, 3x3 512->512 d2 879 vs 669, ASPP 3x3 2048->256 857 vs 693,
// layer3 3x3 256->256 569 vs 500.  With 4 output tiles (the 1x1 256<->1024 layers) filling 256 CUs would take 64
// splits and the slab traffic eats the gain, so those run as 128 workgroups (32 splits): standalone that is a
// few % slower than the small-tile kernel, but the weight gradients share the chip with the main stream and what
// counts there is CU-time -- whole step +0.75 % (3 interleaved A/B runs of bench.py).
// Shared by dml_conv_wgrad (single job, which has validated the descriptor) and the grouped launch (group: the whole
// descriptor is checked here, and a weight tensor below 64 K elements stays out).
static inline bool wgrad_big_eligible(const DmlWgradDesc* d, const bool group) {
    if (!d) return false;
    const int64_t M = wgrad_m(*d), Ktot = (int64_t)d->R * d->S * d->C, tiles = (M + BK - 1) / BK;
    if (group) {
        if (!d->x || !d->dy || !d->dw) return false;
        if (d->C % 8 || d->ldx % 8 || d->N % 8 || d->ldy % 8) return false;
        if ((d->Cm > 0 ? d->Cm : d->C) > d->C) return false;
        if ((int64_t)d->N * Ktot < 65536) return false;
    }
    return d->dtype == DML_BF16 && d->N % 256 == 0 && (d->N / 256) * ((Ktot + 255) / 256) >= 4 && tiles >= 16 &&
           wgrad_x_bytes(*d, 2) < (1ll << 31) && wgrad_dy_bytes(*d, 2) < (1ll << 31) && (int64_t)(d->B + 1) * d->Hi * d->Wi < (1 << 24) &&
           M < (1 << 24) && d->ldx < (1 << 22) && d->ldy < (1 << 22);
}

// Split count of the pixel dimension for a kernel that fills rounds of workgroups: among 1 .. tiles / min_steps candidate counts
// (at most 256, and what the workspace holds) the one whose slabs score best, the fewest splits on ties.  score(slab, real):
// larger is better, slab = pixel tiles per split, real = the splits that slab size leaves.
template <class Score>
static inline int pick_splits(const int tiles, const int min_steps, const int64_t plane, const int64_t ws_elems, Score score) {
    int smax = tiles / min_steps;
    if (smax > 256) smax = 256;
    if ((int64_t)smax * plane > ws_elems) smax = (int)(ws_elems / plane);
    if (smax < 1) smax = 1;
    double best = -1e30;
    int sk = 1;
    for (int c = 1; c <= smax; ++c) {
        const int slab = (tiles + c - 1) / c;
        const int real = (tiles + slab - 1) / slab;
        const double s = score(slab, real);
        if (s > best + 1e-9) { best = s; sk = real; }
    }
    return sk;
}
// the kernels on one workgroup per (output tile, split): measured (tools/bench_conv.py): >= 512 workgroups and ~48 K tiles per
// workgroup with a workspace, >= 1024 workgroups on atomics; at least 8 K tiles per workgroup
static inline int flat_splits(const int base, const int tiles, const bool use_ws) {
    int splitk = use_ws ? (512 + base - 1) / base : (1024 + base - 1) / base;
    if (use_ws && tiles / 48 > splitk) splitk = tiles / 48;
    const int cap = (tiles + 7) / 8;
    if (splitk > cap) splitk = cap;
    if (splitk < 1) splitk = 1;
    return splitk;
}
// a split count within the workspace and the pixel tiles, the tiles per split, and the splits those leave (0: the workspace does
// not hold one slab)
static inline int finish_splits(int sk, const int tiles, const bool use_ws, const int64_t plane, const int64_t ws_elems, int* slab_tiles) {
    if (use_ws && (int64_t)sk * plane > ws_elems) sk = (int)(ws_elems / plane);
    if (use_ws && sk < 1) return 0;
    if (sk > tiles) sk = tiles > 0 ? tiles : 1;
    *slab_tiles = (tiles + sk - 1) / sk;
    return (tiles + *slab_tiles - 1) / *slab_tiles;
}

// Validation of a dml_conv_wgrad descriptor and the choice of its launches.  0, or the DML_E* code dml_conv_wgrad returns for it.
static inline int wgrad_choose(const DmlWgradDesc* dp, WgradChoice* c) {
    *c = WgradChoice{};
    if (!dp || !dp->x || !dp->dy || !dp->dw) return DML_EINVAL;
    const DmlWgradDesc& d = *dp;
    if (d.dtype != DML_F32 && d.dtype != DML_BF16) return DML_EINVAL;
    const int vec = d.dtype == DML_BF16 ? 8 : 4;
    if (d.C % vec || d.ldx % vec || d.N % vec || d.ldy % vec) return DML_EALIGN;
    if (wgrad_m(d) >= (1ll << 31)) return DML_EINVAL;
    const int M = (int)wgrad_m(d), Ktot = wgrad_ktot(d), N = d.N;
    if (d.dtype == DML_F32 && d.f32_split == 2 && d.x_planes && d.dy_planes) {
        if (!d.x_unscale || !d.dy_unscale || d.x_plane_stride <= 0 || d.dy_plane_stride <= 0) return DML_EINVAL;
        if ((addr(d.x_planes) & 15) || (addr(d.dy_planes) & 15) || (d.x_plane_stride & 7) || (d.dy_plane_stride & 7)) return DML_EALIGN;
        // fp16 vectors of 8: C, N, pitches multiples of 8; both planes within 31-bit offsets
        c->planes = d.C % 8 == 0 && d.N % 8 == 0 && d.ldx % 8 == 0 && d.ldy % 8 == 0 &&
                    wgrad_x_bytes(d, 2) + d.x_plane_stride * 2 < 0x7fffffffll && wgrad_dy_bytes(d, 2) + d.dy_plane_stride * 2 < 0x7fffffffll;
    }
    // x == x_planes / dy == dy_planes: that operand exists as fp16 planes ONLY -- the fp32 kernels below must not read it as floats
    if (!c->planes && ((d.x_planes && d.x == d.x_planes) || (d.dy_planes && d.dy == d.dy_planes))) return DML_EUNSUPPORTED;
    const int tiles = c->tiles = (M + BK - 1) / BK;
    const int cm = c->cm = d.Cm > 0 ? d.Cm : d.C;
    if (cm > d.C) return DML_EINVAL;
    if (cm != d.C && !d.ws) return DML_EINVAL;      // dropping padded channels needs the workspace path
    const int64_t plane = (int64_t)N * Ktot;
    // With a workspace every weight gradient is a fixed-order sum of slabs: the train step is bitwise reproducible.  (Small
    // weight tensors -- below 64 K elements -- used to take fp32 atomics instead, the reduce pass being latency-bound there.)
    // Without a workspace: atomics.
    const bool use_ws = c->use_ws = d.ws != nullptr;
    c->lin = (d.R == 1 && d.S == 1 && d.stride == 1 && d.pad == 0) ? 1 : 0;
    c->nrs = (int64_t)N * d.R * d.S;
    c->block = NTHREADS;
    int sk = d.splitk, rblock = 256, rmax = 256 * 8;
    if (use_ws && wgrad_big_eligible(dp, false)) {
        c->family = WGRAD_BIG;
        c->nblk_n = N / 256;
        c->nblk_k = (Ktot + 255) / 256;
        const int base = c->nblk_n * c->nblk_k;
        // one workgroup per CU: pick the split count that fills whole rounds of 256 (128) workgroups best,
        // fewest splits on ties (less slab traffic); at least 8 K steps per workgroup
        if (sk <= 0)
            sk = pick_splits(tiles, 8, plane, d.ws_elems, [&](const int, const int real) {
                const int blocks = base * real;
                const int rnd = base < 6 ? 128 : 256;
                return (double)blocks / (double)(((blocks + rnd - 1) / rnd) * rnd);
            });
        c->block = WB_THREADS;
        c->x_bytes = (uint32_t)wgrad_x_bytes(d, 2);
        c->dy_bytes = (uint32_t)wgrad_dy_bytes(d, 2);
    } else if (c->planes && use_ws && N % WGW_TN == 0 && tiles >= 16 && (addr(d.ws) & 15) == 0) {
        // wave-specialised kernel on planes: 128 x 256 output tiles, persistent workgroups over (tile, slab) items.  Against
        // conv_wgrad_h2_kernel in isolation (same box, tools/bench_h2.py wgrad): 3x3 256 -> 256 167-176 -> 149 us, 1x1 1024 <-> 256
        // 76-83 -> 69-71, ASPP 3x3 1070-1147 -> 939, 3x3 512 -> 512 563 -> 473, decoder 3x3 2614-2724 -> 2532; in the train step,
        // where the weight gradients share the chip with the main stream, the step is unchanged (183.6 vs 183.2 images/s, three
        // interleaved pairs): DESIGN.md section 5, round 4
        c->family = WGRAD_WS;
        c->nblk_n = N / WGW_TN;
        c->nblk_k = (Ktot + WGW_TK - 1) / WGW_TK;
        const int base = c->nblk_n * c->nblk_k;
        // the split count with the smallest modelled time: rounds of 256 workgroups x (K steps of an item x 1.45 us + 8 us for
        // its 128 KB slab store and the restart of the K loop) + the fold pass over the slabs (written and read once, ~4 TB/s);
        // >= 16 K steps per item.  (Round 4 maximised the filling of the rounds alone and took 71 slabs of 16 steps for 3x3
        // 256 -> 256 -- five rounds, a third of each an epilogue, 335 MB of slabs -- where 14 slabs of 83 steps fill one round.)
        if (sk <= 0)
            sk = pick_splits(tiles, 16, plane, d.ws_elems, [&](const int slab, const int real) {
                const int items = base * real;
                return -((double)((items + 255) / 256) * (slab * 1.45 + 8.0) + (double)real * (double)plane * 8.0 / 4.0e6);
            });
        c->block = (4 + WGW_NLD) * 64;
        c->x_bytes = (uint32_t)wgrad_x_bytes(d, 2);
        c->dy_bytes = (uint32_t)wgrad_dy_bytes(d, 2);
        // (one-wave blocks for the fold: they start beside the persistent data-gradient workgroups of the other stream instead of
        // waiting for one to retire -- 28.6 us per launch in the overlapped trace against 9.8 alone, 122 launches per step; see
        // dml_bn_bwd_apply)
        rblock = 64;
        rmax = 256 * 8 * (256 / rblock);
    } else {
        // N <= 64 (bf16): 64 x 256 tiles instead of half-empty 128 x 128 ones
        // (measured, tools/bench_conv.py wgrad at 192 x 192: 3x3 64 -> 64 164 -> 160 us; the 1x1 layers are bound by the
        // operand loads, not by the idle MFMA rows, and LOSE 20 % with the wider x tile -- they stay on the 128 x 128 kernel)
        const bool n64 = d.dtype == DML_BF16 && N <= 64 && d.R * d.S > 1;
        c->nblk_n = n64 ? 1 : (N + 127) / 128;
        c->nblk_k = n64 ? (Ktot + 255) / 256 : (Ktot + 127) / 128;
        if (sk <= 0) sk = flat_splits(c->nblk_n * c->nblk_k, tiles, use_ws);
        // split-product kernel: operands through buffer descriptors (32-bit byte offsets)
        const int64_t x3_xb = wgrad_x_bytes(d, 4), x3_yb = wgrad_dy_bytes(d, 4);
        if (c->planes) {
            c->family = WGRAD_H2;
            c->x_bytes = (uint32_t)wgrad_x_bytes(d, 2);
            c->dy_bytes = (uint32_t)wgrad_dy_bytes(d, 2);
        } else if (n64) {
            c->family = WGRAD_N64;
        } else if (d.dtype == DML_F32 && d.f32_split && x3_xb < (int64_t)0x7fffffff && x3_yb < (int64_t)0x7fffffff) {
            c->family = WGRAD_X3;
            c->x_bytes = (uint32_t)x3_xb;
            c->dy_bytes = (uint32_t)x3_yb;
        } else {
            c->family = WGRAD_PLAIN;
            c->elem_bytes = d.dtype == DML_BF16 ? 2 : 4;
        }
    }
    sk = c->splitk = finish_splits(sk, tiles, use_ws, plane, d.ws_elems, &c->slab_tiles);
    if (sk < 1) return DML_EINVAL;
    c->grid = c->nblk_n * c->nblk_k * sk;
    if (c->family == WGRAD_WS) {
        // (one item per workgroup instead of persistent workgroups, with and without a high-priority main stream: no change of the
        // overlapped step, 83.4-83.9 ms in every combination, serial 86.1 -- profiles/r05_ab_wgrad_nonpersist_priority.txt)
        c->nitems = c->grid;
        c->grid = c->nitems < 256 ? c->nitems : 256;
    }
    if (use_ws) {
        const int gx = blocks_for(c->nrs * cm, rblock, rmax);
        // small tensors with very many splits: fold chunks of 16 splits first (two launches, see wgrad_reduce_kernel)
        const int ychunks = (c->family != WGRAD_BIG && c->family != WGRAD_WS && c->nrs * cm < 65536 && sk > 64) ? (sk + 15) / 16 : 1;
        if (ychunks > 1) {
            c->nreduce = 2;
            c->reduce[0] = ReduceLaunch{gx, ychunks, rblock, sk, 1, 1};
            c->reduce[1] = ReduceLaunch{gx, 1, rblock, ychunks, 16, 0};
        } else {
            c->nreduce = 1;
            c->reduce[0] = ReduceLaunch{gx, 1, rblock, sk, 1, 0};
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Several weight gradients in one launch of the 256 x 256-tile kernel + one fold launch: the shared workspace is partitioned
// here.  Splits are chosen so that the launch is one round of <= 256 workgroups with about the same number of pixel tiles per
// workgroup in every job.
// ------------------------------------------------------------------------------------------------
struct WgradGroupChoice {
    int n;
    int nblk_n[WG_MAX_JOBS], nblk_k[WG_MAX_JOBS], splitk[WG_MAX_JOBS], slab_tiles[WG_MAX_JOBS], cm[WG_MAX_JOBS];
    uint32_t x_bytes[WG_MAX_JOBS], dy_bytes[WG_MAX_JOBS];
    int64_t ws_off[WG_MAX_JOBS], nrs[WG_MAX_JOBS];      // first float of each job's slabs in the workspace; N * R * S
    int start[WG_MAX_JOBS + 1];                         // first workgroup of each job in the launch
    int grid, block;
    int rgrid_x, rgrid_y, rblock;                       // wgrad_reduce_group_kernel
};

static inline int wgrad_group_choose(const DmlWgradDesc* const* descs, const int n, const void* ws, const int64_t ws_elems, WgradGroupChoice* g) {
    *g = WgradGroupChoice{};
    if (!descs || n <= 0 || n > WG_MAX_JOBS || !ws) return DML_EINVAL;
    int base[WG_MAX_JOBS], tiles[WG_MAX_JOBS], sk[WG_MAX_JOBS];
    int64_t plane[WG_MAX_JOBS];
    double work = 0.0;
    int tbase = 0;
    for (int j = 0; j < n; ++j) {
        const DmlWgradDesc* d = descs[j];
        if (!wgrad_big_eligible(d, true)) return DML_EUNSUPPORTED;
        const int Ktot = wgrad_ktot(*d);
        g->nblk_n[j] = d->N / 256;
        g->nblk_k[j] = (Ktot + 255) / 256;
        base[j] = g->nblk_n[j] * g->nblk_k[j];
        tiles[j] = ((int)wgrad_m(*d) + BK - 1) / BK;
        plane[j] = (int64_t)d->N * Ktot;
        work += (double)base[j] * tiles[j];
        tbase += base[j];
        g->x_bytes[j] = (uint32_t)wgrad_x_bytes(*d, 2);
        g->dy_bytes[j] = (uint32_t)wgrad_dy_bytes(*d, 2);
    }
    const int budget = tbase <= 256 ? 256 : ((tbase + 255) / 256) * 256;
    int blocks = 0;
    for (int j = 0; j < n; ++j) {
        int s = (int)((double)tiles[j] * budget / work);             // equal pixel tiles per workgroup
        const int cap = tiles[j] / 8 > 0 ? tiles[j] / 8 : 1;          // at least 8 K steps per workgroup
        if (s > cap) s = cap;
        if (s < 1) s = 1;
        sk[j] = s;
        blocks += base[j] * s;
    }
    // hand the remaining workgroups of the round to the jobs whose workgroups are the longest
    for (;;) {
        int best = -1;
        double longest = 0.0;
        for (int j = 0; j < n; ++j) {
            const double per = (double)tiles[j] / sk[j];
            if (blocks + base[j] <= budget && sk[j] < tiles[j] / 8 && per > longest) { longest = per; best = j; }
        }
        if (best < 0) break;
        ++sk[best];
        blocks += base[best];
    }
    int64_t off = 0, max_items = 0;
    g->n = n;
    g->start[0] = 0;
    for (int j = 0; j < n; ++j) {
        const DmlWgradDesc* d = descs[j];
        g->slab_tiles[j] = (tiles[j] + sk[j] - 1) / sk[j];
        g->splitk[j] = (tiles[j] + g->slab_tiles[j] - 1) / g->slab_tiles[j];
        if (off + (int64_t)g->splitk[j] * plane[j] > ws_elems) return DML_EINVAL;      // workspace too small for this group
        g->ws_off[j] = off;
        g->start[j + 1] = g->start[j] + base[j] * g->splitk[j];
        g->cm[j] = d->Cm > 0 ? d->Cm : d->C;
        g->nrs[j] = (int64_t)d->N * d->R * d->S;
        if (g->nrs[j] * g->cm[j] > max_items) max_items = g->nrs[j] * g->cm[j];
        off += (int64_t)g->splitk[j] * plane[j];
    }
    g->grid = g->start[n];
    g->block = WB_THREADS;
    g->rgrid_x = blocks_for(max_items, 256, 1024);
    g->rgrid_y = n;
    g->rblock = 256;
    return 0;
}

}  // namespace conv_choice
