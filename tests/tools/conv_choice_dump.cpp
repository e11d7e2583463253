// Prints what csrc/conv_choice.h chooses for a table of descriptors: host only, no GPU, nothing dereferenced.
// (tests/test_conv_choice.py compiles this, feeds it tests/golden/conv_choice_cases.json.gz as one line per case, and compares every field
// with what the library launched for the same descriptor before the choice was separated from the launch.)
//
// stdin, one case per line, whitespace separated, every field a decimal integer (pointers as addresses), struct order:
//   <id> C <v1> <bm256> <ws> <DmlConvDesc fields>
//   <id> W <DmlWgradDesc fields>
//   <id> G <n> <ws address> <ws_elems> <n x DmlWgradDesc fields>
// stdout: "<id> rc=<code> key=value ..." per case.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../open-world-semantic-segmentation_amd/csrc/conv_choice.h"

namespace cc = conv_choice;

static long long tok(std::istream& s) {
    long long v = 0;
    s >> v;
    return v;
}
#define P(f) d.f = reinterpret_cast<decltype(d.f)>((uintptr_t)tok(s));
#define I(f) d.f = (decltype(d.f))tok(s);

static DmlConvDesc read_conv(std::istream& s) {
    DmlConvDesc d{};
    P(x) P(w) P(y) P(bias) P(stats)
    I(B) I(Hi) I(Wi) I(C) I(ldx) I(Ho) I(Wo) I(N) I(ldy) I(R) I(S) I(stride) I(dil) I(pad) I(dtype) I(y_f32) I(accum) I(mode)
    P(bnr_y) P(bnr_mask) P(bnr_mean) P(bnr_invstd) P(bnr_partials) I(bnr_ldy) I(bnr_relu)
    P(post_scale) P(post_shift) P(post_mean) P(post_res) I(post_ldres) I(post_relu)
    P(tail_ws) I(tail_ws_elems) P(tail_counters) I(tail_counters_len) I(tail_reserved)
    P(res_dz) P(res_mask) I(res_ld) I(res_reserved)
    P(acc32) I(acc32_ld) I(f32_split) I(w_tiled) I(ws_min_tiles)
    P(x_planes) P(w_planes) P(x_unscale) P(w_unscale) I(x_plane_stride) I(w_plane_stride) P(bnr_gmax)
    I(sub_grid) I(sub_y) I(sub_x) I(pad_w_set) I(pad_w) I(bnr_inc)
    return d;
}

static DmlWgradDesc read_wgrad(std::istream& s) {
    DmlWgradDesc d{};
    P(x) P(dy) P(dw)
    I(B) I(Hi) I(Wi) I(C) I(ldx) I(Ho) I(Wo) I(N) I(ldy) I(R) I(S) I(stride) I(dil) I(pad) I(dtype) I(splitk) I(Cm)
    P(ws) I(ws_elems) I(f32_split) I(reserved)
    P(x_planes) P(dy_planes) P(x_unscale) P(dy_unscale) I(x_plane_stride) I(dy_plane_stride)
    return d;
}

static std::string conv_kernel_name(const cc::ConvChoice& c) {
    char b[128];
    const char* t = c.elem_bytes == 2 ? "bf16" : "f32";
    switch (c.family) {
    case cc::CONV_REG: snprintf(b, sizeof b, "conv_igemm_kernel<%s,%d,%d,%d>", t, c.bn, c.aligned, c.mode); break;
    case cc::CONV_RING: snprintf(b, sizeof b, "conv_igemm_dma_kernel<%d,%d,3,%d,%d,%d>", c.bn, c.mode, c.wpe, c.bm, c.tmw); break;
    case cc::CONV_WS: snprintf(b, sizeof b, "conv_ws_kernel<%d,%d,%d,%d,%d,%d,%d>", c.mw, c.nw, c.mode, cc::WS_NLD, c.pl, c.mt, c.epi); break;
    case cc::CONV_X3: snprintf(b, sizeof b, "conv_igemm_x3_kernel<%d,%d>", c.bn, c.mode); break;
    default: snprintf(b, sizeof b, "?"); break;
    }
    return b;
}

static std::string wgrad_kernel_name(const cc::WgradChoice& c) {
    char b[128];
    switch (c.family) {
    case cc::WGRAD_BIG: snprintf(b, sizeof b, "conv_wgrad_big_kernel<2>"); break;
    case cc::WGRAD_WS: snprintf(b, sizeof b, "conv_wgrad_ws_kernel<%d>", c.lin); break;
    case cc::WGRAD_H2: snprintf(b, sizeof b, "conv_wgrad_h2_kernel<%d>", c.lin); break;
    case cc::WGRAD_N64: snprintf(b, sizeof b, "conv_wgrad_n64_kernel"); break;
    case cc::WGRAD_X3: snprintf(b, sizeof b, "conv_wgrad_x3_kernel<%d>", c.lin); break;
    case cc::WGRAD_PLAIN: snprintf(b, sizeof b, "conv_wgrad_kernel<%s>", c.elem_bytes == 2 ? "bf16" : "f32"); break;
    default: snprintf(b, sizeof b, "?"); break;
    }
    return b;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream s(line);
        std::string id, kind;
        if (!(s >> id >> kind)) continue;
        if (kind == "C") {
            cc::ConvSwitches sw;
            sw.v1 = tok(s) != 0;
            sw.bm256 = (int)tok(s);
            sw.ws = (int)tok(s);
            const DmlConvDesc d = read_conv(s);
            cc::ConvChoice c;
            const int rc = cc::conv_choose(&d, sw, &c);
            printf("%s rc=%d rows=%d", id.c_str(), rc, c.stat_rows);
            if (rc == 0)
                printf(" k=%s grid=%d block=%d nblk_m=%d nblk_n=%d tail_full=%d tail_q=%d nt_out=%d xb=%u wb=%u kxb=%u kwb=%u",
                       conv_kernel_name(c).c_str(), c.grid, c.block, c.nblk_m, c.nblk_n, c.tail_full, c.tail_q, c.nt_out, c.x_bytes,
                       c.w_bytes, c.kx_bytes, c.kw_bytes);
            printf("\n");
        } else if (kind == "W") {
            const DmlWgradDesc d = read_wgrad(s);
            cc::WgradChoice c;
            const int rc = cc::wgrad_choose(&d, &c);
            printf("%s rc=%d", id.c_str(), rc);
            if (rc == 0) {
                printf(" k=%s grid=%d block=%d nblk_n=%d nblk_k=%d splitk=%d slab_tiles=%d ws=%d planes=%d xb=%u yb=%u nitems=%d",
                       wgrad_kernel_name(c).c_str(), c.grid, c.block, c.nblk_n, c.nblk_k, c.splitk, c.slab_tiles, c.use_ws ? 1 : 0,
                       c.planes ? 1 : 0, c.x_bytes, c.dy_bytes, c.nitems);
                for (int i = 0; i < c.nreduce; ++i)
                    printf(" reduce%d=%dx%d/%d/%d/%" PRId64 "/%d/%d/%d/%d", i, c.reduce[i].grid_x, c.reduce[i].grid_y, c.reduce[i].block,
                           c.reduce[i].splits, c.nrs, c.cm, d.C, c.reduce[i].slab_stride, c.reduce[i].fold_only);
            }
            printf("\n");
        } else if (kind == "G") {
            const int n = (int)tok(s);
            const void* ws = reinterpret_cast<const void*>((uintptr_t)tok(s));
            const int64_t ws_elems = tok(s);
            DmlWgradDesc jobs[64];
            const DmlWgradDesc* ptrs[64];
            for (int j = 0; j < n && j < 64; ++j) {
                jobs[j] = read_wgrad(s);
                ptrs[j] = &jobs[j];
            }
            cc::WgradGroupChoice g;
            const int rc = cc::wgrad_group_choose(ptrs, n, ws, ws_elems, &g);
            printf("%s rc=%d", id.c_str(), rc);
            if (rc == 0) {
                printf(" k=conv_wgrad_group_kernel<2> grid=%d block=%d reduce=%dx%d/%d", g.grid, g.block, g.rgrid_x, g.rgrid_y, g.rblock);
                for (int j = 0; j < n; ++j)
                    printf(" job%d=%d/%d/%d/%d/%d/%u/%u/%" PRId64 "/%d/%d/%" PRId64, j, g.nblk_n[j], g.nblk_k[j], g.splitk[j], g.slab_tiles[j],
                           g.start[j], g.x_bytes[j], g.dy_bytes[j], g.ws_off[j], g.cm[j], jobs[j].C, g.nrs[j]);
            }
            printf("\n");
        }
    }
    return 0;
}
