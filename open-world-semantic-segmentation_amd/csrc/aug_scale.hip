// Scale / resize / pad / crop stage of the train and --crop_val transforms (utils/ext_transforms.py:95-146, 328-428, 68-92 of
// the reference), Pillow-exact, for a batch of uint8 NHWC frames: per sample a VIRTUAL image -- the frame resized to (Hs, Ws) --
// and a th x tw window of it whose origin may be negative and whose extent may pass the far edge; a pixel outside the virtual
// image is 0 (padding, pad_if_needed, crop and centre crop all reduce to that window on the host).  Image: Pillow's two-pass
// 8-bit BILINEAR resampler (see image_resize.hip and the header); label: a gather through the host's NEAREST index tables.
// One launch for the batch: a workgroup owns (sample, band of window rows, 64 window columns), runs the horizontal pass over
// exactly the source rows the band's vertical taps read into LDS (uint8, packed RGB per dword), then the vertical pass from LDS,
// and writes the uint8 window with 12-byte stores.  Every source index comes from a host table; the kernel still clamps each of
// them to the frame, so that a bad table reads a wrong pixel, never a stray address.
#include "common.h"

namespace {

constexpr int TPB = 256;          // threads per workgroup
constexpr int TW = 64;            // window columns per workgroup
constexpr int MAX_LDS_ROWS = 256; // 64 KiB of intermediate rows
constexpr int PREC = 22;          // fraction bits of the fixed-point weights (Resample.c PRECISION_BITS)

// Resample.c clip8: (acc >> 22) clamped to [0, 255] (arithmetic shift).  The empty asm keeps the shift and the clamp apart:
// fused, hipcc pairs two of them into v_ashr_pk_u8_i32 and then ORs the 16-bit result as if the upper half of the destination
// were zero, which it is not (seen as wrong blue bytes of every third pixel of a thread on the byte-store path).
__device__ __forceinline__ uint32_t clip8(int32_t acc) {
    int32_t v = acc >> PREC;
    asm volatile("" : "+v"(v));
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct __attribute__((aligned(4))) Rgb4 {   // four RGB pixels = three dwords
    uint32_t a, b, c;
};

__global__ __launch_bounds__(TPB) void aug_scale_window_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lbl,
                                                                const DmlScaleWindow* __restrict__ samples,
                                                                const int32_t* __restrict__ tables, int64_t table_len,
                                                                uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_lbl, int H,
                                                                int W, int th, int tw, int band_rows, int lds_rows, int tiles_x,
                                                                int tiles_y) {
    extern __shared__ uint32_t inter[];                      // [lds_rows][TW] packed R | G << 8 | B << 16
    const int t = (int)blockIdx.x;
    const int b = t / (tiles_x * tiles_y), tb = t - b * (tiles_x * tiles_y);
    const int ty = tb / tiles_x, tx = tb - ty * tiles_x;
    const DmlScaleWindow s = samples[b];
    // the sample's tables lie inside the table buffer, or the workgroup writes nothing
    const int64_t kh = s.kh, kv = s.kv;
    if (kh <= 0 || kv <= 0 || s.hbounds < 0 || s.hcoef < 0 || s.vbounds < 0 || s.vcoef < 0 || s.lrow < 0 || s.lcol < 0 ||
        s.hbounds + 2ll * tw > table_len || s.hcoef + kh * tw > table_len || s.vbounds + 2ll * th > table_len ||
        s.vcoef + kv * th > table_len || s.lrow + (int64_t)th > table_len || s.lcol + (int64_t)tw > table_len)
        return;
    const int32_t* hbounds = tables + s.hbounds;
    const int32_t* hcoef = tables + s.hcoef;
    const int32_t* vbounds = tables + s.vbounds;
    const int32_t* vcoef = tables + s.vcoef;
    const uint8_t* src_img = img + (int64_t)b * H * W * 3;
    const int y0 = ty * band_rows, y1 = min(y0 + band_rows, th);
    const int x0 = tx * TW;
    const int r0 = min(max(vbounds[2 * y0], 0), H);
    const int r1 = min(max(vbounds[2 * (y1 - 1)] + vbounds[2 * (y1 - 1) + 1], r0), H);
    const int nrows = min(r1 - r0, lds_rows);                // the host sized lds_rows to cover every band

    // horizontal pass: intermediate rows r0..r1-1, window columns x0..x0+63
    for (int idx = threadIdx.x; idx < nrows * TW; idx += TPB) {
        const int r = idx / TW, xc = idx - r * TW, x = x0 + xc;
        if (x >= tw) continue;
        const int xmin = hbounds[2 * x];
        int n = min(hbounds[2 * x + 1], (int)kh);
        if (xmin < 0 || xmin + n > W) n = 0;
        const int32_t* k = hcoef + (int64_t)x * kh;
        const uint8_t* src = src_img + ((int64_t)(r0 + r) * W + xmin) * 3;
        int32_t a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        for (int q = 0; q < n; ++q) {
            const int32_t c = k[q];
            a0 += (int32_t)src[3 * q] * c;
            a1 += (int32_t)src[3 * q + 1] * c;
            a2 += (int32_t)src[3 * q + 2] * c;
        }
        inter[r * TW + xc] = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16);
    }
    __syncthreads();

    // vertical pass: 16 groups of 4 columns x 16 rows at a time
    const int xg = (threadIdx.x & 15) * 4, x = x0 + xg;
    if (x >= tw) return;
    const bool vec = (tw & 3) == 0;                          // then x + 3 < tw and every row starts on a dword
    uint8_t* oimg = out_img + (int64_t)b * th * tw * 3;
    for (int y = y0 + (threadIdx.x >> 4); y < y1; y += TPB / 16) {
        const int ymin = vbounds[2 * y] - r0;
        int n = min(vbounds[2 * y + 1], (int)kv);
        if (ymin < 0 || ymin + n > nrows) n = 0;
        const int32_t* k = vcoef + (int64_t)y * kv;
        int32_t acc[4][3];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 1 << (PREC - 1);
        for (int q = 0; q < n; ++q) {
            const int32_t c = k[q];
            const uint4 p = *reinterpret_cast<const uint4*>(inter + (ymin + q) * TW + xg);
            const uint32_t pe[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e][0] += (int32_t)(pe[e] & 255u) * c;
                acc[e][1] += (int32_t)((pe[e] >> 8) & 255u) * c;
                acc[e][2] += (int32_t)((pe[e] >> 16) & 255u) * c;
            }
        }
        uint32_t px[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = clip8(acc[e][0]) | (clip8(acc[e][1]) << 8) | (clip8(acc[e][2]) << 16);
        uint8_t* o = oimg + ((int64_t)y * tw + x) * 3;
        if (vec) {
            Rgb4 v;
            v.a = px[0] | (px[1] << 24);
            v.b = (px[1] >> 8) | (px[2] << 16);
            v.c = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<Rgb4*>(o) = v;
        } else {
            for (int e = 0; e < 4 && x + e < tw; ++e) {
                o[3 * e] = (uint8_t)(px[e] & 255u);
                o[3 * e + 1] = (uint8_t)((px[e] >> 8) & 255u);
                o[3 * e + 2] = (uint8_t)(px[e] >> 16);
            }
        }
    }

    // label: Pillow's NEAREST resize as a gather through the host's index tables (-1: outside the virtual image -> 0)
    if (!out_lbl) return;
    const int32_t* lrow = tables + s.lrow;
    const int32_t* lcol = tables + s.lcol;
    const uint8_t* src_lbl = lbl + (int64_t)b * H * W;
    uint8_t* olbl = out_lbl + (int64_t)b * th * tw;
    int cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = x + e < tw ? lcol[x + e] : -1;
        cx[e] = c < W ? c : -1;
    }
    for (int y = y0 + (threadIdx.x >> 4); y < y1; y += TPB / 16) {
        int ry = lrow[y];
        if (ry >= H) ry = -1;
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ry >= 0 && cx[e] >= 0) v |= (uint32_t)src_lbl[(int64_t)ry * W + cx[e]] << (8 * e);
        uint8_t* o = olbl + (int64_t)y * tw + x;
        if (vec) {
            *reinterpret_cast<uint32_t*>(o) = v;
        } else {
            for (int e = 0; e < 4 && x + e < tw; ++e) o[e] = (uint8_t)(v >> (8 * e));
        }
    }
}

}  // namespace

extern "C" int dml_aug_scale_window(const uint8_t* img, const uint8_t* lbl, const DmlScaleWindow* samples, const int32_t* tables,
                                    int64_t table_len, uint8_t* out_img, uint8_t* out_lbl, int B, int H, int W, int th, int tw,
                                    int band_rows, int lds_rows, void* stream) {
    if (!img || !samples || !tables || !out_img || table_len <= 0) return DML_EINVAL;
    if ((lbl == nullptr) != (out_lbl == nullptr)) return DML_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || th <= 0 || tw <= 0 || band_rows <= 0 || lds_rows <= 0) return DML_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out_img) & 3) || (reinterpret_cast<uintptr_t>(out_lbl) & 3)) return DML_EALIGN;
    if (lds_rows > MAX_LDS_ROWS) return DML_EUNSUPPORTED;
    const int tiles_x = (tw + TW - 1) / TW, tiles_y = (th + band_rows - 1) / band_rows;
    const int64_t blocks = (int64_t)B * tiles_x * tiles_y;
    if (blocks > (1ll << 30) || (int64_t)B * H * W * 3 > (1ll << 40)) return DML_EUNSUPPORTED;
    hipLaunchKernelGGL(aug_scale_window_kernel, dim3((unsigned)blocks), dim3(TPB), (size_t)lds_rows * TW * sizeof(uint32_t),
                       static_cast<hipStream_t>(stream), img, lbl, samples, tables, table_len, out_img, out_lbl, H, W, th, tw,
                       band_rows, lds_rows, tiles_x, tiles_y);
    DML_LAUNCH_CHECK();
    return 0;
}
