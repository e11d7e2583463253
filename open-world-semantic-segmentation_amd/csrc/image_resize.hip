// Evaluation input of the anomaly sub-project: Pillow's 8-bit BILINEAR resize of one uint8 HWC RGB frame to every scale of
// the multi-scale test, + ToTensor + Normalize (anomaly/dataset.py:249-300 of the reference), bit for bit -- see the header.
// One launch for all scales: a workgroup owns a band of output rows x 64 output columns of one scale, runs the horizontal
// pass over exactly the source rows that band's vertical taps read into LDS (uint8, packed RGB per dword) and then the
// vertical pass from LDS, writing fp32 NCHW with 16-byte stores.  HBM-bound: ~2.8 MB in, ~22 MB out per StreetHazards frame.
#include "common.h"

namespace {

constexpr int TPB = 256;          // threads per workgroup
constexpr int TW = 64;            // output columns per workgroup
constexpr int MAX_LDS_ROWS = 256; // 64 KiB of intermediate rows
constexpr int PREC = 22;          // fraction bits of the fixed-point weights (Resample.c PRECISION_BITS)

struct ResizeArgs {
    DmlResizeScale s[DML_RESIZE_MAX_SCALES];
    int32_t block0[DML_RESIZE_MAX_SCALES + 1];   // first workgroup of each scale; block0[S] = grid size
    int32_t tiles_x[DML_RESIZE_MAX_SCALES];
    int32_t S;
    float mean[3], stdv[3];
};

// Resample.c clip8: (acc >> 22) clamped to [0, 255] (arithmetic shift)
__device__ __forceinline__ uint32_t clip8(int32_t acc) {
    const int32_t v = acc >> PREC;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ToTensor (float32 v / 255) then Normalize (sub then true division)
__device__ __forceinline__ float norm(uint32_t v, float m, float s) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), m), s);
}

__global__ __launch_bounds__(TPB) void pil_resize_normalize_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                    const ResizeArgs a) {
    extern __shared__ uint32_t inter[];                      // [lds_rows][TW] packed R | G << 8 | B << 16
    int si = 0;
    while (si + 1 < a.S && (int)blockIdx.x >= a.block0[si + 1]) ++si;
    const DmlResizeScale& s = a.s[si];
    const int t = (int)blockIdx.x - a.block0[si];
    const int ty = t / a.tiles_x[si], tx = t - ty * a.tiles_x[si];
    const int y0 = ty * s.band_rows, y1 = min(y0 + s.band_rows, s.Hs);
    const int x0 = tx * TW;
    const int r0 = s.vbounds[2 * y0];
    const int r1 = min(s.vbounds[2 * (y1 - 1)] + s.vbounds[2 * (y1 - 1) + 1], h);
    const int nrows = min(r1 - r0, s.lds_rows);             // the host sized lds_rows to cover every band

    // horizontal pass: intermediate rows r0..r1-1, columns x0..x0+63 of this scale
    for (int idx = threadIdx.x; idx < nrows * TW; idx += TPB) {
        const int r = idx / TW, xc = idx - r * TW, x = x0 + xc;
        if (x >= s.Ws) continue;
        const int xmin = s.hbounds[2 * x], n = s.hbounds[2 * x + 1];
        const int32_t* k = s.hcoef + (int64_t)x * s.kh;
        const uint8_t* src = img + ((int64_t)(r0 + r) * w + xmin) * 3;
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

    // vertical pass + normalisation: 16 groups of 4 columns x 16 rows at a time
    const int xg = (threadIdx.x & 15) * 4, x = x0 + xg;
    if (x >= s.Ws) return;
    const int64_t plane = (int64_t)s.Hs * s.Ws;
    const bool vec = (s.Ws & 3) == 0 && (reinterpret_cast<uintptr_t>(s.out) & 15) == 0;   // then x + 3 < Ws too
    for (int y = y0 + (threadIdx.x >> 4); y < y1; y += TPB / 16) {
        const int ymin = s.vbounds[2 * y] - r0, n = min(s.vbounds[2 * y + 1], nrows - ymin);
        const int32_t* k = s.vcoef + (int64_t)y * s.kv;
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
        float* o = s.out + (int64_t)y * s.Ws + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = norm(clip8(acc[e][c]), a.mean[c], a.stdv[c]);
            if (vec) {
                *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int e = 0; e < 4 && x + e < s.Ws; ++e) o[c * plane + e] = v[e];
            }
        }
    }
}

__global__ __launch_bounds__(256) void segm_to_label_kernel(const uint8_t* __restrict__ segm, int64_t n, int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (int64_t)segm[i] - 1;
}

}  // namespace

extern "C" int dml_pil_resize_normalize(const uint8_t* img, int h, int w, const DmlResizeScale* scales, int S, float mean0,
                                        float mean1, float mean2, float std0, float std1, float std2, void* stream) {
    if (!img || !scales || h <= 0 || w <= 0 || S <= 0 || S > DML_RESIZE_MAX_SCALES) return DML_EINVAL;
    if (std0 == 0.f || std1 == 0.f || std2 == 0.f) return DML_EINVAL;
    ResizeArgs a;
    a.S = S;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
    a.stdv[0] = std0; a.stdv[1] = std1; a.stdv[2] = std2;
    int64_t blocks = 0;
    int lds_rows = 1;
    for (int i = 0; i < S; ++i) {
        const DmlResizeScale& s = scales[i];
        if (!s.out || !s.hbounds || !s.hcoef || !s.vbounds || !s.vcoef) return DML_EINVAL;
        if (s.Hs <= 0 || s.Ws <= 0 || s.kh <= 0 || s.kv <= 0 || s.band_rows <= 0 || s.lds_rows <= 0) return DML_EINVAL;
        if (s.lds_rows > MAX_LDS_ROWS) return DML_EUNSUPPORTED;
        a.s[i] = s;
        a.tiles_x[i] = (s.Ws + TW - 1) / TW;
        a.block0[i] = (int32_t)blocks;
        blocks += (int64_t)a.tiles_x[i] * ((s.Hs + s.band_rows - 1) / s.band_rows);
        lds_rows = s.lds_rows > lds_rows ? s.lds_rows : lds_rows;
    }
    if (blocks > (1ll << 30)) return DML_EUNSUPPORTED;
    a.block0[S] = (int32_t)blocks;
    hipLaunchKernelGGL(pil_resize_normalize_kernel, dim3((unsigned)blocks), dim3(TPB), (size_t)lds_rows * TW * sizeof(uint32_t),
                       static_cast<hipStream_t>(stream), img, h, w, a);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_segm_to_label(const uint8_t* segm, int64_t n, int64_t* out, void* stream) {
    if (n == 0) return 0;
    if (!segm || !out || n < 0) return DML_EINVAL;
    const int64_t want = (n + 256 * 8 - 1) / (256 * 8);
    hipLaunchKernelGGL(segm_to_label_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), segm, n, out);
    DML_LAUNCH_CHECK();
    return 0;
}
