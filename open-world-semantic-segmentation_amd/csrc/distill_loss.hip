// Feature-distillation term of the reference's utils/loss.py:104-117 on teacher features t[B,H,W,Ct] and student features
// s[B,H,W,Cs] (fp32, channels last): one fused forward pass (with the teacher's pseudo-labels written on the way), one fused
// backward pass that writes d dis / d s.  Definition, limits and normalisation: include/dmlnet_hip.h, DESIGN.md 7j.
//
// Lane-to-data mapping (both passes).  A pixel of 17 floats is 68 bytes, so a lane per pixel would load nothing wider than a
// dword.  Instead an image's student tensor is taken flat, in groups of four consecutive floats: group g of image b is the
// elements 4 g .. 4 g + 3, one lane each, a workgroup 256 consecutive groups, the workgroups of an image striding over it
// (the forward with teacher logits walks the same groups tile by tile of 256 pixels: distill_fwd_fill_kernel).
// Pixel and channel of the first element come from one multiplication (FastDiv); the other three step (channel + 1, wrap).
// The teacher floats the four elements need are consecutive as well (the pad channels are skipped, not stored), so they are one
// load of four floats at a 4-byte aligned address.  A label is loaded when the pixel changes, at most once per element.
// The aligned form loads and stores the group as 16 bytes, the other one float at a time; the group, the order of its four
// elements and every operation on them are the same, so both forms give the same bits.
#include "common.h"

#include <math.h>

namespace {

typedef float distill_f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at any 4-byte boundary

// the four teacher floats from tb on, zero past the image's end (nT floats)
__device__ __forceinline__ void distill_load_teacher(const float* timg, uint32_t tb, uint32_t nT, float (&tv)[4]) {
    if (tb + 4u <= nT) {
        const distill_f4u q = *reinterpret_cast<const distill_f4u*>(timg + tb);
        tv[0] = q.x; tv[1] = q.y; tv[2] = q.z; tv[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) tv[k] = tb + (uint32_t)k < nT ? timg[tb + k] : 0.f;
    }
}

// first maximal class of a pixel's teacher logits (NCHW; the tie rule of dml_argmax_msp); every load is issued before the first use
__device__ __forceinline__ int64_t distill_argmax(const float* lg, int Ct, int64_t HW) {
    float v[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
        if (k < Ct) v[k] = lg[(int64_t)k * HW];
    float best = v[0];
    int bi = 0;
#pragma unroll
    for (int k = 1; k < MAXC; ++k)
        if (k < Ct && v[k] > best) { best = v[k]; bi = k; }
    return bi;
}

// One group of four elements: d[k] = s - pad(t), m[k] = the element is there and its pixel is masked in, first[k] = it is channel 0
// of its pixel.  label(pix) is the (filled) label of a pixel of this image.
template <bool VEC, typename LabelOf>
__device__ __forceinline__ void distill_group(const float* timg, const float* simg, uint32_t g, uint32_t n_img, uint32_t nT, int Ct,
                                              int Cs, const FastDiv& divCs, int64_t novel_id, LabelOf label, float (&d)[4],
                                              bool (&m)[4], bool (&first)[4]) {
#pragma clang fp contract(off)
    const uint32_t e0 = 4u * g, left = n_img - e0;
    uint32_t pix = fdiv(e0, divCs);
    int c = (int)(e0 - pix * (uint32_t)Cs);
    float sv[4], tv[4];
    load4_tail<VEC>(simg + e0, left, sv);
    distill_load_teacher(timg, pix * (uint32_t)Ct + (uint32_t)(c < Ct ? c : Ct), nT, tv);
    int j = 0;
    bool in = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool there = VEC || (uint32_t)k < left;
        first[k] = there && c == 0;
        if (there && (k == 0 || c == 0)) in = label(pix) != novel_id;
        float t = 0.f;
        if (c < Ct) {
            t = j == 0 ? tv[0] : j == 1 ? tv[1] : j == 2 ? tv[2] : tv[3];
            ++j;
        }
        d[k] = sv[k] - t;
        m[k] = there && in;
        if (++c == Cs) { c = 0; ++pix; }
    }
}

__device__ __forceinline__ void distill_accumulate(const float (&d)[4], const bool (&m)[4], const bool (&first)[4], float& acc,
                                                   uint32_t& cnt) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (m[k]) acc = acc + d[k] * d[k];
        if (m[k] && first[k]) ++cnt;
    }
}

// a workgroup's partial = (sum d^2, #pixels as the bits of a uint32: exact whatever the workgroup's share of the image is), folded as
// one value of common.h's block_fold: the float by wave_sum, the count by integer additions
struct DistillPartial {
    float acc;
    uint32_t cnt;
};
__device__ __forceinline__ DistillPartial operator+(const DistillPartial& a, const DistillPartial& b) {
    return {a.acc + b.acc, a.cnt + b.cnt};
}
__device__ __forceinline__ DistillPartial wave_sum(DistillPartial v) {
    v.acc = ::wave_sum(v.acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v.cnt += (uint32_t)__shfl_xor((int)v.cnt, o, 64);
    return v;
}
__device__ __forceinline__ void distill_block_partial(float acc, uint32_t cnt, float* out) {
    const DistillPartial v[1] = {{acc, cnt}};
    block_fold(v, [&](int, const DistillPartial& s) {
        out[0] = s.acc;
        out[1] = __uint_as_float(s.cnt);
    });
}

// Without teacher logits.  grid (bpi, B): workgroup (j, b) takes the groups j * 256 + lane, stepping bpi * 256, of image b; a lane
// loads the label of each pixel its group touches.
template <bool VEC>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const float* __restrict__ t, const float* __restrict__ s,
                                                          const int64_t* __restrict__ labels, float* __restrict__ partials, int Ct,
                                                          int Cs, int64_t HW, FastDiv divCs, int64_t novel_id) {
    const int64_t b = blockIdx.y;
    const uint32_t n_img = (uint32_t)(HW * Cs), nT = (uint32_t)(HW * Ct), groups = (n_img + 3u) / 4u;
    const float* timg = t + b * HW * Ct;
    const float* simg = s + b * HW * Cs;
    const int64_t* lin = labels + b * HW;
    float acc = 0.f;
    uint32_t cnt = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256u) {
        float d[4];
        bool m[4], first[4];
        distill_group<VEC>(timg, simg, (uint32_t)g, n_img, nT, Ct, Cs, divCs, novel_id, [&](uint32_t pix) { return lin[pix]; }, d, m,
                           first);
        distill_accumulate(d, m, first, acc, cnt);
    }
    distill_block_partial(acc, cnt, partials + ((int64_t)b * gridDim.x + blockIdx.x) * 2);
}

// With teacher logits.  The logits are pixel-major planes, the features channel-major pixels: a workgroup takes tiles of 256
// consecutive pixels, grid (bpi, B), tile j, j + bpi, ... of image b.  First a lane fills one pixel's label -- label and, where it
// is ignored, the Ct logits, both coalesced over the tile -- writes labels_out and leaves it in LDS; then the tile's 64 Cs groups
// (256 Cs floats: a tile starts on a group) go over the lanes as above, their labels read from LDS.  A pixel's label is read and
// written by one lane only, so labels_out may be labels_in.  (Filling from the lane that holds a pixel's channel 0 in the
// mapping above was measured first: 16 dependent, scattered dword loads per ignored pixel, 2.09 ms against 0.28 ms without the
// fill at 16 x 768 x 768 x (16, 17).)
template <bool VEC>
__global__ __launch_bounds__(256) void distill_fwd_fill_kernel(const float* __restrict__ t_logits, const float* __restrict__ t,
                                                               const float* __restrict__ s, const int64_t* labels_in,
                                                               int64_t* labels_out, float* __restrict__ partials, int Ct, int Cs,
                                                               int64_t HW, FastDiv divCs, int64_t ignore_index, int64_t novel_id) {
    __shared__ int64_t lab_sh[256];
    const int64_t b = blockIdx.y;
    const uint32_t n_img = (uint32_t)(HW * Cs), nT = (uint32_t)(HW * Ct), px = (uint32_t)HW, tiles = (px + 255u) / 256u;
    const float* timg = t + b * HW * Ct;
    const float* simg = s + b * HW * Cs;
    const int64_t* lin = labels_in + b * HW;
    int64_t* lout = labels_out + b * HW;
    const float* lgimg = t_logits + b * Ct * HW;
    float acc = 0.f;
    uint32_t cnt = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t p0 = tile * 256u, p = p0 + threadIdx.x, npx = px - p0 < 256u ? px - p0 : 256u;
        if (p < px) {
            int64_t lab = lin[p];
            const bool ign = lab == ignore_index;
            if (ign) lab = distill_argmax(lgimg + p, Ct, HW);
            if (ign || lout != lin) lout[p] = lab;
            lab_sh[threadIdx.x] = lab;
        }
        __syncthreads();
        const uint32_t g0 = p0 / 4u * (uint32_t)Cs, ng = (npx * (uint32_t)Cs + 3u) / 4u;      // p0 % 256 == 0
        for (uint32_t g = threadIdx.x; g < ng; g += 256u) {
            float d[4];
            bool m[4], first[4];
            distill_group<VEC>(timg, simg, g0 + g, n_img, nT, Ct, Cs, divCs, novel_id, [&](uint32_t pix) { return lab_sh[pix - p0]; },
                               d, m, first);
            distill_accumulate(d, m, first, acc, cnt);
        }
        __syncthreads();                                         // the next tile's labels replace these
    }
    distill_block_partial(acc, cnt, partials + ((int64_t)b * gridDim.x + blockIdx.x) * 2);
}


// the double fold of the workgroups' partials in a fixed order: a wave per image, then one wave over the images' S / cnt
__global__ __launch_bounds__(256) void distill_sum_kernel(const float* __restrict__ partials, int B, int bpi, double* sums) {
    __shared__ double ratio[MAX_BLOCKS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = wv; i < B; i += 4) {
        double a = 0, c = 0;
        for (int j = lane; j < bpi; j += 64) {
            a += (double)partials[((int64_t)i * bpi + j) * 2];
            c += (double)__float_as_uint(partials[((int64_t)i * bpi + j) * 2 + 1]);
        }
        a = wave_sum_d(a); c = wave_sum_d(c);
        if (lane == 0) {
            sums[2 * i] = a;
            sums[2 * i + 1] = c;
            ratio[i] = c > 0 ? a / c : 0.0;
        }
    }
    __syncthreads();
    if (wv == 0) {
        double r = 0;
        for (int i = lane; i < B; i += 64) r += ratio[i];
        r = wave_sum_d(r);
        if (lane == 0) { sums[2 * B] = r; sums[2 * B + 1] = (double)B; }
    }
}

__global__ void distill_finalize_kernel(const double* sums, int B, float n_images, float* dis) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double n = n_images > 0.f ? (double)n_images : sums[2 * B + 1];
        *dis = (float)(sums[2 * B] / n);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const float* __restrict__ t, const float* __restrict__ s,
                                                          const int64_t* __restrict__ labels, const double* __restrict__ sums,
                                                          const float* __restrict__ gout, float* __restrict__ gs, int B, int Ct,
                                                          int Cs, int64_t HW, FastDiv divCs, int64_t novel_id, float n_images) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const uint32_t n_img = (uint32_t)(HW * Cs), nT = (uint32_t)(HW * Ct), groups = (n_img + 3u) / 4u;
    const double n = n_images > 0.f ? (double)n_images : sums[2 * B + 1], cnt = sums[2 * b + 1];
    const double go = gout ? (double)*gout : 1.0;
    const float w = cnt > 0 ? (float)(go * 2.0 / (n * cnt)) : 0.f;
    const float* timg = t + b * HW * Ct;
    const float* simg = s + b * HW * Cs;
    const int64_t* lin = labels + b * HW;
    float* gimg = gs + b * HW * Cs;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256u) {
        float d[4], r[4];
        bool m[4], first[4];
        distill_group<VEC>(timg, simg, (uint32_t)g, n_img, nT, Ct, Cs, divCs, novel_id, [&](uint32_t pix) { return lin[pix]; }, d, m,
                           first);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = m[k] ? w * d[k] : 0.f;
        store4_tail<VEC>(gimg + 4u * (uint32_t)g, n_img - 4u * (uint32_t)g, r);
    }
}

int distill_shape_check(int B, int Ct, int Cs, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || Ct < 1 || Ct > Cs || Cs > MAXC) return DML_EINVAL;
    if (B > MAX_BLOCKS || (int64_t)H * W * Cs >= ((int64_t)1 << 31)) return DML_EUNSUPPORTED;
    return 0;
}
int distill_bpi(int B, int64_t HW, int Cs) {
    const int64_t groups = (HW * Cs + 3) / 4;
    return grid_for(groups, 256, MAX_BLOCKS / B);
}
bool distill_vec(int64_t HW, int Cs, const void* a, const void* b) {
    return (HW * Cs) % 4 == 0 && aligned16(a, b);
}

}  // namespace

extern "C" int dml_distill_fwd(const float* t_logits, const float* t, const float* s, const int64_t* labels_in,
                               int64_t* labels_out, double* sums, float* block_partials, int B, int Ct, int Cs, int H, int W,
                               int64_t ignore_index, int64_t novel_id, void* stream) {
    if (!t || !s || !labels_in || !sums || !block_partials || (t_logits && !labels_out)) return DML_EINVAL;
    if (const int rc = distill_shape_check(B, Ct, Cs, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    const bool vec = distill_vec(HW, Cs, s, nullptr), fill = t_logits != nullptr;
    const int bpi = fill ? grid_for((HW + 255) / 256, 1, MAX_BLOCKS / B) : distill_bpi(B, HW, Cs);      // tiles : groups
    const FastDiv divCs = make_fastdiv((uint32_t)Cs);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define DISTILL_FILL(VEC)                                                                                                      \
    hipLaunchKernelGGL((distill_fwd_fill_kernel<VEC>), dim3(bpi, B), dim3(256), 0, st, t_logits, t, s, labels_in, labels_out,  \
                       block_partials, Ct, Cs, HW, divCs, ignore_index, novel_id)
#define DISTILL_FWD(VEC)                                                                                                       \
    hipLaunchKernelGGL((distill_fwd_kernel<VEC>), dim3(bpi, B), dim3(256), 0, st, t, s, labels_in, block_partials, Ct, Cs, HW, \
                       divCs, novel_id)
    if (vec && fill) DISTILL_FILL(true);
    else if (fill) DISTILL_FILL(false);
    else if (vec) DISTILL_FWD(true);
    else DISTILL_FWD(false);
#undef DISTILL_FILL
#undef DISTILL_FWD
    hipLaunchKernelGGL(distill_sum_kernel, dim3(1), dim3(256), 0, st, block_partials, B, bpi, sums);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_distill_finalize(const double* sums, int B, float n_images, float* dis, void* stream) {
    if (!sums || !dis || B <= 0) return DML_EINVAL;
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sums, B, n_images, dis);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_distill_bwd(const float* t, const float* s, const int64_t* labels, const double* sums, const float* gout,
                               float* gs, int B, int Ct, int Cs, int H, int W, int64_t novel_id, float n_images, void* stream) {
    if (!t || !s || !labels || !sums || !gs) return DML_EINVAL;
    if (const int rc = distill_shape_check(B, Ct, Cs, H, W)) return rc;
    const int64_t HW = (int64_t)H * W;
    const int bpi = distill_bpi(B, HW, Cs);
    const FastDiv divCs = make_fastdiv((uint32_t)Cs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (distill_vec(HW, Cs, s, gs))
        hipLaunchKernelGGL((distill_bwd_kernel<true>), dim3(bpi, B), dim3(256), 0, st, t, s, labels, sums, gout, gs, B, Ct, Cs, HW,
                           divCs, novel_id, n_images);
    else
        hipLaunchKernelGGL((distill_bwd_kernel<false>), dim3(bpi, B), dim3(256), 0, st, t, s, labels, sums, gout, gs, B, Ct, Cs, HW,
                           divCs, novel_id, n_images);
    DML_LAUNCH_CHECK();
    return 0;
}
