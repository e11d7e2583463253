// Shared device/host helpers for the gfx950 kernels (wave = 64 lanes, MFMA, LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "../../include/dmlnet_hip.h"

#define DML_LAUNCH_CHECK()                        \
    do {                                          \
        hipError_t e__ = hipGetLastError();       \
        if (e__ != hipSuccess) return (int)e__;   \
    } while (0)

typedef unsigned short bf16_t;   // raw bfloat16 bits

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // MFMA operand: 8 bf16 in 4 VGPRs
typedef __attribute__((ext_vector_type(4))) short bf16x4;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even, NaN preserved
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
// two floats -> packed bf16 pair (lo in bits 0-15), round-to-nearest-even: one v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
    typedef float f32x2_hw __attribute__((ext_vector_type(2)));
    const f32x2_hw v = {lo, hi};
    const bf16x2_hw b = __builtin_convertvector(v, bf16x2_hw);
    return __builtin_bit_cast(uint32_t, b);
}

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int VEC = 4;   // elements per 16-byte vector
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct Elem<bf16_t> {
    static constexpr int VEC = 8;
    __device__ static __forceinline__ float ld(const bf16_t* p) { return bf16_to_f32(*p); }
    __device__ static __forceinline__ void st(bf16_t* p, float v) { *p = f32_to_bf16(v); }
};

// 16-byte vector of T unpacked to floats and back.
template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    __device__ static __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec16<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    __device__ static __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

// unsigned division by a runtime constant: q = n / d for n < 2^31
struct FastDiv {
    uint32_t mul, shr, d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    if (d == 1) { f.mul = 0; f.shr = 0; return f; }
    uint32_t l = 0;
    while ((1u << l) < d) ++l;                       // ceil(log2 d)
    const uint64_t p = 31 + l;
    f.mul = (uint32_t)(((1ull << p) + d - 1) / d);
    f.shr = (uint32_t)(p - 32);
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    return f.d == 1 ? n : (__umulhi(n, f.mul) >> f.shr);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_d(v); }

// Sum of Q per-lane values over the four waves of a 256-thread workgroup, always in the order ((w0 + w1) + w2) + w3: thread q < Q
// gets value q as deliver(q, sum).  T needs operator+ and a wave_sum.  The helper owns a __shared__ array: two uses in one kernel
// need a __syncthreads() between them.
template <int Q, typename T, typename F> __device__ __forceinline__ void block_fold(const T (&v)[Q], F&& deliver) {
    __shared__ T sh[4][Q];
    T w[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) w[q] = wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) sh[threadIdx.x >> 6][q] = w[q];
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        const int q = threadIdx.x;
        deliver(q, ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q]);
    }
}

// ---- the pixel kernels' shared pieces
constexpr int MAXC = 32, MAXK = 33;   // channels or classes a lane keeps in registers / prototype rows of the distance head
constexpr int MAX_BLOCKS = 2048;      // workgroups of a launch that leaves one partial each: what the callers' buffers hold
// non-temporal stores of logits / features: standalone head 0.378 -> 0.358 ms, staged x4 kernel 0.237 -> 0.219 ms
// (tools/bench_dist_variants.py, 768 x 768 x 16)
constexpr bool DIST_NT_DEFAULT = true;

// 16-byte load / store; NT = true marks it non-temporal: a stream that is read once or that nobody re-reads from cache (logits and
// features, 1.2 GB per step, far beyond L2)
template <bool NT = false> __device__ __forceinline__ float4 load4(const float* p) {
    if constexpr (NT) {
        typedef float f32x4_nt __attribute__((ext_vector_type(4)));
        const f32x4_nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(p));
        return make_float4(t.x, t.y, t.z, t.w);
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}
template <bool NT = false> __device__ __forceinline__ void store4(float* p, const float4 v) {
    if constexpr (NT) {
        typedef float f32x4_nt __attribute__((ext_vector_type(4)));
        f32x4_nt t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<f32x4_nt*>(p));
    } else {
        *reinterpret_cast<float4*>(p) = v;
    }
}
// PX = 1 or 4 consecutive floats of one lane: 16 bytes when PX == 4
template <int PX, bool NT = false> __device__ __forceinline__ void load_px(const float* p, float (&v)[PX]) {
    if constexpr (PX == 4) {
        const float4 t = load4<NT>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int PX, bool NT = false> __device__ __forceinline__ void store_px(float* p, const float (&v)[PX]) {
    if constexpr (PX == 4) store4<NT>(p, make_float4(v[0], v[1], v[2], v[3]));
    else *p = v[0];
}
// four floats of which only the first `left` are there: VEC (left >= 4 and p 16-byte aligned) takes them as one vector
template <bool VEC> __device__ __forceinline__ void load4_tail(const float* p, uint32_t left, float (&v)[4]) {
    if constexpr (VEC) {
        Vec16<float>::load(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (uint32_t)k < left ? p[k] : 0.f;
    }
}
template <bool VEC> __device__ __forceinline__ void store4_tail(float* p, uint32_t left, const float (&v)[4]) {
    if constexpr (VEC) {
        Vec16<float>::store(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint32_t)k < left) p[k] = v[k];
    }
}

// Bilinear resize, align_corners = False (PyTorch's area_pixel_compute_source_index): the two source taps of output index I on an
// axis of n samples at scale s = n / N.  Every kernel that resizes goes through this, so they all see the same coordinates and
// weights:  src = max(s * (I + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < n - 1), l1 = src - i0
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

__device__ __forceinline__ void load_protos(float* sp, const float* __restrict__ protos, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = protos[i];
    __syncthreads();
}

// every pointer is a multiple of `bytes` (a power of two); a null pointer counts as aligned
template <typename... P> static inline bool aligned_to(uintptr_t bytes, const P*... p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & (bytes - 1)) == 0;
}
template <typename... P> static inline bool aligned16(const P*... p) { return aligned_to(16, p...); }

// Workgroups for a grid-stride streaming kernel.  Caps of 2048 and above are "enough to fill the chip" choices, not
// buffer sizes (short-lived workgroups stream faster than persistent ones, see bn.hip).
static inline int grid_for(int64_t work_items, int block, int max_blocks = 256 * 8) {
    int64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}
