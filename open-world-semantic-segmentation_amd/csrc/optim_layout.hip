// Optimizer step and layout/precision conversion kernels for gfx950 (all HBM-bound).
//
// dml_sgd_step replaces torch.optim.SGD.step as configured at main_embedding.py:385-388
// (momentum 0.9, weight decay added to the gradient before the momentum update, two LR groups).
// The remaining kernels exist because the MI355X design keeps fp32 master weights in K-R-S-C order
// and feeds the MFMA kernels from bf16/fp32 compute copies (and transposed copies for dgrad).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ v, int64_t n, float lr, float mu, float wd,
                                                  float gscale) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        vv.x = mu * vv.x + (gscale * gg.x + wd * pp.x);
        vv.y = mu * vv.y + (gscale * gg.y + wd * pp.y);
        vv.z = mu * vv.z + (gscale * gg.z + wd * pp.z);
        vv.w = mu * vv.w + (gscale * gg.w + wd * pp.w);
        pp.x -= lr * vv.x; pp.y -= lr * vv.y; pp.z -= lr * vv.z; pp.w -= lr * vv.w;
        reinterpret_cast<float4*>(v)[i] = vv;
        reinterpret_cast<float4*>(p)[i] = pp;
    }
    // tail
    const int64_t base = n4 << 2;
    const int64_t t = base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const float d = gscale * g[t] + wd * p[t];
        const float nv = mu * v[t] + d;
        v[t] = nv;
        p[t] -= lr * nv;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ p, int64_t n, float value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = value;
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void convert_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        Elem<TD>::st(dst + i, Elem<TS>::ld(src + i));
}

// master [N][RS][Cm] fp32 -> w [N][RS][Cp] and wt [Cp][RS][N]
template <typename T>
__global__ __launch_bounds__(256) void prep_weight_kernel(const float* __restrict__ src, T* __restrict__ w,
                                                          T* __restrict__ wt, int N, int RS, int Cm, int Cp) {
    const int64_t total = (int64_t)N * RS * Cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cp);
        const int64_t t = i / Cp;
        const int rs = (int)(t % RS);
        const int n = (int)(t / RS);
        const float v = c < Cm ? src[((int64_t)n * RS + rs) * Cm + c] : 0.f;
        Elem<T>::st(w + i, v);
        if (wt != nullptr) Elem<T>::st(wt + ((int64_t)c * RS + rs) * N + n, v);
    }
}

// all convolutions of a model in ONE launch: blockIdx.y selects the descriptor.  32 x 32 (n x c) tiles go through
// LDS so that BOTH copies are written with consecutive addresses (the naive scatter into wt[c][rs][n] cost 7x
// its bytes in partial-sector writes).
template <typename T>
__global__ __launch_bounds__(256) void prep_weights_kernel(const DmlPrepDesc* __restrict__ descs) {
    __shared__ float tile[32][33];
    const DmlPrepDesc d = descs[blockIdx.y];
    const float* __restrict__ src = d.src;
    T* __restrict__ w = static_cast<T*>(d.w);
    T* __restrict__ wt = static_cast<T*>(d.wt);
    const int N = d.N, RS = d.RS, Cm = d.Cm, Cp = d.Cp;
    // tile-major copies (DmlPrepDesc::w_tiled / wt_tiled): matrix [rows][K] as [rows / 64][K / 32][64][32]; a 32 x 32 tile of
    // this loop (32-aligned in both directions) is 1024 consecutive elements there as well
    const bool wtl = d.w_tiled != 0, wttl = d.wt_tiled != 0;
    const int64_t KTw = (int64_t)RS * Cp / 32, KTt = (int64_t)RS * N / 32;
    auto idx_w = [&](int n, int rs, int c) -> int64_t {
        if (!wtl) return ((int64_t)n * RS + rs) * Cp + c;
        const int64_t k = (int64_t)rs * Cp + c;
        return ((int64_t)(n >> 6) * KTw + (k >> 5)) * 2048 + (n & 63) * 32 + (k & 31);
    };
    auto idx_wt = [&](int c, int rs, int n) -> int64_t {
        if (!wttl) return ((int64_t)c * RS + rs) * N + n;
        const int64_t k = (int64_t)rs * N + n;
        return ((int64_t)(c >> 6) * KTt + (k >> 5)) * 2048 + (c & 63) * 32 + (k & 31);
    };
    const int tn = (N + 31) / 32, tc = (Cp + 31) / 32;
    const int ntiles = tn * tc * RS;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int rs = t % RS;
        const int tt = t / RS;
        const int c0 = (tt % tc) * 32, n0 = (tt / tc) * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + ty + j * 8, c = c0 + tx;
            float v = 0.f;
            if (n < N && c < Cp) {
                if (c < Cm) v = src[((int64_t)n * RS + rs) * Cm + c];
                Elem<T>::st(w + idx_w(n, rs, c), v);
            }
            tile[ty + j * 8][tx] = v;
        }
        __syncthreads();
        if (wt != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + ty + j * 8, n = n0 + tx;
                if (c < Cp && n < N) Elem<T>::st(wt + idx_wt(c, rs, n), tile[tx][ty + j * 8]);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void unpad_wgrad_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          int N, int RS, int Cm, int Cp) {
    const int64_t total = (int64_t)N * RS * Cm;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cm);
        const int64_t t = i / Cm;
        dst[i] += src[t * Cp + c];
    }
}

// db[n] += sum_m dy[m][n]; one block per 64 rows-lanes x N columns
template <typename T>
__global__ __launch_bounds__(256) void bias_grad_kernel(const T* __restrict__ dy, float* __restrict__ db, int64_t M,
                                                        int N, int ldy, float* __restrict__ part) {
    // thread -> column n = tid % N (N <= 256), row lane = tid / N
    const int n = threadIdx.x % N, rl = threadIdx.x / N, rt = blockDim.x / N;
    float acc = 0.f;
    if (rl < rt)
        for (int64_t m = (int64_t)blockIdx.x * rt + rl; m < M; m += (int64_t)gridDim.x * rt)
            acc += Elem<T>::ld(dy + m * ldy + n);
    if (rl < rt) {
        if (part != nullptr) part[((int64_t)blockIdx.x * rt + rl) * N + n] = acc;
        else atomicAdd(db + n, acc);
    }
}

// db[n] += sum_r part[r][n] in row order (second stage of the deterministic bias gradient)
__global__ __launch_bounds__(256) void bias_grad_fold_kernel(const float* __restrict__ part, float* __restrict__ db, int rows, int N) {
    __shared__ float sh[256];
    const int n = threadIdx.x % N, rl = threadIdx.x / N, rt = 256 / N;
    float acc = 0.f;
    if (rl < rt)
        for (int r = rl; r < rows; r += rt) acc += part[(int64_t)r * N + n];
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < N) {
        float t = 0.f;
        for (int r = 0; r < rt; ++r) t += sh[r * N + threadIdx.x];
        db[threadIdx.x] += t;
    }
}

// vector form: a thread owns one 16-byte channel vector and walks rows; row lanes are folded through LDS so that a
// block issues one atomic per channel
template <typename T>
__global__ __launch_bounds__(256) void bias_grad_vec_kernel(const T* __restrict__ dy, float* __restrict__ db, int64_t M,
                                                            int N, int ldy, int rows_per_block, float* __restrict__ part) {
    constexpr int V = Vec16<T>::N;
    __shared__ float sh[256 * V];
    const int NV = N / V, rt = 256 / NV;
    const int col = threadIdx.x % NV, rl = threadIdx.x / NV;
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.f;
    if (rl < rt) {
        const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
        for (int64_t m = r0 + rl; m < r1; m += rt) {
            float v[V];
            Vec16<T>::load(dy + m * ldy + col * V, v);
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] += v[q];
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) sh[threadIdx.x * V + q] = acc[q];
    __syncthreads();
    if (threadIdx.x < N) {
        const int c = threadIdx.x / V, q = threadIdx.x % V;
        float t = 0.f;
        for (int r = 0; r < rt; ++r) t += sh[(r * NV + c) * V + q];
        if (part != nullptr) part[(int64_t)blockIdx.x * N + threadIdx.x] = t;
        else atomicAdd(db + threadIdx.x, t);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_input_kernel(const float* __restrict__ x, T* __restrict__ y, int B,
                                                         int C, int64_t HW, int Cp) {
    const int64_t total = (int64_t)B * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, pix = i - b * HW;
        for (int c = 0; c < Cp; ++c) {
            const float v = c < C ? x[(b * C + c) * HW + pix] : 0.f;
            Elem<T>::st(y + i * Cp + c, v);
        }
    }
}

}  // namespace

extern "C" int dml_abi_version(void) { return DML_ABI_VERSION; }
extern "C" const char* dml_target_arch(void) { return "gfx950"; }

extern "C" int dml_sgd_step(float* p, const float* g, float* v, int64_t n, float lr, float momentum,
                            float weight_decay, float gscale, void* stream) {
    if (!p || !g || !v || n <= 0) return DML_EINVAL;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) return DML_EALIGN;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n / 4 + 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       p, g, v, n, lr, momentum, weight_decay, gscale);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_fill_f32(float* p, int64_t n, float value, void* stream) {
    if (!p || n <= 0) return DML_EINVAL;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), p, n,
                       value);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_convert_dtype(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream) {
    if (!src || !dst || n <= 0) return DML_EINVAL;
    if ((src_dtype != DML_F32 && src_dtype != DML_BF16) || (dst_dtype != DML_F32 && dst_dtype != DML_BF16)) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(n, 256)), blk(256);
    if (src_dtype == DML_F32 && dst_dtype == DML_BF16)
        hipLaunchKernelGGL((convert_kernel<float, bf16_t>), grid, blk, 0, st, (const float*)src, (bf16_t*)dst, n);
    else if (src_dtype == DML_BF16 && dst_dtype == DML_F32)
        hipLaunchKernelGGL((convert_kernel<bf16_t, float>), grid, blk, 0, st, (const bf16_t*)src, (float*)dst, n);
    else if (src_dtype == DML_F32)
        hipLaunchKernelGGL((convert_kernel<float, float>), grid, blk, 0, st, (const float*)src, (float*)dst, n);
    else
        hipLaunchKernelGGL((convert_kernel<bf16_t, bf16_t>), grid, blk, 0, st, (const bf16_t*)src, (bf16_t*)dst, n);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_prep_weight(const float* w_master, void* w, void* wt, int N, int RS, int Cm, int Cp, int dtype,
                               void* stream) {
    if (!w_master || !w || N <= 0 || RS <= 0 || Cm <= 0 || Cp < Cm) return DML_EINVAL;
    const int grid = grid_for((int64_t)N * RS * Cp, 256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DML_BF16)
        hipLaunchKernelGGL(prep_weight_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, w_master, (bf16_t*)w,
                           (bf16_t*)wt, N, RS, Cm, Cp);
    else
        hipLaunchKernelGGL(prep_weight_kernel<float>, dim3(grid), dim3(256), 0, st, w_master, (float*)w, (float*)wt,
                           N, RS, Cm, Cp);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_prep_weights(const DmlPrepDesc* descs_device, int count, int dtype, void* stream) {
    if (!descs_device || count <= 0) return DML_EINVAL;
    dim3 grid(256, count);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DML_BF16) hipLaunchKernelGGL(prep_weights_kernel<bf16_t>, grid, dim3(256), 0, st, descs_device);
    else hipLaunchKernelGGL(prep_weights_kernel<float>, grid, dim3(256), 0, st, descs_device);
    DML_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// fp32 -> two fp16 planes of the power-of-two-scaled tensor (DmlConvDesc.x_planes / w_planes, dml_h2_split).
// Why fp16 and a scale: two bf16 terms carry 16 significand bits -- the parity fixtures' gradients then miss their 2e-3 bars by
// 10x (tests/tools/emu_split_terms.py) -- two fp16 terms carry 22, which sits at the reference's own fp32-vs-fp64 noise; fp16's
// narrow exponent range is met by scaling the whole tensor with a power of two that puts its largest magnitude just below 2^15
// (products up to 2^30 accumulate in fp32; small elements lose relative precision only below 2^-29 of the maximum).
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int H2_MAXBLK = 1024;
__global__ __launch_bounds__(256) void h2_amax_kernel(const float* __restrict__ x, int64_t rows, int C, int ld, float* __restrict__ work) {
    // per-workgroup maxima of |x| (as unsigned bit patterns: order-preserving for non-negative floats, NaN ends up largest)
    const int cv = C >> 2;                                 // float4 per row
    const int64_t total = rows * cv;
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cv;
        const int c = (int)(i - r * cv) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c);
        m = max(max(m, __float_as_uint(v.x) & 0x7fffffffu), max(__float_as_uint(v.y) & 0x7fffffffu, max(__float_as_uint(v.z) & 0x7fffffffu,
                                                                                               __float_as_uint(v.w) & 0x7fffffffu)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) work[blockIdx.x] = __uint_as_float(max(max(sh[0], sh[1]), max(sh[2], sh[3])));
}

// scale = 2^(14 - floor(log2 amax)) so that amax * scale is in [2^14, 2^15); amax = 0 -> 1
__device__ __forceinline__ float h2_scale_from(const float* work, int nblk) {
    uint32_t m = 0;
    for (int i = threadIdx.x; i < nblk; i += 256) m = max(m, __float_as_uint(work[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t shm[4];
    if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = max(max(shm[0], shm[1]), max(shm[2], shm[3]));
    if (m == 0) return 1.0f;
    const int e = (int)(m >> 23) - 127;                    // floor(log2 amax) (subnormal amax: -127, scale saturates at 2^127)
    int se = 14 - e;
    se = se > 127 ? 127 : (se < -126 ? -126 : se);
    float s = __uint_as_float((uint32_t)(se + 127) << 23);
    if ((m & 0x7fffffffu) >= 0x7f800000u) s = __uint_as_float(m);      // Inf / NaN in the tensor: propagate through the scale
    return s;
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void h2_split_kernel(const float* __restrict__ x, int64_t rows, int C, int ld, _Float16* __restrict__ planes,
                                                       int64_t plane_stride, int ldp, float* __restrict__ work, int nblk) {
    const float s = h2_scale_from(work, nblk);
    if (blockIdx.x == 0 && threadIdx.x == 0) work[H2_MAXBLK] = 1.0f / s;
    const int cv = C >> 3;                                 // 8 elements per thread
    const int64_t total = rows * cv;
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cv;
        const int c = (int)(i - r * cv) * 8;
        const float4 v0 = *reinterpret_cast<const float4*>(x + r * ld + c);
        const float4 v1 = *reinterpret_cast<const float4*>(x + r * ld + c + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xs = v[e] * s;
            const _Float16 h = (_Float16)xs;               // round to nearest even
            hi[e] = h;
            lo[e] = (_Float16)(xs - (float)h);             // the residual is exact in fp32
        }
        int64_t off;
        if (LAYOUT == 0) off = r * ldp + c;
        else off = (((r >> 6) * (C >> 5) + (c >> 5)) * 64 + (r & 63)) * 32 + (c & 31);      // [rows / 64][C / 32][64][32]
        *reinterpret_cast<h8*>(planes + off) = hi;
        *reinterpret_cast<h8*>(planes + plane_stride + off) = lo;
    }
}
}  // namespace

extern "C" int dml_h2_split(const float* x, int64_t rows, int32_t C, int32_t ld, void* planes, int64_t plane_stride, int32_t ldp,
                            int32_t layout, float* work, int32_t amax_known, void* stream) {
    if (!x || !planes || !work || rows <= 0 || C <= 0 || plane_stride <= 0) return DML_EINVAL;
    if (C % 8 || ld % 4 || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(planes) & 15) || (plane_stride & 7))
        return DML_EALIGN;
    if (layout == 0 ? (ldp % 8 != 0 || ldp < C) : (rows % 64 != 0 || C % 32 != 0)) return DML_EALIGN;
    if (layout != 0 && layout != 1) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // amax_known: the maximum over work[0 .. 1024) already is max |x| (or any bound within a few binades above it) -- the
    // producer of the tensor collected it there (dml_bn_apply / dml_bn_bwd_apply, `amax`): one pass over the tensor, not two
    const int nblk = amax_known ? H2_MAXBLK : grid_for(rows * (C / 4), 256, H2_MAXBLK);
    if (!amax_known) hipLaunchKernelGGL(h2_amax_kernel, dim3(nblk), dim3(256), 0, st, x, rows, C, ld, work);
    const int grid = grid_for(rows * (C / 8), 256);
    _Float16* pl = static_cast<_Float16*>(planes);
    if (layout == 0) hipLaunchKernelGGL(h2_split_kernel<0>, dim3(grid), dim3(256), 0, st, x, rows, C, ld, pl, plane_stride, ldp, work, nblk);
    else hipLaunchKernelGGL(h2_split_kernel<1>, dim3(grid), dim3(256), 0, st, x, rows, C, ld, pl, plane_stride, ldp, work, nblk);
    DML_LAUNCH_CHECK();
    return 0;
}

// the same for a table of tensors in two launches (every weight copy of a plan after each optimizer step: ~200 tensors, whose
// ~400 tiny launches cost ~2 ms of the step on the main stream)
namespace {
constexpr int H2_TABLE_BLK = 64;           // workgroups per tensor
__global__ __launch_bounds__(256) void h2_amax_table_kernel(const DmlH2Desc* __restrict__ table) {
    const DmlH2Desc d = table[blockIdx.y];
    const int cv = d.C >> 2;
    const int64_t total = d.rows * cv;
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)H2_TABLE_BLK * 256) {
        const int64_t r = i / cv;
        const int c = (int)(i - r * cv) * 4;
        const float4 v = *reinterpret_cast<const float4*>(d.x + r * d.ld + c);
        m = max(max(m, __float_as_uint(v.x) & 0x7fffffffu), max(__float_as_uint(v.y) & 0x7fffffffu, max(__float_as_uint(v.z) & 0x7fffffffu,
                                                                                               __float_as_uint(v.w) & 0x7fffffffu)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) d.work[blockIdx.x] = __uint_as_float(max(max(sh[0], sh[1]), max(sh[2], sh[3])));
}
__global__ __launch_bounds__(256) void h2_split_table_kernel(const DmlH2Desc* __restrict__ table) {
    const DmlH2Desc d = table[blockIdx.y];
    const float s = h2_scale_from(d.work, H2_TABLE_BLK);
    if (blockIdx.x == 0 && threadIdx.x == 0) d.work[H2_MAXBLK] = 1.0f / s;
    const int cv = d.C >> 3;
    const int64_t total = d.rows * cv;
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    _Float16* const planes = static_cast<_Float16*>(d.planes);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)H2_TABLE_BLK * 256) {
        const int64_t r = i / cv;
        const int c = (int)(i - r * cv) * 8;
        const float4 v0 = *reinterpret_cast<const float4*>(d.x + r * d.ld + c);
        const float4 v1 = *reinterpret_cast<const float4*>(d.x + r * d.ld + c + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xs = v[e] * s;
            const _Float16 h = (_Float16)xs;
            hi[e] = h;
            lo[e] = (_Float16)(xs - (float)h);
        }
        int64_t off;
        if (d.layout == 0) off = r * d.ldp + c;
        else off = (((r >> 6) * (d.C >> 5) + (c >> 5)) * 64 + (r & 63)) * 32 + (c & 31);
        *reinterpret_cast<h8*>(planes + off) = hi;
        *reinterpret_cast<h8*>(planes + d.plane_stride + off) = lo;
    }
}
}  // namespace

extern "C" int dml_h2_split_table(const DmlH2Desc* table_device, int count, void* stream) {
    if (!table_device || count <= 0) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(h2_amax_table_kernel, dim3(H2_TABLE_BLK, count), dim3(256), 0, st, table_device);
    hipLaunchKernelGGL(h2_split_table_kernel, dim3(H2_TABLE_BLK, count), dim3(256), 0, st, table_device);
    DML_LAUNCH_CHECK();
    return 0;
}

// ---- space-to-depth form of a k x k stride-2 convolution on few channels (the stem: 7x7 s2 on 3 channels) -----------------
// out[yo][xo] = sum_{t,u,c} w[t][u][c] x[2 yo - p + t][2 xo - p + u][c], p = (k - 1) / 2 odd.  With x2[y2][x2][(dy 2 + dx) C + c] =
// x[2 y2 + dy][2 x2 + dx][c] (half the map, 4 C channels) and t = 2 r2 + dy - 1, u = 2 s2 + dx - 1 this is a (k + 1) / 2 square
// STRIDE-1 convolution with padding (p + 1) / 2 on x2 whose taps outside 0 .. k - 1 carry zero weights: K = 4 C ((k + 1) / 2)^2 --
// 192 for the stem -- instead of the 8 k^2 = 392 of the image padded to 8 channels (16-byte vectors per tap).  Same products;
// the exact-fp32 stem forward 1.36 -> 0.66 ms, its weight gradient 2.81 -> 1.42 ms (tools/probe_stem_s2d.py).
namespace {
__global__ __launch_bounds__(256) void pack_input_s2d_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int H, int W) {
    const int H2 = H >> 1, W2 = W >> 1, C4 = 4 * C;
    const int64_t total = (int64_t)B * H2 * W2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / ((int64_t)H2 * W2);
        const int64_t rem = i - b * H2 * W2;
        const int y2 = (int)(rem / W2), x2 = (int)(rem - (int64_t)y2 * W2);
        float* o = y + i * C4;
        for (int c = 0; c < C; ++c) {
            const float* src = x + ((b * C + c) * H + 2 * y2) * W + 2 * x2;
            o[c] = src[0]; o[C + c] = src[1]; o[2 * C + c] = src[W]; o[3 * C + c] = src[W + 1];      // (any alignment of the image)
        }
    }
}
// w[N][k][k][C] <-> w2[N][k2][k2][4 C]; TO_S2D: w2 = gather(w) (zero taps outside), else: w += scatter(w2) (the weight gradient)
template <bool TO_S2D>
__global__ __launch_bounds__(256) void s2d_weights_kernel(float* __restrict__ w, float* __restrict__ w2, int N, int k, int C) {
    const int k2 = (k + 1) / 2, C4 = 4 * C, off = 2 * (((k - 1) / 2 + 1) / 2) - (k - 1) / 2;      // t = 2 r2 + dy - off
    const int total = N * k2 * k2 * C4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i % C4, s2 = (i / C4) % k2, r2 = (i / (C4 * k2)) % k2, n = i / (C4 * k2 * k2);
        const int c = j % C, dx = (j / C) & 1, dy = j / (2 * C);
        const int t = 2 * r2 + dy - off, u = 2 * s2 + dx - off;
        const bool in = t >= 0 && t < k && u >= 0 && u < k;
        const int wi = ((n * k + t) * k + u) * C + c;
        if (TO_S2D) w2[i] = in ? w[wi] : 0.f;
        else if (in) w[wi] += w2[i];
    }
}
}  // namespace

// sub-filter of a weight copy: dst[row][j][0 .. n) = src[row][taps[j]][0 .. n), j < ntaps <= 4 (dml_gather_taps)
namespace {
__global__ __launch_bounds__(256) void gather_taps_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int taps_src,
                                                          int n, int ntaps, int t0, int t1, int t2, int t3) {
    const int n4 = n >> 2;
    const int64_t total = (int64_t)rows * ntaps * n4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(i % n4), j = (int)((i / n4) % ntaps);
        const int64_t row = i / ((int64_t)n4 * ntaps);
        const int t = j == 0 ? t0 : (j == 1 ? t1 : (j == 2 ? t2 : t3));
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[(row * taps_src + t) * n4 + v];
    }
}
}  // namespace

extern "C" int dml_gather_taps(const float* src, float* dst, int rows, int taps_src, int n, int ntaps, int t0, int t1, int t2, int t3,
                               void* stream) {
    if (!src || !dst || rows <= 0 || taps_src <= 0 || n <= 0 || ntaps <= 0 || ntaps > 4) return DML_EINVAL;
    const int t[4] = {t0, t1, t2, t3};
    for (int j = 0; j < ntaps; ++j)
        if (t[j] < 0 || t[j] >= taps_src) return DML_EINVAL;
    if ((n & 3) || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15)) return DML_EALIGN;
    hipLaunchKernelGGL(gather_taps_kernel, dim3(grid_for((int64_t)rows * ntaps * (n >> 2), 256, 256 * 16)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, dst, rows, taps_src, n, ntaps, t0, t1, t2, t3);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_pack_input_s2d(const float* x_nchw, float* y, int B, int C, int H, int W, void* stream) {
    if (!x_nchw || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if ((H | W) & 1) return DML_EALIGN;
    hipLaunchKernelGGL(pack_input_s2d_kernel, dim3(grid_for((int64_t)B * (H / 2) * (W / 2), 256, 256 * 16)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x_nchw, y, B, C, H, W);
    DML_LAUNCH_CHECK();
    return 0;
}
extern "C" int dml_s2d_weights(const float* w, float* w2, int N, int k, int C, void* stream) {
    if (!w || !w2 || N <= 0 || C <= 0 || k < 3 || (k & 1) == 0 || (((k - 1) / 2) & 1) == 0) return DML_EINVAL;
    const int k2 = (k + 1) / 2;
    hipLaunchKernelGGL(s2d_weights_kernel<true>, dim3(grid_for((int64_t)N * k2 * k2 * 4 * C, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), const_cast<float*>(w), w2, N, k, C);
    DML_LAUNCH_CHECK();
    return 0;
}
extern "C" int dml_s2d_wgrad(const float* dw2, float* dw, int N, int k, int C, void* stream) {
    if (!dw2 || !dw || N <= 0 || C <= 0 || k < 3 || (k & 1) == 0 || (((k - 1) / 2) & 1) == 0) return DML_EINVAL;
    const int k2 = (k + 1) / 2;
    hipLaunchKernelGGL(s2d_weights_kernel<false>, dim3(grid_for((int64_t)N * k2 * k2 * 4 * C, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dw, const_cast<float*>(dw2), N, k, C);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_unpad_wgrad(const float* src, float* dst, int N, int RS, int Cm, int Cp, void* stream) {
    if (!src || !dst || Cp < Cm) return DML_EINVAL;
    hipLaunchKernelGGL(unpad_wgrad_kernel, dim3(grid_for((int64_t)N * RS * Cm, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, dst, N, RS, Cm, Cp);
    DML_LAUNCH_CHECK();
    return 0;
}

// ws == nullptr: one launch, fp32 atomics across workgroups (order-dependent in the last bit).  With a workspace of at least
// 1024 * N floats: partial sums per workgroup, then a fixed-order fold -- deterministic.
static int bias_grad_impl(const void* dy, float* db, int64_t M, int N, int ldy, int dtype, float* ws, int64_t ws_elems,
                          void* stream) {
    if (!dy || !db || M <= 0 || N <= 0 || N > 256) return DML_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int V = dtype == DML_BF16 ? 8 : 4;
    if (N % V == 0 && ldy % V == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0) {
        const int64_t rpb = (M + 1023) / 1024;
        const int grid = (int)((M + rpb - 1) / rpb);
        if (ws != nullptr && (int64_t)grid * N > ws_elems) return DML_EINVAL;
        if (dtype == DML_BF16)
            hipLaunchKernelGGL(bias_grad_vec_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)dy, db, M, N, ldy,
                               (int)rpb, ws);
        else
            hipLaunchKernelGGL(bias_grad_vec_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)dy, db, M, N, ldy,
                               (int)rpb, ws);
        if (ws != nullptr) hipLaunchKernelGGL(bias_grad_fold_kernel, dim3(1), dim3(256), 0, st, ws, db, grid, N);
        DML_LAUNCH_CHECK();
        return 0;
    }
    const int rt = 256 / N;
    int grid = grid_for((M + rt - 1) / rt, 1, 512);
    if (ws != nullptr && (int64_t)grid * rt * N > ws_elems) grid = (int)(ws_elems / ((int64_t)rt * N));
    if (grid < 1) return DML_EINVAL;
    if (dtype == DML_BF16)
        hipLaunchKernelGGL(bias_grad_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)dy, db, M, N, ldy, ws);
    else
        hipLaunchKernelGGL(bias_grad_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)dy, db, M, N, ldy, ws);
    if (ws != nullptr) hipLaunchKernelGGL(bias_grad_fold_kernel, dim3(1), dim3(256), 0, st, ws, db, grid * rt, N);
    DML_LAUNCH_CHECK();
    return 0;
}

extern "C" int dml_bias_grad(const void* dy, float* db, int64_t M, int N, int ldy, int dtype, void* stream) {
    return bias_grad_impl(dy, db, M, N, ldy, dtype, nullptr, 0, stream);
}

extern "C" int dml_bias_grad_ws(const void* dy, float* db, int64_t M, int N, int ldy, int dtype, float* ws, int64_t ws_elems,
                                void* stream) {
    if (!ws || ws_elems < (int64_t)N) return DML_EINVAL;
    return bias_grad_impl(dy, db, M, N, ldy, dtype, ws, ws_elems, stream);
}

extern "C" int dml_pack_input(const float* x_nchw, void* y_nhwc, int B, int C, int H, int W, int Cp, int dtype,
                              void* stream) {
    if (!x_nchw || !y_nhwc || B <= 0 || C <= 0 || Cp < C) return DML_EINVAL;
    const int64_t HW = (int64_t)H * W;
    const int grid = grid_for(B * HW, 256, 256 * 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DML_BF16)
        hipLaunchKernelGGL(pack_input_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, x_nchw, (bf16_t*)y_nhwc, B, C, HW,
                           Cp);
    else
        hipLaunchKernelGGL(pack_input_kernel<float>, dim3(grid), dim3(256), 0, st, x_nchw, (float*)y_nhwc, B, C, HW,
                           Cp);
    DML_LAUNCH_CHECK();
    return 0;
}
