// Open-set prediction and its threshold sweep (anomaly/eval_ood_traditional.py:155-156,227-229,537-549,599-607 of the reference;
// DeepLabV3Plus-Pytorch/test_embedding.py:385-386): the closed-set arg-max with every pixel whose confidence is below a threshold
// relabelled "unknown", scored as a (K+1)-class segmentation, for T thresholds in one read of the three maps.
//
// For sorted thresholds t_0 < ... < t_{T-1} the open-set prediction of a pixel depends on them only through
// j = #{i : conf >= t_i}, so one histogram over (label, pred, j) -- the cube, T + 1 bins along j -- holds the confusion matrices of
// all T thresholds (the identity is in the header).  A workgroup counts its pixels in uint32 LDS cells sized by the actual
// n_classes and T and adds the non-zero ones to the int64 cube with integer atomics: the sums are exact and order-free, so the
// result is bitwise reproducible.  20 bytes per pixel are read once, 8 more are written when the prediction itself is wanted.
#include "common.h"

#include <cmath>

namespace {

constexpr int SWEEP_MAX_T = 12, SWEEP_MAX_OUT = 8, SWEEP_MAX_CLASSES = 33;
constexpr int SWEEP_THREADS = 256, SWEEP_PX = 8;                 // a lane holds 8 pixels of a pass, 256 apart: 24 loads in flight
constexpr int SWEEP_SPAN = SWEEP_THREADS * SWEEP_PX;             // pixels of one workgroup's pass (dmlnet/_lib.py OPEN_SWEEP_SPAN)
// two workgroups per CU: each zeroes and flushes up to 33 * 33 * 13 cells, so a frame is cut into few, long workgroups
constexpr int SWEEP_MAX_BLOCKS = 512;                            // (dmlnet/_lib.py OPEN_SWEEP_MAX_BLOCKS)

struct SweepArgs {
    float t[SWEEP_MAX_T];            // entries from T on are NaN: they compare false and add nothing to j
    int64_t out[SWEEP_MAX_OUT];
    float t_write;                   // t[write_idx], for open_pred
    int n_out, T, n_classes, unknown_id;
};

template <bool CUBE, bool WRITE>
__global__ __launch_bounds__(SWEEP_THREADS) void open_sweep_kernel(const float* __restrict__ conf, const int64_t* __restrict__ pred,
                                                                   const int64_t* __restrict__ label, int64_t n, SweepArgs a,
                                                                   unsigned long long* __restrict__ cube,
                                                                   int64_t* __restrict__ open_pred) {
    extern __shared__ uint32_t cells[];
    const int nc = a.n_classes, bins = a.T + 1, n_cells = nc * nc * bins;
    if (CUBE) {
        for (int i = threadIdx.x; i < n_cells; i += SWEEP_THREADS) cells[i] = 0u;
        __syncthreads();
    }
    for (int64_t base = (int64_t)blockIdx.x * SWEEP_SPAN; base < n; base += (int64_t)gridDim.x * SWEEP_SPAN) {
        float c[SWEEP_PX];
        int64_t q[SWEEP_PX], l[SWEEP_PX];
#pragma unroll
        for (int k = 0; k < SWEEP_PX; ++k) {
            const int64_t p = base + k * SWEEP_THREADS + threadIdx.x;
            const bool in = p < n;
            c[k] = in ? conf[p] : 0.f;
            q[k] = in ? pred[p] : -1;
            l[k] = (CUBE && in) ? label[p] : -1;
        }
#pragma unroll
        for (int k = 0; k < SWEEP_PX; ++k) {
            const int64_t p = base + k * SWEEP_THREADS + threadIdx.x;
            if (p >= n) continue;
            if (CUBE) {
                int64_t lab = l[k];
#pragma unroll
                for (int o = 0; o < SWEEP_MAX_OUT; ++o)
                    if (o < a.n_out && l[k] == a.out[o]) lab = a.unknown_id;
                int j = 0;
#pragma unroll
                for (int i = 0; i < SWEEP_MAX_T; ++i) j += c[k] >= a.t[i] ? 1 : 0;
                if (lab >= 0 && lab < nc && q[k] >= 0 && q[k] < nc)
                    atomicAdd(&cells[((int)lab * nc + (int)q[k]) * bins + j], 1u);
            }
            if (WRITE) open_pred[p] = c[k] >= a.t_write ? q[k] : (int64_t)a.unknown_id;
        }
    }
    if (CUBE) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += SWEEP_THREADS)
            if (cells[i]) atomicAdd(cube + i, (unsigned long long)cells[i]);
    }
}

}  // namespace

extern "C" int dml_open_set_sweep(const float* conf, const int64_t* pred, const int64_t* label, int64_t n,
                                  const float* thresholds, int T, const int64_t* out_labels, int n_out, int n_classes,
                                  int unknown_id, int64_t* cube, int64_t* open_pred, int write_idx, void* stream) {
    if (!conf || !pred || !thresholds || n < 0 || (!cube && !open_pred) || (cube && !label)) return DML_EINVAL;
    if (T < 1 || T > SWEEP_MAX_T || n_classes < 2 || n_classes > SWEEP_MAX_CLASSES || unknown_id < 0 || unknown_id >= n_classes)
        return DML_EINVAL;
    if (n_out < 0 || n_out > SWEEP_MAX_OUT || (n_out > 0 && !out_labels)) return DML_EINVAL;
    if (open_pred && (write_idx < 0 || write_idx >= T)) return DML_EINVAL;
    if (std::isnan(thresholds[0])) return DML_EINVAL;
    for (int i = 1; i < T; ++i)
        if (!(thresholds[i] > thresholds[i - 1])) return DML_EINVAL;      // equal, descending or NaN
    if ((reinterpret_cast<uintptr_t>(conf) & 3) ||
        ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(cube) |
          reinterpret_cast<uintptr_t>(open_pred)) & 7))
        return DML_EALIGN;
    if (n == 0) return 0;
    SweepArgs a;
    for (int i = 0; i < SWEEP_MAX_T; ++i) a.t[i] = i < T ? thresholds[i] : NAN;
    for (int o = 0; o < SWEEP_MAX_OUT; ++o) a.out[o] = o < n_out ? out_labels[o] : 0;
    a.n_out = n_out;
    a.T = T;
    a.n_classes = n_classes;
    a.unknown_id = unknown_id;
    a.t_write = open_pred ? thresholds[write_idx] : NAN;
    const int64_t passes = (n + SWEEP_SPAN - 1) / SWEEP_SPAN;
    const int blocks = (int)(passes < SWEEP_MAX_BLOCKS ? passes : SWEEP_MAX_BLOCKS);
    // a workgroup's uint32 cells cannot overflow: it sees at most ceil(passes / blocks) * SWEEP_SPAN pixels
    if ((passes + blocks - 1) / blocks >= (1ll << 32) / SWEEP_SPAN) return DML_EUNSUPPORTED;
    const size_t lds = cube ? sizeof(uint32_t) * n_classes * n_classes * (T + 1) : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* cu = reinterpret_cast<unsigned long long*>(cube);
    if (cube && open_pred)
        hipLaunchKernelGGL((open_sweep_kernel<true, true>), dim3(blocks), dim3(SWEEP_THREADS), lds, st, conf, pred, label, n, a, cu,
                           open_pred);
    else if (cube)
        hipLaunchKernelGGL((open_sweep_kernel<true, false>), dim3(blocks), dim3(SWEEP_THREADS), lds, st, conf, pred, label, n, a, cu,
                           open_pred);
    else
        hipLaunchKernelGGL((open_sweep_kernel<false, true>), dim3(blocks), dim3(SWEEP_THREADS), lds, st, conf, pred, label, n, a, cu,
                           open_pred);
    DML_LAUNCH_CHECK();
    return 0;
}
