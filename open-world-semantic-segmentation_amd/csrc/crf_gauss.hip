// Dense CRF with one spatial Gaussian pairwise term (anomaly/eval_ood_traditional.py:492-510 of the reference, `--ood crf-gauss`:
// pydensecrf's DenseCRF2D, unary_from_softmax, addPairwiseGaussian(sxy = 3, compat = 3), inference(100), max over the classes).
// The reference runs the permutohedral lattice on one CPU thread per frame; the lattice approximates a Gaussian filter, and a 2-D
// Gaussian is separable, so a mean-field step here is the exact filter as two 1-D passes and a softmax over the classes:
//
//   U_c = -log(min(max(softmax_c(L), clip), 1))                       kx(d) = exp(-d^2 / (2 sx^2)), |d| <= Rx = ceil(6 sx); ky alike
//   nx(x) = 1 / sqrt(sum_x' kx(x - x')), ny(y) alike, x', y' inside the image (densecrf's symmetric normalisation, which factorises)
//   T_c(y, x)  = ny(y) sum_x' kx(x - x') nx(x') Q_c(y, x')                                               (row pass)
//   M_c(y, x)  = ny(y) nx(x) sum_y' ky(y - y') T_c(y', x)                                                (column pass)
//   Q^0 = softmax_c(-U),  Q^{t+1} = softmax_c(-U + compat M(Q^t)),  conf = max_c Q^iters, map = argmax_c Q^iters
//
// 1 + 2 iters launches ordered by the stream and by nothing else (no cooperative grid, no flag, no atomic): the init launch writes U,
// Q^0, the two tap tables and nx, ny; each step is a row launch Q -> T and a column launch T, U -> Q; the last column launch (the
// init launch when iters = 0) writes conf and map instead of Q.  Per step and unit of B C H W 4 bytes: Q read, T written, T read
// (plus the halo rows of the column tile, from cache), U read, Q written = 5 units.
//
// Every sum runs over its taps in ascending x' (y') with fmaf, whatever the tile a pixel falls into: a tap outside the image or
// beyond the radius adds an exact +0.  Bitwise reproducible, and image b of a batch equals that image alone.
#include "common.h"

#include <cmath>

namespace {

constexpr int CRF_MAXR = 48;        // ceil(6 sigma), sigma <= 8
constexpr int CRF_TAB = 128;        // floats of one tap table
// tap tables, zero outside |d| <= R: wx[i] = kx(i - Rpx - CRF_XPAD) (Rpx = Rx rounded up to 4; read up to i = 2 Rpx + 7 <= 103),
// wy[i] = ky(i - Ry - CRF_YPAD) (read up to i = 2 Ry + 14 <= 110)
constexpr int CRF_XPAD = 3, CRF_YPAD = 7;
constexpr int CRF_ROW_TX = 256, CRF_ROW_TY = 4;     // row pass: a workgroup owns 4 rows x 256 columns, a lane 4 adjacent columns
constexpr int CRF_COL_TX = 64;                      // column pass: 64 columns x 4 V rows, a lane V rows of one column

__host__ __device__ constexpr int crf_rp(int R) { return (R + 3) & ~3; }

__device__ __forceinline__ float crf_tap(int d, float inv2s2) { return expf(-(float)(d * d) * inv2s2); }

// q_c = exp(a_c - max a) / sum_c exp(a_c - max a), in place.  No contraction: the init launch and the column launch must give the
// same bits for the same a (compat = 0 returns Q^0 after any number of steps).
template <int CMAX> __device__ __forceinline__ void crf_softmax(float (&a)[CMAX], int C) {
#pragma clang fp contract(off)
    float m = a[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C) m = fmaxf(m, a[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) {
            a[c] = expf(a[c] - m);
            s += a[c];
        }
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) a[c] = a[c] / s;
}

// conf = max_c q_c, map = the lowest c that reaches it
template <int CMAX>
__device__ __forceinline__ void crf_write_result(const float (&q)[CMAX], int C, float* conf, int64_t* map, int64_t i) {
    float best = q[0];
    int arg = 0;
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C && q[c] > best) { best = q[c]; arg = c; }
    conf[i] = best;
    if (map) map[i] = arg;
}

// grid (pixel workgroups + 1, B): the last workgroup of image 0 writes the tables, the last of the other images has nothing to do
__global__ __launch_bounds__(256) void crf_init_kernel(const float* __restrict__ logits, float* __restrict__ U,
                                                       float* __restrict__ Q, float* __restrict__ conf,
                                                       int64_t* __restrict__ map, float* __restrict__ tabs, int K, int k_first,
                                                       int H, int W, float inv2sx2, float inv2sy2, int Rx, int Ry, float clip,
                                                       int last) {
    const int C = K - k_first, b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    if (blockIdx.x == gridDim.x - 1) {
        if (b != 0) return;
        float* wx = tabs;
        float* wy = tabs + CRF_TAB;
        float* nx = tabs + 2 * CRF_TAB;
        float* ny = nx + W;
        const int Rpx = crf_rp(Rx);
        for (int i = threadIdx.x; i < CRF_TAB; i += blockDim.x) {
            const int dx = i - Rpx - CRF_XPAD, dy = i - Ry - CRF_YPAD;
            wx[i] = (dx >= -Rx && dx <= Rx) ? crf_tap(dx, inv2sx2) : 0.f;
            wy[i] = (dy >= -Ry && dy <= Ry) ? crf_tap(dy, inv2sy2) : 0.f;
        }
        for (int x = threadIdx.x; x < W; x += blockDim.x) {
            const int lo = x - Rx < 0 ? 0 : x - Rx, hi = x + Rx > W - 1 ? W - 1 : x + Rx;
            float s = 0.f;
            for (int xx = lo; xx <= hi; ++xx) s += crf_tap(xx - x, inv2sx2);
            nx[x] = 1.f / sqrtf(s);
        }
        for (int y = threadIdx.x; y < H; y += blockDim.x) {
            const int lo = y - Ry < 0 ? 0 : y - Ry, hi = y + Ry > H - 1 ? H - 1 : y + Ry;
            float s = 0.f;
            for (int yy = lo; yy <= hi; ++yy) s += crf_tap(yy - y, inv2sy2);
            ny[y] = 1.f / sqrtf(s);
        }
        return;
    }
    const float* img = logits + ((int64_t)b * K + k_first) * HW;
    const int64_t obase = (int64_t)b * C * HW;
    for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < HW;
         pix += (int64_t)(gridDim.x - 1) * blockDim.x) {
        float a[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) a[c] = img[(int64_t)c * HW + pix];
        crf_softmax<MAXC>(a, C);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) {
                const float u = -logf(fminf(fmaxf(a[c], clip), 1.f));
                U[obase + (int64_t)c * HW + pix] = u;
                a[c] = -u;
            }
        crf_softmax<MAXC>(a, C);
        if (last) {
            crf_write_result<MAXC>(a, C, conf, map, (int64_t)b * HW + pix);
        } else {
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) Q[obase + (int64_t)c * HW + pix] = a[c];
        }
    }
}

// T(r, x) = ny(y) sum_x' kx(x - x') nx(x') Q(r, x') over the `rows` = B C H rows of Q, y = r % H.  LDS: 4 rows of
// 256 + 2 Rp <= 352 floats = 5632 bytes, static; A holds nx(x') Q(r, x'), 0 outside the image.  A lane reads the 2 Rp + 4 values its four outputs span as 16-byte
// vectors (lane stride 16 bytes: conflict-free) and takes the taps from the table through uniform (scalar) loads.
// VEC: W % 4 == 0 and a 16-byte aligned workspace -- whole vectors are inside or outside the image as one.
template <bool VEC>
__global__ __launch_bounds__(256) void crf_row_kernel(const float* __restrict__ Q, float* __restrict__ T,
                                                      const float* __restrict__ wx, const float* __restrict__ nx,
                                                      const float* __restrict__ ny, int64_t rows, int H, int W, int Rp,
                                                      int tiles_x, int64_t tiles) {
    __shared__ __attribute__((aligned(16))) float A[CRF_ROW_TY * (CRF_ROW_TX + 2 * CRF_MAXR)];
    const int WA = CRF_ROW_TX + 2 * Rp;
    const int tid = threadIdx.x, lx = tid & 63, r = tid >> 6;
    const int nq = Rp / 2 + 1;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = (tile / tiles_x) * CRF_ROW_TY;
        const int tx0 = (int)(tile % tiles_x) * CRF_ROW_TX;
        if constexpr (VEC) {
            const int wv = WA / 4;
            for (int it = tid; it < CRF_ROW_TY * wv; it += 256) {
                const int rr = it / wv, c = (it - rr * wv) * 4;
                const int gx = tx0 - Rp + c;
                const int64_t gr = row0 + rr;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gr < rows && gx >= 0 && gx < W) {          // gx % 4 == 0 and W % 4 == 0: gx + 3 < W as well
                    const float4 q = *reinterpret_cast<const float4*>(Q + gr * W + gx);
                    const float4 n = *reinterpret_cast<const float4*>(nx + gx);
                    v = make_float4(q.x * n.x, q.y * n.y, q.z * n.z, q.w * n.w);
                }
                *reinterpret_cast<float4*>(A + rr * WA + c) = v;
            }
        } else {
            for (int it = tid; it < CRF_ROW_TY * WA; it += 256) {
                const int rr = it / WA, c = it - rr * WA;
                const int gx = tx0 - Rp + c;
                const int64_t gr = row0 + rr;
                float v = 0.f;
                if (gr < rows && gx >= 0 && gx < W) v = Q[gr * W + gx] * nx[gx];
                A[rr * WA + c] = v;
            }
        }
        __syncthreads();
        // value e of vector q sits d = 4 q + e - k - Rp columns from output k: tap wx[4 q + e - k + 3]
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* base = A + r * WA + 4 * lx;
        for (int q = 0; q < nq; ++q) {
            const float4 v4 = *reinterpret_cast<const float4*>(base + 4 * q);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            const float* w = wx + 4 * q;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[e - k + CRF_XPAD], v[e], acc[k]);
        }
        const int64_t gr = row0 + r;
        const int gx = tx0 + 4 * lx;
        if (gr < rows) {
            float* o = T + gr * W + gx;
            const float n = ny[gr % H];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] *= n;
            if constexpr (VEC) {
                if (gx < W) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < W) o[k] = acc[k];
            }
        }
        __syncthreads();
    }
}

// M_c(y, x) = ny(y) nx(x) sum_y' ky(y - y') T_c(y', x) with the row launch's T (ny(y') is in it), then
// Q_c = softmax_c(-U_c + compat M_c) (last: conf and map).  A workgroup owns 64 columns x 4 V rows of one image, a lane V
// consecutive rows of one column; the V * C messages of a lane stay in registers (CMAX 16 with V = 8, CMAX 32 with V = 4: 128
// accumulators).  LDS: one channel's tile with its halo, 0 outside the image -- (4 V + 2 RMAX) * 64 floats, RMAX = 24 or 48 the
// largest radius of the instantiation: at most 32768 bytes, static.  A wave stages the same (4 V + 2 RMAX) / 4 rows whatever R is
// (rows beyond the halo are loaded from a clamped address and never read back), so the staging has no branch.  Lanes of a wave read 64 adjacent floats of one LDS row: conflict-free.  Row t of a lane's span sits
// d = t - k - R rows from its output k: tap wy[t - k + 7], a uniform (scalar) load.  The tile of channel c + 1 is fetched into
// registers while channel c is summed, and the span is walked four rows at a time with the next four rows and their taps already
// on their way.
template <int CMAX, int V, int RMAX>
__global__ __launch_bounds__(256, 2) void crf_col_kernel(const float* __restrict__ T, const float* __restrict__ U,
                                                      float* __restrict__ Q, float* __restrict__ conf,
                                                      int64_t* __restrict__ map, const float* __restrict__ wy,
                                                      const float* __restrict__ nx, const float* __restrict__ ny, int C, int H,
                                                      int W, int R, float compat, int last, int tiles_x, int tiles) {
    constexpr int TY = 4 * V;
    constexpr int NS = (TY + 2 * RMAX) / 4;            // rows of the haloed tile one wave stages
    constexpr int NW = V + 3;                          // taps four rows of the span meet
    __shared__ float S[(TY + 2 * RMAX) * CRF_COL_TX];
    const int tx = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int64_t ibase = (int64_t)b * C * HW;
    // the span 2 R + V in whole groups of four rows: with an odd R two more rows are staged and meet zero taps
    const int rows = (TY + 2 * R + 3) & ~3, span = rows - TY + V;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * TY, gx = (tile % tiles_x) * CRF_COL_TX + tx;
        const int gxc = gx < W ? gx : W - 1;
        float m[CMAX][V];
        float nxt[NS];
        // always a load from inside the image (the address is clamped); what lies outside is multiplied by 0 on its way into the
        // LDS -- a product, not a select, and not here, so that the loads stay unconditional, leave together and are waited for
        // only after the sums of the channel before (T is finite)
        const float inx = gx < W ? 1.f : 0.f;
        auto fetch = [&](int c) {
            const float* Tc = T + ibase + (int64_t)c * HW + gxc;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int gy = ty0 - R + wv + 4 * j;
                const int gyc = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
                nxt[j] = Tc[(int64_t)gyc * W];
            }
        };
        fetch(0);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int gy = ty0 - R + wv + 4 * j;
                    S[(wv + 4 * j) * CRF_COL_TX + tx] = nxt[j] * ((gy >= 0 && gy < H) ? inx : 0.f);
                }
                __syncthreads();
                if (c + 1 < C) fetch(c + 1);
                float acc[V];
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] = 0.f;
                const float* col = S + wv * V * CRF_COL_TX + tx;
                // rows t0 .. t0 + 3 of the span and the taps wy[t0 + 7 - (V - 1) .. t0 + 10] they meet
                float dc[4], dn[4], wc[NW], wn[NW];
#pragma unroll
                for (int i = 0; i < 4; ++i) dc[i] = col[i * CRF_COL_TX];
#pragma unroll
                for (int i = 0; i < NW; ++i) wc[i] = wy[CRF_YPAD - (V - 1) + i];
                for (int t0 = 0; t0 < span; t0 += 4) {
                    if (t0 + 4 < span) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) dn[i] = col[(t0 + 4 + i) * CRF_COL_TX];
#pragma unroll
                        for (int i = 0; i < NW; ++i) wn[i] = wy[t0 + 4 + CRF_YPAD - (V - 1) + i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int k = 0; k < V; ++k) acc[k] = fmaf(wc[i + (V - 1) - k], dc[i], acc[k]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dc[i] = dn[i];
#pragma unroll
                    for (int i = 0; i < NW; ++i) wc[i] = wn[i];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) m[c][k] = acc[k];
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int gy = ty0 + wv * V + k;
            if (gy < H && gx < W) {
                const int64_t pix = (int64_t)gy * W + gx;
                const float scale = ny[gy] * nx[gx];
                float a[CMAX];
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) a[c] = fmaf(compat, scale * m[c][k], -U[ibase + (int64_t)c * HW + pix]);
                crf_softmax<CMAX>(a, C);
                if (last) {
                    crf_write_result<CMAX>(a, C, conf, map, (int64_t)b * HW + pix);
                } else {
#pragma unroll
                    for (int c = 0; c < CMAX; ++c)
                        if (c < C) Q[ibase + (int64_t)c * HW + pix] = a[c];
                }
            }
        }
    }
}

template <int CMAX, int V, int RMAX>
void crf_col_launch(const float* T, const float* U, float* Q, float* conf, int64_t* map, const float* tabs, int B, int C, int H,
                    int W, int R, float compat, int last, hipStream_t st) {
    const int tiles_x = (W + CRF_COL_TX - 1) / CRF_COL_TX;
    // H W <= 2^40 keeps this below 2^31
    const int64_t tiles = (int64_t)tiles_x * ((H + 4 * V - 1) / (4 * V));
    const dim3 grid((unsigned)(tiles < (1 << 20) ? tiles : (1 << 20)), (unsigned)B);
    hipLaunchKernelGGL((crf_col_kernel<CMAX, V, RMAX>), grid, dim3(256), 0, st, T, U, Q, conf, map, tabs + CRF_TAB, tabs + 2 * CRF_TAB,
                       tabs + 2 * CRF_TAB + W, C, H, W, R, compat, last, tiles_x, (int)tiles);
}

// the checks the two entry points share; 0 = a supported call
int crf_check_shape(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return DML_EINVAL;
    if (C > MAXC || B > 65535) return DML_EUNSUPPORTED;
    // the image index is the grid's y; 2^40 pixels keep every offset (x 32 channels x 3 tensors x 4 bytes) inside int64
    if ((int64_t)H * W > (1ll << 40) / B) return DML_EUNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int64_t dml_crf_gauss_workspace_bytes(int B, int C, int H, int W) {
    const int rc = crf_check_shape(B, C, H, W);
    if (rc) return rc;
    return 4 * (3 * (int64_t)B * C * H * W + H + W + 2 * CRF_TAB);
}

extern "C" int dml_crf_gauss(const float* logits, float* conf, int64_t* map, void* work, int B, int K, int H, int W,
                             int k_first, float sx, float sy, float compat, int iters, float clip, void* stream) {
    if (!logits || !conf || !work || K <= 0 || k_first < 0 || k_first >= K || iters < 0) return DML_EINVAL;
    if (!(sx > 0.f) || !(sy > 0.f) || !(clip > 0.f) || !(clip < 1.f)) return DML_EINVAL;
    const int C = K - k_first;
    const int rc = crf_check_shape(B, C, H, W);
    if (rc) return rc;
    if (sx > CRF_MAXR / 6.f || sy > CRF_MAXR / 6.f) return DML_EUNSUPPORTED;
    const int Rx = (int)std::ceil(6.0 * (double)sx), Ry = (int)std::ceil(6.0 * (double)sy);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W, N = (int64_t)B * C * HW;
    float* U = static_cast<float*>(work);
    float* Q = U + N;
    float* T = Q + N;
    float* tabs = T + N;                 // wx[128], wy[128], nx[W], ny[H]
    const float inv2sx2 = (float)(1.0 / (2.0 * (double)sx * (double)sx)), inv2sy2 = (float)(1.0 / (2.0 * (double)sy * (double)sy));
    hipLaunchKernelGGL(crf_init_kernel, dim3(grid_for(HW, 256, 2048) + 1, B), dim3(256), 0, st, logits, U, Q, conf, map, tabs, K,
                       k_first, H, W, inv2sx2, inv2sy2, Rx, Ry, clip, iters == 0 ? 1 : 0);
    // with W % 4 == 0 every row of Q and T and the nx table keep the workspace's alignment
    const bool vec = W % 4 == 0 && aligned16(work);
    const int Rpx = crf_rp(Rx);
    const int row_tiles_x = (W + CRF_ROW_TX - 1) / CRF_ROW_TX;
    const int64_t rows = (int64_t)B * C * H;
    const int64_t row_tiles = row_tiles_x * ((rows + CRF_ROW_TY - 1) / CRF_ROW_TY);
    const dim3 row_grid((unsigned)(row_tiles < (1 << 20) ? row_tiles : (1 << 20)));
    for (int it = 0; it < iters; ++it) {
        const int last = it == iters - 1 ? 1 : 0;
        if (vec)
            hipLaunchKernelGGL(crf_row_kernel<true>, row_grid, dim3(256), 0, st, Q, T, tabs, tabs + 2 * CRF_TAB,
                               tabs + 2 * CRF_TAB + W, rows, H, W, Rpx, row_tiles_x, row_tiles);
        else
            hipLaunchKernelGGL(crf_row_kernel<false>, row_grid, dim3(256), 0, st, Q, T, tabs, tabs + 2 * CRF_TAB,
                               tabs + 2 * CRF_TAB + W, rows, H, W, Rpx, row_tiles_x, row_tiles);
        if (C <= 16 && Ry <= 24) crf_col_launch<16, 8, 24>(T, U, Q, conf, map, tabs, B, C, H, W, Ry, compat, last, st);
        else if (C <= 16) crf_col_launch<16, 8, CRF_MAXR>(T, U, Q, conf, map, tabs, B, C, H, W, Ry, compat, last, st);
        else if (Ry <= 24) crf_col_launch<32, 4, 24>(T, U, Q, conf, map, tabs, B, C, H, W, Ry, compat, last, st);
        else crf_col_launch<32, 4, CRF_MAXR>(T, U, Q, conf, map, tabs, B, C, H, W, Ry, compat, last, st);
    }
    DML_LAUNCH_CHECK();
    return 0;
}
