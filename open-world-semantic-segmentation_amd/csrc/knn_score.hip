// kNN cosine-similarity anomaly score of the open-set driver (anomaly/eval_ood_traditional.py:511-530 of the reference, `--ood knn`):
// for every pixel the sum of the cosine similarities between its embedding and those of the R x R pixels down-right of it and the
// R x R pixels up-left of it, R = neighbor_size - 1; a neighbour outside the image counts 0.  One launch, no workspace, no atomics.
//
// With n(p) = f(p) / max(|f(p)|, 1e-8) the score is sum_c n_c(p) * S_c(p), S_c(p) = sum of n_c over the two quadrants, and S_c is
// separable: a workgroup owns a 16 x 64 output tile, keeps one channel plane of the tile plus its halo of R, already divided by
// the norms, in LDS, takes the row sums over x+1 .. x+R and x-R .. x-1 for every row of the haloed tile and then the column sums of
// those over y+1 .. y+R and y-R .. y-1: 4 R additions per pixel and channel instead of 2 R^2 products.  Every sum runs over the plain
// values in a fixed order (no sliding window, no prefix differences), so a pixel's result depends on nothing but its own
// neighbourhood: bitwise reproducible, the same in a batch and alone, exact integers for C = 1.
#include "common.h"

namespace {

constexpr int KNN_TY = 16, KNN_TX = 64, KNN_THREADS = 256;
constexpr int KNN_MAXR = 16;       // neighbor_size <= 17
constexpr int KNN_MAX_GRID = 16384;

__host__ __device__ constexpr int knn_rp(int R) { return (R + 3) & ~3; }   // halo columns kept left and right: R rounded up to whole 16-byte vectors

// RC > 0: R is the compile-time constant RC (the reference's 8: every loop below unrolls and the window tests fold); RC == 0: R is a
// launch argument, 1 .. KNN_MAXR.  VEC: W % 4 == 0 and both pointers 16-byte aligned -- 16-byte loads and stores on whole vectors that
// are inside or outside the image as one; otherwise one float per lane with a test per element.
template <int RC, bool VEC>
__global__ __launch_bounds__(KNN_THREADS) void knn_cosine_kernel(const float* __restrict__ feats, float* __restrict__ score, int C,
                                                                 int H, int W, int r_arg, int tiles_x, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float knn_lds[];
    constexpr int RMAX = RC > 0 ? RC : KNN_MAXR;
    constexpr int V = VEC ? 4 : 1;
    // haloed-tile elements (vectors) one thread stages per plane, for the largest R of this instantiation
    constexpr int NI = ((KNN_TY + 2 * RMAX) * (KNN_TX + 2 * knn_rp(RMAX)) / V + KNN_THREADS - 1) / KNN_THREADS;
    const int R = RC > 0 ? RC : r_arg;
    const int Rp = knn_rp(R);
    const int rows = KNN_TY + 2 * R;          // haloed rows
    const int WA = KNN_TX + 2 * Rp;           // haloed columns: image column tx0 - Rp + c, a multiple of 4
    const int items = rows * WA / V;
    float* A = knn_lds;                       // [rows][WA]    one channel of n = f / max(|f|, 1e-8); 0 outside the image
    float* HR = A + rows * WA;                // [rows][KNN_TX] sum of A over the R columns right of the output column
    float* HL = HR + rows * KNN_TX;           // [rows][KNN_TX] ... left of it
    const int tid = threadIdx.x;
    const int orow = tid >> 4, ox0 = (tid & 15) * 4;      // this thread's four output pixels: one row, four adjacent columns
    const int64_t plane = (int64_t)H * W;
    const float* fb = feats + (int64_t)blockIdx.y * C * plane;
    float* sb = score + (int64_t)blockIdx.y * plane;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * KNN_TY, tx0 = (tile % tiles_x) * KNN_TX;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (R > 0) {
            // step 1: max(|f|, 1e-8) of the haloed pixels this thread stages (it stages the same ones for every channel, so the
            // norms and the offsets stay in registers); off < 0 marks a pixel outside the image
            float den[NI][V];
            int64_t off[NI];
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int it = tid + j * KNN_THREADS;
                off[j] = -1;
#pragma unroll
                for (int e = 0; e < V; ++e) den[j][e] = 1.f;
                if (it < items) {
                    const int e0 = it * V, r = e0 / WA, c = e0 - r * WA;
                    const int gy = ty0 - R + r, gx = tx0 - Rp + c;
                    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {       // VEC: gx % 4 == 0 and W % 4 == 0, so gx + 3 < W as well
                        off[j] = (int64_t)gy * W + gx;
                        float ss[V];
#pragma unroll
                        for (int e = 0; e < V; ++e) ss[e] = 0.f;
                        const float* p = fb + off[j];
                        for (int ch = 0; ch < C; ++ch, p += plane) {
                            if constexpr (VEC) {
                                const float4 v = *reinterpret_cast<const float4*>(p);
                                ss[0] = fmaf(v.x, v.x, ss[0]); ss[1] = fmaf(v.y, v.y, ss[1]);
                                ss[2] = fmaf(v.z, v.z, ss[2]); ss[3] = fmaf(v.w, v.w, ss[3]);
                            } else {
                                ss[0] = fmaf(*p, *p, ss[0]);
                            }
                        }
#pragma unroll
                        for (int e = 0; e < V; ++e) den[j][e] = fmaxf(sqrtf(ss[e]), 1e-8f);
                    }
                }
            }

            // the plane of channel ch + 1 is fetched while channel ch is summed: `nxt` holds it from one pass of the loop to the next
            float nxt[NI][V];
            auto fetch = [&](int ch) {
                const float* pc = fb + (int64_t)ch * plane;
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    if (off[j] >= 0) {
                        if constexpr (VEC) {
                            const float4 v = *reinterpret_cast<const float4*>(pc + off[j]);
                            nxt[j][0] = v.x; nxt[j][1] = v.y; nxt[j][2] = v.z; nxt[j][3] = v.w;
                        } else {
                            nxt[j][0] = pc[off[j]];
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e) nxt[j][e] = 0.f;
                    }
                }
            };
            fetch(0);
            for (int ch = 0; ch < C; ++ch) {
                // (a) the haloed plane, divided by the norms (a true division: f / |f| is exactly +-1 for C = 1; outside the
                // image 0 / 1)
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int it = tid + j * KNN_THREADS;
                    if (it < items) {
                        if constexpr (VEC)
                            *reinterpret_cast<float4*>(A + it * 4) = make_float4(nxt[j][0] / den[j][0], nxt[j][1] / den[j][1],
                                                                                 nxt[j][2] / den[j][2], nxt[j][3] / den[j][3]);
                        else
                            A[it] = nxt[j][0] / den[j][0];
                    }
                }
                if (ch + 1 < C) fetch(ch + 1);
                __syncthreads();
                // (b) row sums: one (haloed row, four output columns) per step; the 2 Rp + 4 values the four windows span are read
                // once as 16-byte vectors.  Value t of the span sits d = t - k - Rp columns from output column k.
                const float4 ctr = *reinterpret_cast<const float4*>(A + (orow + R) * WA + Rp + ox0);
                const int nquad = Rp / 2 + 1;
                for (int it = tid; it < rows * (KNN_TX / 4); it += KNN_THREADS) {
                    const int r = it >> 4, x0 = (it & 15) * 4;
                    const float* base = A + r * WA + x0;
                    float hl[4] = {0.f, 0.f, 0.f, 0.f}, hr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < nquad; ++q) {
                        const float4 v4 = *reinterpret_cast<const float4*>(base + 4 * q);
                        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int d = 4 * q + e - k - Rp;
                                if (d >= -R && d <= -1) hl[k] += v[e];
                                if (d >= 1 && d <= R) hr[k] += v[e];
                            }
                    }
                    *reinterpret_cast<float4*>(HL + r * KNN_TX + x0) = make_float4(hl[0], hl[1], hl[2], hl[3]);
                    *reinterpret_cast<float4*>(HR + r * KNN_TX + x0) = make_float4(hr[0], hr[1], hr[2], hr[3]);
                }
                __syncthreads();
                // (c) column sums of the row sums: right windows of the R rows below, left windows of the R rows above
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 1; i <= R; ++i) {
                    const float4 h = *reinterpret_cast<const float4*>(HR + (orow + R + i) * KNN_TX + ox0);
                    s[0] += h.x; s[1] += h.y; s[2] += h.z; s[3] += h.w;
                }
#pragma unroll
                for (int i = 1; i <= R; ++i) {
                    const float4 h = *reinterpret_cast<const float4*>(HL + (orow + R - i) * KNN_TX + ox0);
                    s[0] += h.x; s[1] += h.y; s[2] += h.z; s[3] += h.w;
                }
                acc[0] = fmaf(ctr.x, s[0], acc[0]); acc[1] = fmaf(ctr.y, s[1], acc[1]);
                acc[2] = fmaf(ctr.z, s[2], acc[2]); acc[3] = fmaf(ctr.w, s[3], acc[3]);
                // the next (a) writes A only after every thread has passed the barrier behind (b); the next (b) writes HL / HR only
                // after the barrier behind that (a), which every thread reaches after its (c)
            }
        }
        const int gy = ty0 + orow, gx = tx0 + ox0;
        if (gy < H) {
            float* o = sb + (int64_t)gy * W + gx;
            if constexpr (VEC) {
                if (gx < W) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < W) o[k] = acc[k];
            }
        }
    }
}

template <int RC, bool VEC>
void knn_launch(const float* feats, float* score, int B, int C, int H, int W, int R, hipStream_t st) {
    const int tiles_x = (W + KNN_TX - 1) / KNN_TX;
    // B H W <= 2^40 keeps this below 2^31: H W / 1024 + H / 16 + W / 64 + 1
    const int64_t tiles = (int64_t)tiles_x * ((H + KNN_TY - 1) / KNN_TY);
    const int rows = KNN_TY + 2 * R, WA = KNN_TX + 2 * knn_rp(R);
    const size_t lds = (size_t)(rows * WA + 2 * rows * KNN_TX) * sizeof(float);        // 61440 bytes at R = 16
    const dim3 grid((unsigned)(tiles < KNN_MAX_GRID ? tiles : KNN_MAX_GRID), (unsigned)B);
    hipLaunchKernelGGL((knn_cosine_kernel<RC, VEC>), grid, dim3(KNN_THREADS), lds, st, feats, score, C, H, W, R, tiles_x,
                       (int)tiles);
}


}  // namespace

extern "C" int dml_knn_cosine_score(const float* feats, float* score, int B, int C, int H, int W, int neighbor_size,
                                    void* stream) {
    if (!feats || !score || B <= 0 || C <= 0 || H <= 0 || W <= 0 || neighbor_size < 1) return DML_EINVAL;
    if (C > MAXC || neighbor_size > KNN_MAXR + 1 || B > 65535) return DML_EUNSUPPORTED;
    // the image index is the grid's y; 2^40 pixels keep every element offset (x C, x 4 bytes) inside int64
    if ((int64_t)H * W > (1ll << 40) / B) return DML_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int R = neighbor_size - 1;
    const bool vec = W % 4 == 0 && aligned16(feats, score);
    if (R == 8 && vec) knn_launch<8, true>(feats, score, B, C, H, W, R, st);
    else if (R == 8) knn_launch<8, false>(feats, score, B, C, H, W, R, st);
    else if (vec) knn_launch<0, true>(feats, score, B, C, H, W, R, st);
    else knn_launch<0, false>(feats, score, B, C, H, W, R, st);
    DML_LAUNCH_CHECK();
    return 0;
}
