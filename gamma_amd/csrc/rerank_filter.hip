// rerank_filter.hip -- the exact re-rank of a dense fp32 raw store with a filter in front: a one-byte image of the rows proves most
// of a query's R candidates out of its first k + 1, and only the survivors get the reference's fvec_L2sqr / fvec_inner_product
// over their fp32 rows (k_rerank_topk's arithmetic, rerank.hip).  Results are those of k_rerank_topk, bit for bit.
//
// The image.  Row y of the store is kept as u8[d] with y^_j = lo_j + Delta u_j (lo: per dimension, Delta: one per store, both
// fixed when the image is created from the rows then present; a value outside [lo_j, lo_j + 255 Delta] clamps) and two fp32 words
//     err >= |y - y^|_2                 (whatever the clamp did: an outlier only has a large err and always survives)
//     nrm >= |y|_2 + Delta |u|_2
// lane l of the 8 lanes of a candidate loads bytes 16 l .. 16 l + 15 of each 128-byte piece of the row: one 16-byte load.
//
// The bound (u = 2^-24, gamma_n = n u / (1 - n u), n <= d / 8 + 4 <= 196 for d <= 1536; M = kRerankFilterMargin = 2^-15 = 512 u).
// L2.  The kernel computes x'_j = fl(x_j - lo_j) once per query, t_j = fma(-Delta, u_j, x'_j) and est = sum t_j^2 (fma chain of a
//   lane, then a tree over the 8 lanes).  With t* = x - y^ exactly: t_j = t*_j + e_j, |e_j| <= u |x_j - lo_j| + (u + u^2) |t_j|, so
//   | |t| - |t*| | <= |e| <= 1.01 u (|x - lo| + |t|); est = |t|^2 (1 + th), |th| <= gamma_n; rt = sqrtf(est) = |t| (1 + th / 2)(1 + u).
//   The triangle inequality gives | |x - y| - |t*| | <= err.  Together | |x - y| - rt | <= err + (gamma_n / 2 + 3 u)(rt + xn) with
//   xn >= |x - lo|, which is below err + 0.21 M (rt + xn).  The kernel takes slack = err + M (rt + xn),
//       ub = (rt + slack)^2 (1 + M),   lb = max(rt - slack, 0)^2 (1 - M);
//   the reference's value is |x - y|^2 (1 + th'), |th'| <= gamma_(n + 2) < 0.39 M, and the few roundings of slack, ub and lb
//   themselves (each <= u relative) fit into what is left of M: lb <= exact <= ub.
// Inner product.  est = fma(Delta, S, c0), S = sum x_j u_j (the same chain), c0 = sum x_j lo_j once per query.  Against <x, y^>:
//   |est - <x, y^>| <= (gamma_n + 2 u) |x| (|lo| + Delta |u|); Cauchy-Schwarz: |<x, y> - <x, y^>| <= |x| err; the reference's value
//   differs from <x, y> by at most gamma_n |x| |y|.  With xn >= |x| and lon >= |lo|:
//       slack = xn (err + M (nrm + lon)),   ub = est + slack,   lb = est - slack
//   (the three gamma terms come to < 400 u (nrm + lon) |x|; err <= nrm + lon, so the roundings of slack and of est +- slack are
//   covered by the remaining 112 u).
// A NaN or an overflow anywhere makes lb, ub or both NaN or infinite in the direction of "survives": every test below is written
// so that a NaN comparison keeps the candidate.
//
// The filter.  "Certainly inside the score window": ub <= max_score and lb >= min_score.  tau = the K1-th best upper bound (L2:
// smallest ub; inner product: largest lb) among candidates certainly inside, K1 = min(k + 1, R); none when fewer than K1 are
// (which candidates it is taken among -- the first 64 or all of them -- is a matter of cost: the kernel says where).
// A candidate survives unless it is certainly outside the window or its lb lies beyond tau (L2: lb > tau; inner product:
// ub < tau).  K1 candidates have an exact in-window value within tau, a non-survivor's exact value is strictly beyond it: it is
// neither among the first K1 items nor equal to one of them, so the first K1 items -- all that is read -- are k_rerank_topk's.
//
// Timing builds (results invalid, never committed switched on; what they measured: DESIGN.md section 29): -DGH_RERANK_TIMING=1
// k_rerank_topk's d = 128 row loads replaced by a constant (rerank.hip); here 2 = no err / nrm loads, 3 = no exact phase, 4 = no
// survivor counter, 5 = no image loads; 6 = results valid, thread 0 of one workgroup in 16 reads the clock (100 MHz) between the
// phases and the sums are printed every 20 launches (with -DGH_RERANK_TIMING_FORM=1 the workgroup kernel runs throughout).
#include <hip/hip_runtime.h>
#include <stdint.h>
#if GH_RERANK_TIMING == 6
#include <stdio.h>
#endif

#include <algorithm>

#include "block_utils.h"
#include "device_math.h"
#include "kernels.h"
#include "rerank_dev.h"
#include "rerank_topk_dev.h"

namespace gh {

namespace {
constexpr float kM = kRerankFilterMargin;

__device__ __forceinline__ float group8_sum(float a) {
    a += __shfl_down(a, 4, 8);
    a += __shfl_down(a, 2, 8);
    return a + __shfl_down(a, 1, 8);
}
__device__ __forceinline__ float byte_f(uint32_t w, int b) { return (float)((w >> (8 * b)) & 0xffu); }

// sum over the workgroup (256 threads), the same value on every thread; red: 4 floats of LDS
__device__ __forceinline__ float block_sum256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

#if GH_RERANK_TIMING == 6
// [i] = clock ticks between marks i and i + 1, summed over the timed workgroups; [15] = their number.  Marks: 0 start, 1 ids and
// query staged, 2 estimates in LDS, 3 bounds (err / nrm landed), 4 tau, 5 survivors listed, 6 their rows measured, 7 first K1
// items sorted, 8 output written
__device__ unsigned long long g_phase_clk[16];
#define GH_CLK_DECL unsigned long long clk[9]; const bool clk_on = threadIdx.x == 0 && (blockIdx.x & 15) == 0
#define GH_CLK(i) do { if (clk_on) clk[i] = wall_clock64(); } while (0)
#define GH_CLK_END do { if (clk_on) { for (int i_ = 0; i_ < 8; i_++) atomicAdd(g_phase_clk + i_, clk[i_ + 1] - clk[i_]); atomicAdd(g_phase_clk + 15, 1ull); } } while (0)
#else
#define GH_CLK_DECL
#define GH_CLK(i)
#define GH_CLK_END
#endif
}  // namespace

// ---- the image's parameters -----------------------------------------------------------------------------------------------------
// par: [0, d) lo | [d] Delta | [d + 1] lon | then 2 d uint32 keys (running minimum, running maximum per dimension, f2key order)
__global__ __launch_bounds__(256) void k_img_minmax_init(uint32_t* __restrict__ keys, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < d) {
        keys[j] = 0xffffffffu;
        keys[d + j] = 0u;
    }
}
// grid (d / 64 rounded up, row slices): thread (ty, tx) folds rows of its slice, finite values only
__global__ __launch_bounds__(256) void k_img_minmax(const float* __restrict__ rows, int64_t n, int d, uint32_t* __restrict__ keys) {
    __shared__ uint32_t s_lo[4][64], s_hi[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + tx;
    uint32_t lo = 0xffffffffu, hi = 0u;
    if (j < d)
        for (int64_t r = (int64_t)blockIdx.y * 4 + ty; r < n; r += (int64_t)gridDim.y * 4) {
            const float v = rows[r * d + j];
            if (fabsf(v) < INFINITY) {   // (false for NaN)
                const uint32_t kk = f2key(v);
                lo = min(lo, kk);
                hi = max(hi, kk);
            }
        }
    s_lo[ty][tx] = lo;
    s_hi[ty][tx] = hi;
    __syncthreads();
    if (ty == 0 && j < d) {
        lo = min(min(s_lo[0][tx], s_lo[1][tx]), min(s_lo[2][tx], s_lo[3][tx]));
        hi = max(max(s_hi[0][tx], s_hi[1][tx]), max(s_hi[2][tx], s_hi[3][tx]));
        atomicMin(keys + j, lo);
        atomicMax(keys + d + j, hi);
    }
}
// one workgroup: lo_j = the minimum (0 for a dimension without a finite value), Delta = the widest range / 255 (1 when that is
// zero or not finite: any positive Delta is a valid image), lon = |lo| rounded up.  Every extremum an integer and no range
// beyond 255 -- SIFT-like descriptors, pixel data -- : Delta = 1, the image of integer rows is then exact.
__global__ __launch_bounds__(256) void k_img_params(float* __restrict__ par, int d) {
    __shared__ float red[4];
    const uint32_t* keys = reinterpret_cast<const uint32_t*>(par + d + 2);
    float span = 0.f, ss = 0.f;
    int whole = 1;
    for (int j = threadIdx.x; j < d; j += 256) {
        const uint32_t kl = keys[j], kh = keys[d + j];
        float lo = 0.f, w = 0.f;
        if (kl <= kh) {
            lo = key2f(kl);
            w = key2f(kh) - lo;
        }
        par[j] = lo;
        if (kl <= kh && !(lo == rintf(lo) && w == rintf(w))) whole = 0;
        span = fmaxf(span, w);
        ss = __builtin_fmaf(lo, lo, ss);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) span = fmaxf(span, __shfl_down(span, o, 64));
    ss = block_sum256(ss, red);   // (its barriers order the span exchange below as well)
    whole = __syncthreads_and(whole);
    __shared__ float smax[4];
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = span;
    __syncthreads();
    if (threadIdx.x == 0) {
        span = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        float delta = span / 255.0f;
        if (!(delta > 0.f) || !(delta < INFINITY) || (whole && span <= 255.0f)) delta = 1.0f;
        par[d] = delta;
        par[d + 1] = sqrtf(ss) * (1.0f + kM);
    }
}

// ---- rows -> image rows: eight lanes per row, lane l the 16-element pieces l, l + 8, ..  (d % 16 == 0) ----------------------------
// rows i of [0, n): store row vids[i] (vids != nullptr; outside [0, nrows) skipped) or first + i
__global__ __launch_bounds__(256) void k_img_quantise(const float* __restrict__ rows, const int64_t* __restrict__ vids, int64_t first,
                                                      int64_t n, int d, const float* __restrict__ par, uint8_t* __restrict__ img,
                                                      float2* __restrict__ aux, int64_t nrows) {
    const int l = threadIdx.x & 7;
    const int64_t i = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    int64_t row = -1;
    if (i < n) row = vids ? vids[i] : first + i;
    const bool live = row >= 0 && row < nrows;
    const float delta = par[d], inv = 1.0f / delta;
    float sr = 0.f, syl = 0.f, sy = 0.f, su = 0.f;
    if (live) {
        const float* y = rows + row * d;
        for (int c = l; c < (d >> 4); c += 8) {
            uint32_t w[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const float4 f = *reinterpret_cast<const float4*>(y + 16 * c + 4 * v);
                const float4 lo = *reinterpret_cast<const float4*>(par + 16 * c + 4 * v);
                const float yy[4] = {f.x, f.y, f.z, f.w}, ll[4] = {lo.x, lo.y, lo.z, lo.w};
                w[v] = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const float yl = __fsub_rn(yy[b], ll[b]);
                    const float uf = fminf(fmaxf(rintf(__fmul_rn(yl, inv)), 0.0f), 255.0f);   // (NaN -> 0: err is NaN then)
                    const float r = __builtin_fmaf(-delta, uf, yl);
                    sr = __builtin_fmaf(r, r, sr);
                    syl = __builtin_fmaf(yl, yl, syl);
                    sy = __builtin_fmaf(yy[b], yy[b], sy);
                    su = __builtin_fmaf(uf, uf, su);
                    w[v] |= (uint32_t)uf << (8 * b);
                }
            }
            *reinterpret_cast<uint4*>(img + row * d + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    sr = group8_sum(sr), syl = group8_sum(syl), sy = group8_sum(sy), su = group8_sum(su);
    if (live && l == 0) {
        const float err = __builtin_fmaf(kM, sqrtf(syl), sqrtf(sr)) * (1.0f + kM);
        const float nrm = __builtin_fmaf(delta, sqrtf(su), sqrtf(sy)) * (1.0f + kM);
        aux[row] = make_float2(err, nrm);
    }
}

void launch_rerank_image_params(hipStream_t s, const float* rows, int64_t n, int d, float* par) {
    if (d <= 0) return;
    uint32_t* keys = reinterpret_cast<uint32_t*>(par + d + 2);
    hipLaunchKernelGGL(k_img_minmax_init, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, keys, d);
    if (n > 0) {
        const unsigned gy = (unsigned)std::min<int64_t>((n + 63) / 64, 2048);
        hipLaunchKernelGGL(k_img_minmax, dim3((unsigned)((d + 63) / 64), gy), dim3(256), 0, s, rows, n, d, keys);
    }
    hipLaunchKernelGGL(k_img_params, dim3(1), dim3(256), 0, s, par, d);
}
void launch_rerank_image_rows(hipStream_t s, const float* rows, const int64_t* vids, int64_t first, int64_t n, int d, const float* par,
                              uint8_t* img, float* aux, int64_t nrows) {
    if (n <= 0 || d <= 0 || nrows <= 0) return;
    if (d % 16 != 0) {
        launch_refused("launch_rerank_image_rows: d is not a multiple of 16");
        return;
    }
    hipLaunchKernelGGL(k_img_quantise, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, s, rows, vids, first, n, d, par, img,
                       reinterpret_cast<float2*>(aux), nrows);
}

// ---- the re-rank ---------------------------------------------------------------------------------------------------------------------
// One workgroup per query, as k_rerank_topk.  D128: d == 128, the lane's 16 query elements in registers in both phases.
template <bool L2, bool D128>
__global__ __launch_bounds__(256) void k_rerank_topk_filt(const float* __restrict__ x, int d, const float* __restrict__ raw, int64_t nraw,
                                                          const uint8_t* __restrict__ img, const float2* __restrict__ aux,
                                                          const float* __restrict__ par, const int64_t* __restrict__ cand_ids, int R,
                                                          int k, float min_score, float max_score, float neutral,
                                                          float* __restrict__ distances, int64_t* __restrict__ labels, int nq,
                                                          const int* __restrict__ qperm, TieFlags tf,
                                                          unsigned long long* __restrict__ stat) {
    __shared__ unsigned long long s_it[1024];
    __shared__ int64_t s_id[1024];
    __shared__ float s_bd[1024];            // the candidates' estimates
    __shared__ unsigned short s_sv[1024];   // the survivors' candidate ranks
    __shared__ __attribute__((aligned(16))) float s_x[D128 ? 128 : kRerankFilterMaxD];   // L2: x - lo, inner product: x
    __shared__ float s_red[4];
    __shared__ float s_tau;
    __shared__ int s_tie, s_nsv;
    GH_CLK_DECL;
    GH_CLK(0);
    int q = blockIdx.x;   // (the query order: k_rerank_topk)
    if (qperm) {
        const int qi = (blockIdx.x & 7) * ((nq + 7) >> 3) + (blockIdx.x >> 3);
        if (qi >= nq) return;
        q = qperm[qi];
    } else if (q >= nq) {
        return;
    }
    const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
    const float* xq = x + (int64_t)q * d;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const float delta = par[d], lon = par[d + 1];
    for (int r = threadIdx.x; r < R; r += 256) s_id[r] = cand_ids[(int64_t)q * R + r];
    if (threadIdx.x == 0) s_nsv = 0;
    // the query as the filter reads it, its norm and (inner product) <x, lo>
    float sq = 0.f, sc = 0.f;
    for (int j = threadIdx.x; j < d; j += 256) {
        const float xv = xq[j];
        const float v = L2 ? __fsub_rn(xv, par[j]) : xv;
        s_x[j] = v;
        sq = __builtin_fmaf(v, v, sq);
        if (!L2) sc = __builtin_fmaf(xv, par[j], sc);
    }
    const float xn = sqrtf(block_sum256(sq, s_red)) * (1.0f + kM);
    float c0 = 0.f;
    if (!L2) c0 = block_sum256(sc, s_red);   // (uniform)
    // (block_sum256's barriers: s_id, s_x and s_nsv are in place)
    GH_CLK(1);

    // ---- phase 1: estimates from the image, eight lanes per candidate; then every candidate's bounds by a thread of its own ----
    if constexpr (D128) {
        float xx[16];
#pragma unroll
        for (int u = 0; u < 16; u++) xx[u] = s_x[16 * l + u];
        for (int r0 = 0; r0 < R; r0 += 128) {
            uint4 w[4];
#pragma unroll
            for (int f = 0; f < 4; f++) {
                const int r = r0 + 32 * f + g;
                const int64_t id = r < R ? s_id[r] : -1;
                w[f] = make_uint4(0, 0, 0, 0);
#if GH_RERANK_TIMING == 5   // timing build (results invalid): no image loads
                w[f] = make_uint4((uint32_t)id, l, f, 7);
#else
                if (id >= 0 && id < nraw) w[f] = *reinterpret_cast<const uint4*>(img + id * 128 + 16 * l);
#endif
            }
#pragma unroll
            for (int f = 0; f < 4; f++) {
                const uint32_t ww[4] = {w[f].x, w[f].y, w[f].z, w[f].w};
                float a = 0.f;
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const float uf = byte_f(ww[u >> 2], u & 3);
                    if (L2) {
                        const float t = __builtin_fmaf(-delta, uf, xx[u]);
                        a = __builtin_fmaf(t, t, a);
                    } else {
                        a = __builtin_fmaf(xx[u], uf, a);
                    }
                }
                a = group8_sum(a);
                if (l == 0 && r0 + 32 * f + g < R) s_bd[r0 + 32 * f + g] = a;
            }
        }
    } else {
        const int nc = d >> 4;
        for (int r0 = 0; r0 < R; r0 += 32) {
            const int r = r0 + g;
            const int64_t id = r < R ? s_id[r] : -1;
            const bool live = id >= 0 && id < nraw;
            float a = 0.f;
            if (live) {
                const uint8_t* yr = img + id * d;
                for (int c = l; c < nc; c += 8) {
                    const uint4 w = *reinterpret_cast<const uint4*>(yr + 16 * c);
                    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        const float4 xv = *reinterpret_cast<const float4*>(s_x + 16 * c + 4 * v);
                        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const float uf = byte_f(ww[v], b);
                            if (L2) {
                                const float t = __builtin_fmaf(-delta, uf, xs[b]);
                                a = __builtin_fmaf(t, t, a);
                            } else {
                                a = __builtin_fmaf(xs[b], uf, a);
                            }
                        }
                    }
                }
            }
            a = group8_sum(a);
            if (l == 0 && r < R) s_bd[r] = a;
        }
    }
    __syncthreads();   // every estimate is in s_bd
    GH_CLK(2);
    float bd[4];      // L2: lb, inner product: ub -- the bound tau is held against
    bool alive[4];    // not certainly outside the window
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int r = threadIdx.x + 256 * u;
        bd[u] = 0.f;
        alive[u] = false;
        if (r < R) {
            const int64_t id = s_id[r];
            const bool live = id >= 0 && id < nraw;
            float2 ax = make_float2(0.f, 0.f);
#if GH_RERANK_TIMING == 2   // timing build (results invalid): no err / nrm loads
            if (live) ax = make_float2(0.1f, 1000.0f);
#else
            if (live) ax = aux[id];
#endif
            const float a = s_bd[r];
            float lb, ub;
            if (L2) {
                const float rt = sqrtf(a);
                const float slack = __builtin_fmaf(kM, rt + xn, ax.x);
                const float ur = rt + slack, lr = fmaxf(rt - slack, 0.0f);
                ub = ur * ur * (1.0f + kM);
                lb = lr * lr * (1.0f - kM);
            } else {
                const float est = __builtin_fmaf(delta, a, c0);
                const float slack = xn * __builtin_fmaf(kM, ax.y + lon, ax.x);
                ub = est + slack;
                lb = est - slack;
            }
            const bool inside = live && ub <= max_score && lb >= min_score;
            alive[u] = live && !(lb > max_score || ub < min_score);
            const uint32_t key = L2 ? f2key(ub) : ~f2key(lb);
            s_it[r] = inside ? (((unsigned long long)key << 32) | (unsigned)r) : ~0ull;
            bd[u] = L2 ? lb : ub;
        }
    }
    GH_CLK(3);
    if (threadIdx.x == 0) {
        if (tf.list) s_tie = tf.cut ? tf.cut[q] : 0;
        s_tau = sentinel;   // (fewer than K1 certainly inside: nothing is proven out)
    }
    // tau: any value that K1 candidates certainly inside have their upper bound within.  Up to K1 = 16 of more than 64 candidates:
    // the K1-th best among the first 64 -- the candidates come in ADC order, so it nearly always is the K1-th best of all, and one
    // wave sorts 64 items once; otherwise the K1-th best of all (rerank_first_k).
    const int K1 = min(k + 1, R);
    const bool head = K1 <= 16 && R > 64;   // (uniform)
    if (head) {
        __syncthreads();
        if (threadIdx.x < 64) {
            const unsigned long long it = wave_sort64(s_it[threadIdx.x]);
            const uint32_t key = (uint32_t)(it >> 32);
            if ((int)threadIdx.x == K1 - 1 && key != 0xffffffffu) s_tau = key2f(L2 ? key : ~key);
        }
    } else {
        rerank_first_k(s_it, R, K1);
        if (threadIdx.x == 0) {
            const uint32_t key = (uint32_t)(s_it[K1 - 1] >> 32);
            if (key != 0xffffffffu) s_tau = key2f(L2 ? key : ~key);
        }
    }
    __syncthreads();
    const float tau = s_tau;
    GH_CLK(4);
    const uint32_t skey = L2 ? f2key(sentinel) : ~f2key(sentinel);
    bool sv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) sv[u] = alive[u] && !(L2 ? bd[u] > tau : bd[u] < tau);
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int r = threadIdx.x + 256 * u;
        if (256 * u < R) {   // (uniform)
            const unsigned long long bal = __ballot(sv[u]);
            const int lane = threadIdx.x & 63;
            int base = 0;
            if (lane == 0 && bal) base = atomicAdd(&s_nsv, __popcll(bal));
            base = __shfl(base, 0, 64);
            if (sv[u]) s_sv[base + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)r;
            else if (r < R) s_it[r] = ((unsigned long long)skey << 32) | (unsigned)r;   // as an out-of-window exact distance
        }
    }
    __syncthreads();
    GH_CLK(5);
#if GH_RERANK_TIMING == 3   // timing build (results invalid): no survivor gets its exact distance
    const int m = 0;
#else
    const int m = s_nsv;
#endif
    // the survivors, counted: one atomic per query, spread over kRerankFilterStatLines words that lie a 128-byte line apart (two
    // atomics per query on 2 x 16 neighbouring words took 70 us of a 16384-query launch: they queue up per line)
#if GH_RERANK_TIMING != 4   // (4: timing build without the counter)
    if (threadIdx.x == 0 && stat) atomicAdd(stat + 16 * (blockIdx.x & (kRerankFilterStatLines - 1)), (unsigned long long)m);
#endif

    // ---- phase 2: k_rerank_topk's arithmetic over the survivors (in any order: an item's place is its candidate rank) ----
    auto put = [&](int r, float dis) {
        if (l == 0) {
            if (!(dis <= max_score && dis >= min_score)) dis = sentinel;
            const uint32_t key = L2 ? f2key(dis) : ~f2key(dis);
            s_it[r] = ((unsigned long long)key << 32) | (unsigned)r;
        }
    };
    if constexpr (D128) {
        float xx[16];
#pragma unroll
        for (int u = 0; u < 16; u++) xx[u] = xq[l + 8 * u];
        // (one candidate per group and round -- there are few -- and a wave none of whose groups has one sits the round out)
        for (int c0_ = 0; c0_ < m; c0_ += 32) {
            if (c0_ + (g & ~7) >= m) continue;   // (uniform over the wave)
            const int c = c0_ + g;
            const bool live = c < m;
            const int r = live ? s_sv[c] : 0;
            const float* v = raw + (live ? s_id[r] : 0) * 128 + l;
            float fa[16];
#pragma unroll
            for (int u = 0; u < 16; u++) fa[u] = v[8 * u];
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++) {
                if (L2) {
                    const float t = xx[u] - fa[u];
                    a = __builtin_fmaf(t, t, a);
                } else {
                    a = __builtin_fmaf(xx[u], fa[u], a);
                }
            }
            const float sa = __shfl_down(a, 4, 8) + a;
            const float ta = sa + __shfl_down(sa, 1, 8);
            const float da = ta + __shfl_down(ta, 2, 8);
            if (live) put(r, da);
        }
    } else {
        for (int c0_ = 0; c0_ < m; c0_ += 32) {
            if (c0_ + (g & ~7) >= m) continue;   // (uniform over the wave)
            const int c = c0_ + g;
            const bool live = c < m;
            const int r = live ? s_sv[c] : 0;
            const float dis = rerank_dist8<L2>(xq, raw + (live ? s_id[r] : 0) * d, d, l, live);
            if (live) put(r, dis);
        }
    }
    GH_CLK(6);
    // the first K1 items: up to 64 survivors are sorted by one wave (every other item carries the sentinel key, as do the places
    // the survivors leave empty); more of them: k_rerank_topk's way
    if (m <= 64) {
        __syncthreads();   // the survivors' items are in s_it
        if (threadIdx.x < 64) {
            const unsigned long long it = wave_sort64((int)threadIdx.x < m ? s_it[s_sv[threadIdx.x]] : ~0ull);
            if ((int)threadIdx.x < K1) s_it[threadIdx.x] = it != ~0ull ? it : ((unsigned long long)skey << 32);
        }
        __syncthreads();
    } else {
        rerank_first_k(s_it, R, K1);
    }
    GH_CLK(7);
    rerank_topk_out<L2>(s_it, s_id, &s_tie, q, R, k, neutral, distances, labels, tf);
    GH_CLK(8);
    GH_CLK_END;
}

// ---- the wave form: d == 128, R <= 256, K1 <= 64 ----------------------------------------------------------------------------------
// One wave owns one query from its ids to its output and waits for no other wave: no workgroup barrier, 3.5 KB of LDS per wave
// (ids, estimates / exact keys, the survivor list), so a CU holds as many queries as it holds waves.  The values are those of
// k_rerank_topk_filt: the same x - lo, xn and c0 (the same sums in the same order), the same estimates, bounds, tau (the head
// rule included), survivor test and exact arithmetic.  What differs is where things stand:
//   * lane i holds candidate i + 64 u, u < 4: its id, its {err, nrm} -- requested with the ids in hand, in front of the image
//     loads and not behind the estimates --, its bounds and its (key, rank) item, all in registers;
//   * eight candidates per round (eight groups of eight lanes), four rounds' image loads in flight;
//   * tau and the first K1 items come from wave_sort64 over one run, or -- more than one run: K1 > 16 for tau, more than 64
//     survivors at the end -- from the sorting network over all 256 items in registers (wave_sort_net).  The items are distinct
//     (the rank field), so the first K1 of any ascending sort are rerank_first_k's.
// One wave per workgroup, so workgroup b is query b of the order and runs on XCD b & 7 as k_rerank_topk_filt's does.  (Four
// waves per workgroup, each on its own, measured slower: DESIGN.md section 31.)
constexpr int kRerankWaveMaxR = 256;

__device__ __forceinline__ float wave_sum_first(float v) {   // block_sum256's sum over one wave, the value of lane 0 on every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

template <bool L2>
__global__ __launch_bounds__(64) void k_rerank_topk_filt_wave(const float* __restrict__ x, const float* __restrict__ raw, int64_t nraw,
                                                                   const uint8_t* __restrict__ img, const float2* __restrict__ aux,
                                                                   const float* __restrict__ par, const int64_t* __restrict__ cand_ids,
                                                                   int R, int k, float min_score, float max_score, float neutral,
                                                                   float* __restrict__ distances, int64_t* __restrict__ labels, int nq,
                                                                   const int* __restrict__ qperm, TieFlags tf,
                                                                   unsigned long long* __restrict__ stat) {
    __shared__ int64_t s_id[kRerankWaveMaxR];
    __shared__ uint32_t s_bd[kRerankWaveMaxR];         // the candidates' estimates; then the survivors' exact keys
    __shared__ unsigned short s_sv[kRerankWaveMaxR];   // the survivors' candidate ranks
    GH_CLK_DECL;
    GH_CLK(0);
    const int lane = threadIdx.x;
    int q = blockIdx.x;   // (the query order: k_rerank_topk)
    if (qperm) {
        const int qi = (blockIdx.x & 7) * ((nq + 7) >> 3) + (blockIdx.x >> 3);
        if (qi >= nq) return;
        q = qperm[qi];
    } else if (q >= nq) {
        return;
    }
    const int l = lane & 7, g = lane >> 3;
    const float* xq = x + (int64_t)q * 128;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const uint32_t skey = L2 ? f2key(sentinel) : ~f2key(sentinel);
    const int K1 = min(k + 1, R);
    // the query's loads go first: what waits for them below then does not wait for the {err, nrm} loads behind them
    float4 xv4[4], lo4[4];
    float xh[2], loh[2];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        xv4[v] = *reinterpret_cast<const float4*>(xq + 16 * l + 4 * v);
        lo4[v] = L2 ? *reinterpret_cast<const float4*>(par + 16 * l + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int h = 0; h < 2; h++) xh[h] = xq[lane + 64 * h], loh[h] = par[lane + 64 * h];
    const float delta = par[128], lon = par[129];
    // ids, and with them every candidate's {err, nrm}
    bool live[4];
    float2 ax[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int r = lane + 64 * u;
        const int64_t id = r < R ? cand_ids[(int64_t)q * R + r] : -1;
        if (64 * u < R) s_id[r] = id;   // (uniform)
        live[u] = id >= 0 && id < nraw;
        ax[u] = make_float2(0.f, 0.f);
        if (live[u]) ax[u] = aux[id];
    }
    int tie = 0;
    if (tf.list && tf.cut) tie = tf.cut[q];
    // the query as the filter reads it (lane l: elements 16 l ..), its norm and (inner product) <x, lo>: block_sum256's sums
    float xx[16];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        xx[4 * v] = xv4[v].x, xx[4 * v + 1] = xv4[v].y, xx[4 * v + 2] = xv4[v].z, xx[4 * v + 3] = xv4[v].w;
        if (L2) {
            xx[4 * v] = __fsub_rn(xv4[v].x, lo4[v].x), xx[4 * v + 1] = __fsub_rn(xv4[v].y, lo4[v].y);
            xx[4 * v + 2] = __fsub_rn(xv4[v].z, lo4[v].z), xx[4 * v + 3] = __fsub_rn(xv4[v].w, lo4[v].w);
        }
    }
    float sq[2], sc[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const float v = L2 ? __fsub_rn(xh[h], loh[h]) : xh[h];
        sq[h] = wave_sum_first(__builtin_fmaf(v, v, 0.f));
        sc[h] = L2 ? 0.f : wave_sum_first(__builtin_fmaf(xh[h], loh[h], 0.f));
    }
    const float xn = sqrtf((sq[0] + sq[1]) + 0.f) * (1.0f + kM);
    const float c0 = L2 ? 0.f : (sc[0] + sc[1]) + 0.f;
    wave_lds_sync();   // s_id
    GH_CLK(1);

    // ---- phase 1: estimates from the image, eight lanes per candidate ----
    for (int r0 = 0; r0 < R; r0 += 32) {
        uint4 w[4];
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const int r = r0 + 8 * f + g;
            const int64_t id = r < R ? s_id[r] : -1;
            w[f] = make_uint4(0, 0, 0, 0);
            if (id >= 0 && id < nraw) w[f] = *reinterpret_cast<const uint4*>(img + id * 128 + 16 * l);
        }
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const uint32_t ww[4] = {w[f].x, w[f].y, w[f].z, w[f].w};
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const float uf = byte_f(ww[u >> 2], u & 3);
                if (L2) {
                    const float t = __builtin_fmaf(-delta, uf, xx[u]);
                    a = __builtin_fmaf(t, t, a);
                } else {
                    a = __builtin_fmaf(xx[u], uf, a);
                }
            }
            a = group8_sum(a);
            if (l == 0 && r0 + 8 * f + g < R) s_bd[r0 + 8 * f + g] = __float_as_uint(a);
        }
    }
    wave_lds_sync();   // every estimate is in s_bd
    GH_CLK(2);
    // the bounds, where the candidate's {err, nrm} landed
    unsigned long long it[4];
    float bd[4];      // L2: lb, inner product: ub -- the bound tau is held against
    bool alive[4];    // not certainly outside the window
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int r = lane + 64 * u;
        it[u] = ~0ull;
        bd[u] = 0.f;
        alive[u] = false;
        if (r < R) {
            const float a = __uint_as_float(s_bd[r]);
            float lb, ub;
            if (L2) {
                const float rt = sqrtf(a);
                const float slack = __builtin_fmaf(kM, rt + xn, ax[u].x);
                const float ur = rt + slack, lr = fmaxf(rt - slack, 0.0f);
                ub = ur * ur * (1.0f + kM);
                lb = lr * lr * (1.0f - kM);
            } else {
                const float est = __builtin_fmaf(delta, a, c0);
                const float slack = xn * __builtin_fmaf(kM, ax[u].y + lon, ax[u].x);
                ub = est + slack;
                lb = est - slack;
            }
            const bool inside = live[u] && ub <= max_score && lb >= min_score;
            alive[u] = live[u] && !(lb > max_score || ub < min_score);
            const uint32_t key = L2 ? f2key(ub) : ~f2key(lb);
            if (inside) it[u] = ((unsigned long long)key << 32) | (unsigned)r;
            bd[u] = L2 ? lb : ub;
        }
    }
    GH_CLK(3);
    // tau (k_rerank_topk_filt says which candidates it is taken among)
    uint32_t tkey;
    if ((K1 <= 16 && R > 64) || R <= 64) {   // (uniform) one run: the head, or all there is
        tkey = (uint32_t)(wave_sort64(it[0]) >> 32);
    } else {
        unsigned long long t4[4] = {it[0], it[1], it[2], it[3]};
        wave_sort_net<4>(t4);
        tkey = (uint32_t)(t4[0] >> 32);
    }
    tkey = (uint32_t)__shfl((int)tkey, K1 - 1, 64);
    const float tau = tkey != 0xffffffffu ? key2f(L2 ? tkey : ~tkey) : sentinel;   // (fewer than K1 certainly inside: nothing is proven out)
    GH_CLK(4);
    // the survivors, compacted; every other candidate's item is that of an out-of-window exact distance
    bool sv[4];
    int m = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int r = lane + 64 * u;
        sv[u] = alive[u] && !(L2 ? bd[u] > tau : bd[u] < tau);
        it[u] = r < R ? (((unsigned long long)skey << 32) | (unsigned)r) : ~0ull;   // (padding sorts last)
        if (64 * u < R) {   // (uniform)
            const unsigned long long bal = __ballot(sv[u]);
            if (sv[u]) s_sv[m + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)r;
            m += __popcll(bal);
        }
    }
    // counted as k_rerank_topk_filt counts them: one atomic per query, on one of kRerankFilterStatLines words a line apart
    if (lane == 0 && stat) atomicAdd(stat + 16 * (blockIdx.x & (kRerankFilterStatLines - 1)), (unsigned long long)m);
    wave_lds_sync();   // s_sv
    GH_CLK(5);

    // ---- phase 2: k_rerank_topk's arithmetic over the survivors, one per group and round; the keys go to s_bd by rank ----
    {
        float x2[16];
#pragma unroll
        for (int u = 0; u < 16; u++) x2[u] = xq[l + 8 * u];
        for (int c0_ = 0; c0_ < m; c0_ += 8) {
            const int c = c0_ + g;
            const bool on = c < m;
            const int r = on ? s_sv[c] : 0;
            const float* v = raw + (on ? s_id[r] : 0) * 128 + l;
            float fa[16];
#pragma unroll
            for (int u = 0; u < 16; u++) fa[u] = v[8 * u];
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++) {
                if (L2) {
                    const float t = x2[u] - fa[u];
                    a = __builtin_fmaf(t, t, a);
                } else {
                    a = __builtin_fmaf(x2[u], fa[u], a);
                }
            }
            const float sa = __shfl_down(a, 4, 8) + a;
            const float ta = sa + __shfl_down(sa, 1, 8);
            float dis = ta + __shfl_down(ta, 2, 8);
            if (on && l == 0) {
                if (!(dis <= max_score && dis >= min_score)) dis = sentinel;
                s_bd[r] = L2 ? f2key(dis) : ~f2key(dis);
            }
        }
    }
    wave_lds_sync();   // the survivors' keys
    GH_CLK(6);
    // the first K1 items, one per lane
    unsigned long long first;
    if (m <= 64) {   // (uniform) every other item carries the sentinel key, as do the places the survivors leave empty
        unsigned long long mine = ~0ull;
        if (lane < m) {
            const unsigned r = s_sv[lane];
            mine = ((unsigned long long)s_bd[r] << 32) | r;
        }
        mine = wave_sort64(mine);
        first = mine != ~0ull ? mine : ((unsigned long long)skey << 32);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (sv[u]) it[u] = ((unsigned long long)s_bd[lane + 64 * u] << 32) | (unsigned)(lane + 64 * u);
        wave_sort_net<4>(it);
        first = it[0];
    }
    GH_CLK(7);
    rerank_topk_out_wave<L2>(first, s_id, tie, q, R, k, neutral, distances, labels, tf);
    GH_CLK(8);
    GH_CLK_END;
}

bool rerank_filter_wave_ok(int d, int R, int k) { return d == 128 && R >= 1 && R <= kRerankWaveMaxR && std::min(k + 1, R) <= 64; }

bool rerank_filter_shape_ok(int d, int R, int k) { return d > 0 && d % 16 == 0 && d <= kRerankFilterMaxD && R >= 1 && R <= 1024 && std::min(k + 1, R) <= 64; }

int launch_rerank_topk_filtered(hipStream_t s, bool l2, const float* x, int nq, int d, const float* raw, int64_t nraw, const uint8_t* img,
                                const float* aux, const float* par, const int64_t* cand_ids, int R, int k, float min_score,
                                float max_score, float neutral, float* distances, int64_t* labels, const int* qperm,
                                const TieFlags* ties, unsigned long long* stat, int form) {
    if (nq <= 0) return 0;
    if (!rerank_filter_shape_ok(d, R, k) || nraw <= 0 || form < 0 || form > 2) {
        launch_refused("launch_rerank_topk_filtered: a shape its caller rules out");
        return 0;
    }
    const TieFlags tf = ties ? *ties : TieFlags{};
    const float2* ax = reinterpret_cast<const float2*>(aux);
#if GH_RERANK_TIMING == 6   // timing build: the clock sums so far, every 20 launches
#ifdef GH_RERANK_TIMING_FORM
    form = GH_RERANK_TIMING_FORM;
#endif
    static int timed_launches = 0;   // (not thread-safe: a timing build is driven by one caller)
    if (++timed_launches % 20 == 0) {
        unsigned long long v[16];
        if (hipStreamSynchronize(s) == hipSuccess && hipMemcpyFromSymbol(v, HIP_SYMBOL(g_phase_clk), sizeof(v)) == hipSuccess && v[15]) {
            fprintf(stderr, "rerank phase clocks, form %d, %llu workgroups, mean ticks of 10 ns:", form, v[15]);
            for (int i = 0; i < 8; i++) fprintf(stderr, " %.1f", (double)v[i] / (double)v[15]);
            fprintf(stderr, "\n");
        }
    }
#endif
    if (rerank_filter_wave_ok(d, R, k) && (form == 2 || (form == 0 && nq >= kRerankWaveAutoMinNq))) {
        const dim3 grid((unsigned)(8 * ((nq + 7) / 8)));
#define GH_FILT_WAVE(L2_)                                                                                                            \
    hipLaunchKernelGGL((k_rerank_topk_filt_wave<L2_>), grid, dim3(64), 0, s, x, raw, nraw, img, ax, par, cand_ids, R, k, min_score,  \
                       max_score, neutral, distances, labels, nq, qperm, tf, stat)
        if (l2) GH_FILT_WAVE(true);
        else GH_FILT_WAVE(false);
#undef GH_FILT_WAVE
        return 2;
    }
    const dim3 grid((unsigned)(8 * ((nq + 7) / 8)));
#define GH_FILT(L2_, D128_)                                                                                                          \
    hipLaunchKernelGGL((k_rerank_topk_filt<L2_, D128_>), grid, dim3(256), 0, s, x, d, raw, nraw, img, ax, par, cand_ids, R, k,      \
                       min_score, max_score, neutral, distances, labels, nq, qperm, tf, stat)
    if (d == 128) {
        if (l2) GH_FILT(true, true);
        else GH_FILT(false, true);
    } else {
        if (l2) GH_FILT(true, false);
        else GH_FILT(false, false);
    }
#undef GH_FILT
    return 1;
}

}  // namespace gh
