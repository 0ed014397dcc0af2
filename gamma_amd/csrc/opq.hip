// opq.hip -- the OPQ rotation (faiss::LinearTransform::apply_noalloc as GammaIVFPQIndex runs it in front of the coarse
// quantizer and the PQ encoder, index/impl/gamma_index_ivfpq.cc:375-512,514-566; faiss:VectorTransform.cpp:41-80):
// xt = x A^T, A d x d row-major.
//
// The arithmetic is OURS, fixed by contract (DESIGN.md "OPQ"): the reference's one sgemm_("T", "N", d, n, d, ..) call sums
// in an order its BLAS picks from the shape, so the same vector rotates to different bits in Update (n = 1) and Add
// (n = 1000) -- there is no reference bit pattern to restate.  Here every output element is ONE fp32 accumulator that
// starts at +0 and takes its d terms in ascending j, one fmaf each.  That is what v_mfma_f32_32x32x2_f32 computes per
// element (gemm.hip) and what the VALU kernel below spells out, so a row's result depends neither on n, nor on where the
// row sits in the batch, nor on the kernel that served it.  No split-K, no zero padding inside a chain (the matrix-pipe
// kernel issues d / 2 MFMAs per tile; it serves d % 4 == 0, every other d goes to the VALU kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "opq.h"

namespace gh {

typedef float opq_f32x16 __attribute__((ext_vector_type(16)));

// every other d: one thread per output element, the chain as written
__global__ __launch_bounds__(256) void k_opq_apply_valu(const float* __restrict__ A, int d, const float* __restrict__ x,
                                                        int64_t n, float* __restrict__ xt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * d) return;
    const int64_t r = e / d;
    const int i = (int)(e - r * d);
    const float* ar = A + (int64_t)i * d;
    const float* xr = x + r * d;
    float acc = 0.f;
    for (int j = 0; j < d; j++) acc = __builtin_fmaf(ar[j], xr[j], acc);
    xt[e] = acc;
}

// d % 4 == 0: a 64 x 64 output tile per workgroup (64 rows of x by 64 rows of A), 32 x 32 per wave, K slabs of 32 staged
// in LDS (row stride 33: the fragment reads of 32 rows at one k hit 32 banks).  Lane l of a wave holds x[i = l & 31][k = l >> 5]
// and A[j = l & 31][k = l >> 5]; an MFMA consumes k and k + 1 in that order, the slabs and the MFMAs of a slab advance in
// ascending k: every accumulator receives its d terms as the chain of the contract.  Rows and columns beyond n / d are
// zero in LDS and never stored.
__global__ __launch_bounds__(256) void k_opq_apply_mfma(const float* __restrict__ A, int d, const float* __restrict__ x,
                                                        int64_t n, float* __restrict__ xt) {
    constexpr int KS = 32, LD = KS + 1;
    __shared__ float sX[64 * LD];
    __shared__ float sA[64 * LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int64_t r_base = (int64_t)blockIdx.x * 64;
    const int c_base = blockIdx.y * 64;
    opq_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    const float* fx = sX + (wr * 32 + (lane & 31)) * LD + (lane >> 5);
    const float* fa = sA + (wc * 32 + (lane & 31)) * LD + (lane >> 5);
    for (int k0 = 0; k0 < d; k0 += KS) {
        const int kw = min(KS, d - k0);   // a multiple of 4
#pragma unroll
        for (int it = 0; it < 8; it++) {   // 64 rows x 32 floats per operand: a wave instruction covers 2 rows (128 B each)
            const int e = it * 256 + tid;
            const int r = e >> 5, c = e & 31;
            const int64_t row = r_base + r;
            const int col = c_base + r;
            sX[r * LD + c] = (row < n && c < kw) ? x[row * d + k0 + c] : 0.f;
            sA[r * LD + c] = (col < d && c < kw) ? A[(int64_t)col * d + k0 + c] : 0.f;
        }
        __syncthreads();
        for (int u = 0; u < kw; u += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fx[u], fa[u], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = c_base + wc * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int64_t row = r_base + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < n && col < d) xt[row * d + col] = acc[r];
    }
}

// ---- training (gamma_hip_opq_train): the pieces of an alternation that touch the whole training set ---------------------------
// columns [c0, c0 + ds) of the rotated set as a contiguous n x ds set (what a sub-quantizer's k-means trains on)
__global__ __launch_bounds__(256) void k_opq_slice(const float* __restrict__ x, int64_t n, int d, int c0, int ds,
                                                   float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * ds) return;
    const int64_t r = e / ds;
    const int t = (int)(e - r * ds);
    out[e] = x[r * d + c0 + t];
}
// decode: the centroid each point was assigned to, back into columns [c0, c0 + ds) of the reconstruction
__global__ __launch_bounds__(256) void k_opq_recons(const float* __restrict__ cen, const int* __restrict__ assign, int k, int64_t n,
                                                    int d, int c0, int ds, float* __restrict__ rec) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * ds) return;
    const int64_t r = e / ds;
    const int t = (int)(e - r * ds);
    const int c = min(max(assign[r], 0), k - 1);
    rec[r * d + c0 + t] = cen[(int64_t)c * ds + t];
}
// P[b][i][j] = sum over the rows r of block b (RB rows, ascending) of y[r][i] * x[r][j], in double: 16 x 16 outputs per
// workgroup, 16 rows at a time through LDS.  Not bit-constrained, but deterministic: one accumulator per (b, i, j), the
// blocks are added in ascending b by k_opq_cross_sum -- no atomics.
constexpr int kCrossRows = 4096;
__global__ __launch_bounds__(256) void k_opq_cross(const float* __restrict__ y, const float* __restrict__ x, int64_t n, int d,
                                                   double* __restrict__ P) {
    __shared__ float sy[16][17];
    __shared__ float sx[16][17];
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const int64_t r0 = (int64_t)blockIdx.z * kCrossRows, r1 = min(n, r0 + kCrossRows);
    double acc = 0.0;
    for (int64_t rb = r0; rb < r1; rb += 16) {
        const int64_t r = rb + ti;   // thread (ti, tj) loads row rb + ti, column tile offset tj
        sy[ti][tj] = (r < r1 && i0 + tj < d) ? y[r * d + i0 + tj] : 0.f;
        sx[ti][tj] = (r < r1 && j0 + tj < d) ? x[r * d + j0 + tj] : 0.f;
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; rr++) acc += (double)sy[rr][ti] * (double)sx[rr][tj];
        __syncthreads();
    }
    if (i0 + ti < d && j0 + tj < d) P[((int64_t)blockIdx.z * d + i0 + ti) * d + j0 + tj] = acc;
}
__global__ __launch_bounds__(256) void k_opq_cross_sum(const double* __restrict__ P, int nb, int d, double* __restrict__ C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)d * d) return;
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += P[(int64_t)b * d * d + e];
    C[e] = s;
}

void launch_opq_slice(hipStream_t s, const float* x, int64_t n, int d, int c0, int ds, float* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_opq_slice, dim3((unsigned)((n * ds + 255) / 256)), dim3(256), 0, s, x, n, d, c0, ds, out);
}
void launch_opq_recons(hipStream_t s, const float* cen, const int* assign, int k, int64_t n, int d, int c0, int ds, float* rec) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_opq_recons, dim3((unsigned)((n * ds + 255) / 256)), dim3(256), 0, s, cen, assign, k, n, d, c0, ds, rec);
}
int opq_cross_blocks(int64_t n) { return (int)((n + kCrossRows - 1) / kCrossRows); }
void launch_opq_cross(hipStream_t s, const float* y, const float* x, int64_t n, int d, double* P, double* C) {
    if (n <= 0) return;
    const int nb = opq_cross_blocks(n);
    if (nb > 65535) return launch_refused("opq_cross: more than 2^28 rows");
    hipLaunchKernelGGL(k_opq_cross, dim3((d + 15) / 16, (d + 15) / 16, nb), dim3(256), 0, s, y, x, n, d, P);
    hipLaunchKernelGGL(k_opq_cross_sum, dim3((unsigned)(((int64_t)d * d + 255) / 256)), dim3(256), 0, s, P, nb, d, C);
}

void launch_opq_apply(hipStream_t s, const float* A, int d, const float* x, int64_t n, float* xt) {
    if (n <= 0 || d <= 0) return;
    if ((d & 3) == 0) {
        const int64_t gx = (n + 63) / 64;
        if (gx > INT32_MAX) return launch_refused("opq_apply: more than 2^37 rows");
        hipLaunchKernelGGL(k_opq_apply_mfma, dim3((unsigned)gx, (unsigned)((d + 63) / 64)), dim3(256), 0, s, A, d, x, n, xt);
    } else {
        const int64_t gx = (n * d + 255) / 256;
        if (gx > INT32_MAX) return launch_refused("opq_apply: more than 2^39 elements");
        hipLaunchKernelGGL(k_opq_apply_valu, dim3((unsigned)gx), dim3(256), 0, s, A, d, x, n, xt);
    }
}

}  // namespace gh
