// opq.h -- launcher of the OPQ rotation kernels (opq.hip): xt = x A^T for n rows, A d x d row-major
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gh {

// xt[r][i] = sum_j A[i][j] x[r][j]: ONE fp32 accumulator per output element, j ascending from 0, one fmaf per term --
// whichever of the two kernels serves the shape (the matrix pipe for d % 4 == 0, the VALU chain otherwise).  x and xt may not
// overlap.  Enqueued on s, no sync.
void launch_opq_apply(hipStream_t s, const float* A, int d, const float* x, int64_t n, float* xt);

// training (gamma_hip_opq_train): columns [c0, c0 + ds) of x (n x d) as a contiguous n x ds set; the decode of a sub-quantizer's
// assignment into the same columns of rec (n x d); C[i][j] = sum_r y[r][i] x[r][j] in double, deterministic -- P: workspace of
// opq_cross_blocks(n) x d x d doubles, C: d x d doubles
void launch_opq_slice(hipStream_t s, const float* x, int64_t n, int d, int c0, int ds, float* out);
void launch_opq_recons(hipStream_t s, const float* cen, const int* assign, int k, int64_t n, int d, int c0, int ds, float* rec);
int opq_cross_blocks(int64_t n);
void launch_opq_cross(hipStream_t s, const float* y, const float* x, int64_t n, int d, double* P, double* C);

}  // namespace gh
