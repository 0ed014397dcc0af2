// bf16_split.h -- fp32 -> bf16 hi / lo pairs for the three-product filters (flat_mfma.hip, coarse.hip):
// x = xh + xl + rx with xh = bf16(x), xl = bf16(x - xh), |rx| <= 2^-18 |x|.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gh {

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;

// two floats -> two bf16 (round to nearest even), lo in bits 0..15
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// 8 floats -> (hi, lo) bf16x8: hi = bf16(f), lo = bf16(f - hi)
__device__ __forceinline__ void split_bf16x8(const float* f, uint4& hi, uint4& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        h[i] = cvt_pk_bf16(f[2 * i], f[2 * i + 1]);
        const float h0 = __uint_as_float(h[i] << 16), h1 = __uint_as_float(h[i] & 0xffff0000u);
        l[i] = cvt_pk_bf16(f[2 * i] - h0, f[2 * i + 1] - h1);   // the differences are exact in fp32
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

}  // namespace gh
