// flat_rows_dev.h -- loads of narrow raw rows for the readers of the flat path (kernels.hip, flat_mfma.hip) and of the
// IVFFLAT list-major scan (ivfflat.hip): rows of IEEE binary16
// (uint16_t), uint8 and int8 widen to fp32 EXACTLY, so a reader that widens on load and then runs its fp32 arithmetic unchanged
// computes, bit for bit, what it computes over an fp32 store that holds the widened rows.  Only loads and widenings live here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rerank_dev.h"

namespace gh {

template <class Row> struct RowKind;
template <> struct RowKind<float> { static constexpr bool fp32 = true, half = false, byte = false, sgn = false; };
template <> struct RowKind<uint16_t> { static constexpr bool fp32 = false, half = true, byte = false, sgn = false; };
template <> struct RowKind<uint8_t> { static constexpr bool fp32 = false, half = false, byte = true, sgn = false; };
template <> struct RowKind<int8_t> { static constexpr bool fp32 = false, half = false, byte = true, sgn = true; };

// one element
template <class Row>
__device__ __forceinline__ float row_elem_f(Row v) {
    if constexpr (RowKind<Row>::fp32) return v;
    else if constexpr (RowKind<Row>::half) return half_bits_f(v);
    else return byte_row_f<RowKind<Row>::sgn>((uint32_t)(uint8_t)v);
}
// a row behind operator[] (fvec_dist takes any indexable): element loads, for rows aligned to their element only
template <class Row>
struct RowElems {
    const Row* p;
    __device__ __forceinline__ float operator[](int i) const { return row_elem_f<Row>(p[i]); }
};

// the values of one dword of a narrow row: 2 halves or 4 bytes, in memory order
template <class Row>
__device__ __forceinline__ void row_dword_f(uint32_t w, float* f) {
    static_assert(!RowKind<Row>::fp32, "narrow rows only");
    if constexpr (RowKind<Row>::half) {
        f[0] = half_bits_f(w & 0xffffu);
        f[1] = half_bits_f(w >> 16);
    } else {
        constexpr bool S = RowKind<Row>::sgn;
        if (S) w ^= 0x80808080u;   // value + 128 in every byte, shifted back after the (exact) conversion
        f[0] = (float)(w & 0xffu) - (S ? 128.0f : 0.0f);           // v_cvt_f32_ubyte0 .. 3
        f[1] = (float)((w >> 8) & 0xffu) - (S ? 128.0f : 0.0f);
        f[2] = (float)((w >> 16) & 0xffu) - (S ? 128.0f : 0.0f);
        f[3] = (float)(w >> 24) - (S ? 128.0f : 0.0f);
    }
}

// 8 consecutive elements of a row, as loaded (p aligned to 8 elements of its type: 32 / 16 / 8 bytes) and widened later
template <class Row> struct Raw8;
template <> struct Raw8<float> { float4 a, b; };
template <> struct Raw8<uint16_t> { uint4 a; };
template <> struct Raw8<uint8_t> { uint2 a; };
template <> struct Raw8<int8_t> { uint2 a; };

template <class Row>
__device__ __forceinline__ Raw8<Row> row_load8(const Row* __restrict__ p) {
    Raw8<Row> r;
    if constexpr (RowKind<Row>::fp32) {
        r.a = *reinterpret_cast<const float4*>(p);
        r.b = *reinterpret_cast<const float4*>(p + 4);
    } else if constexpr (RowKind<Row>::half) {
        r.a = *reinterpret_cast<const uint4*>(p);
    } else {
        r.a = *reinterpret_cast<const uint2*>(p);
    }
    return r;
}
template <class Row>
__device__ __forceinline__ void row_widen8(const Raw8<Row>& r, float* f) {
    if constexpr (RowKind<Row>::fp32) {
        f[0] = r.a.x; f[1] = r.a.y; f[2] = r.a.z; f[3] = r.a.w;
        f[4] = r.b.x; f[5] = r.b.y; f[6] = r.b.z; f[7] = r.b.w;
    } else if constexpr (RowKind<Row>::half) {
        row_dword_f<Row>(r.a.x, f);
        row_dword_f<Row>(r.a.y, f + 2);
        row_dword_f<Row>(r.a.z, f + 4);
        row_dword_f<Row>(r.a.w, f + 6);
    } else {
        row_dword_f<Row>(r.a.x, f);
        row_dword_f<Row>(r.a.y, f + 4);
    }
}

// A row held by TWO threads (k_pairwise_lds, k_ivfflat_lm): the even thread owns AVX lanes 0-3 (elements 8i .. 8i + 3), the odd
// one lanes 4-7, D / 2 values each, as D / 4 packed pairs in element order.  rowp: the row's first element, 16-byte aligned
// (D % 16 == 0).  Narrow rows: both threads of a row ask for the SAME 16 bytes (one request) and each keeps its dwords --
// value selects on scalars, never an indexed private array -- widened once.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <class Row, int D>
__device__ __forceinline__ void row_pair_load(const Row* __restrict__ rowp, int half, f32x2* yr) {
    if constexpr (RowKind<Row>::half) {
        // 16 bytes = the 8 halves 8i .. 8i + 7; the even thread's are dwords x, y, the odd thread's z, w
        const uint4* yp = reinterpret_cast<const uint4*>(rowp);
#pragma unroll
        for (int i = 0; i < D / 8; i++) {
            const uint4 v = yp[i];
            const uint32_t vx = v.x, vy = v.y, vz = v.z, vw = v.w;
            float f[4];
            row_dword_f<Row>(half ? vz : vx, f);
            row_dword_f<Row>(half ? vw : vy, f + 2);
            yr[2 * i] = f32x2{f[0], f[1]};
            yr[2 * i + 1] = f32x2{f[2], f[3]};
        }
    } else if constexpr (RowKind<Row>::byte) {
        // 16 bytes = the element groups 2i and 2i + 1 (whole pieces); the even thread's elements are dwords x and z, the odd
        // thread's y and w
        const uint4* yp = reinterpret_cast<const uint4*>(rowp);
#pragma unroll
        for (int i = 0; i < D / 16; i++) {
            const uint4 v = yp[i];
            const uint32_t vx = v.x, vy = v.y, vz = v.z, vw = v.w;
            float f[8];
            row_dword_f<Row>(half ? vy : vx, f);
            row_dword_f<Row>(half ? vw : vz, f + 4);
            yr[4 * i] = f32x2{f[0], f[1]};
            yr[4 * i + 1] = f32x2{f[2], f[3]};
            yr[4 * i + 2] = f32x2{f[4], f[5]};
            yr[4 * i + 3] = f32x2{f[6], f[7]};
        }
    } else {
        const float4* yp = reinterpret_cast<const float4*>(rowp) + half;
#pragma unroll
        for (int i = 0; i < D / 8; i++) {
            const float4 v = yp[2 * i];
            yr[2 * i] = f32x2{v.x, v.y};
            yr[2 * i + 1] = f32x2{v.z, v.w};
        }
    }
}

}  // namespace gh
