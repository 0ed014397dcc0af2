// flat_rows_dev.h -- loads of narrow raw rows for the readers of the flat path (kernels.hip, flat_mfma.hip) and of the
// IVFFLAT list-major scan (ivfflat.hip): rows of IEEE binary16
// (uint16_t), uint8 and int8 widen to fp32 EXACTLY, so a reader that widens on load and then runs its fp32 arithmetic unchanged
// computes, bit for bit, what it computes over an fp32 store that holds the widened rows.  Only loads and widenings live here.
// Rows of scalar-quantised codes (sq8_t, rerank_dev.h; gamma_hip_set_flat_sq8_rows) are loaded the way uint8 rows are and then
// DECODED through the store's table, w = vmin[j] + float(code) * step[j] (sq8_dec: a multiply, then an add, each rounded in fp32):
// the fp32 store such a reader matches is the one that holds the decoded rows.  A code's table entry depends on its dimension
// only, so a reader loads the entries of its elements once and decodes every row it holds with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rerank_dev.h"

namespace gh {

template <class Row> struct RowKind;
// byte: the VALUES are bytes (exact in one bf16); sq8: one code per element, a value only after the decode; b8: either -- one
// byte per element in memory, the byte rows' loads
template <> struct RowKind<float> { static constexpr bool fp32 = true, half = false, byte = false, sgn = false, sq8 = false, b8 = false; };
template <> struct RowKind<uint16_t> { static constexpr bool fp32 = false, half = true, byte = false, sgn = false, sq8 = false, b8 = false; };
template <> struct RowKind<uint8_t> { static constexpr bool fp32 = false, half = false, byte = true, sgn = false, sq8 = false, b8 = true; };
template <> struct RowKind<int8_t> { static constexpr bool fp32 = false, half = false, byte = true, sgn = true, sq8 = false, b8 = true; };
template <> struct RowKind<sq8_t> { static constexpr bool fp32 = false, half = false, byte = false, sgn = false, sq8 = true, b8 = true; };

// What a reader needs beside the rows: nothing, or the decode table of sq8 rows, d x {step[j], vmin[j]}.  Empty for the four
// other row types, so a kernel's trailing RowTab<Row> argument adds nothing to their instantiations.
template <class Row> struct RowTab {};
template <> struct RowTab<sq8_t> { const float2* t; };
template <class Row>
inline RowTab<Row> row_tab(const float* tab) {
    if constexpr (RowKind<Row>::sq8) return RowTab<Row>{reinterpret_cast<const float2*>(tab)};
    else return RowTab<Row>{};
}
// the decode: c = float(code), never contracted into an fma (the bits of rerank_dev.h's sq8_row_f)
__device__ __forceinline__ float sq8_dec(float c, float step, float vmin) { return __fadd_rn(vmin, __fmul_rn(c, step)); }

// one element (an sq8 code: as a number, still to be decoded)
template <class Row>
__device__ __forceinline__ float row_elem_f(Row v) {
    if constexpr (RowKind<Row>::fp32) return v;
    else if constexpr (RowKind<Row>::half) return half_bits_f(v);
    else if constexpr (RowKind<Row>::sq8) return (float)v.code;
    else return byte_row_f<RowKind<Row>::sgn>((uint32_t)(uint8_t)v);
}
// a row behind operator[] (fvec_dist takes any indexable): element loads, for rows aligned to their element only
template <class Row>
struct RowElems {
    const Row* p;
    __device__ __forceinline__ float operator[](int i) const { return row_elem_f<Row>(p[i]); }
};
// (sq8: the decoded element; the table entry is wave-uniform -- every thread of k_pairwise_generic is at the same i -- and comes
//  through the scalar cache beside the query's element)
template <>
struct RowElems<sq8_t> {
    const sq8_t* p;
    const float2* t;
    __device__ __forceinline__ float operator[](int i) const {
        const float2 e = t[i];
        return sq8_dec((float)p[i].code, e.x, e.y);
    }
};

// the values of one dword of a narrow row: 2 halves or 4 bytes, in memory order (sq8: the 4 codes as numbers)
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
template <> struct Raw8<sq8_t> { uint2 a; };

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
// sq8 rows: the byte rows' loads; each thread decodes its D / 2 codes with the table entries of ITS elements (they depend on
// `half` only), loaded here once for the row it keeps in registers for the whole launch.
template <class Row, int D>
__device__ __forceinline__ void row_pair_load(const Row* __restrict__ rowp, int half, f32x2* yr, RowTab<Row> tab = RowTab<Row>{}) {
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
    } else if constexpr (RowKind<Row>::b8) {
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
            if constexpr (RowKind<Row>::sq8) {
                // f[0..3]: elements 16 i + 4 half + 0..3, f[4..7]: 8 further on; two table entries per 16-byte load
                const float4* tp = reinterpret_cast<const float4*>(tab.t + 16 * i + 4 * half);
                const float4 t0 = tp[0], t1 = tp[1], t2 = tp[4], t3 = tp[5];
                f[0] = sq8_dec(f[0], t0.x, t0.y); f[1] = sq8_dec(f[1], t0.z, t0.w);
                f[2] = sq8_dec(f[2], t1.x, t1.y); f[3] = sq8_dec(f[3], t1.z, t1.w);
                f[4] = sq8_dec(f[4], t2.x, t2.y); f[5] = sq8_dec(f[5], t2.z, t2.w);
                f[6] = sq8_dec(f[6], t3.x, t3.y); f[7] = sq8_dec(f[7], t3.z, t3.w);
            }
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

// The same pair of threads over sq8 rows with the decode table staged in LDS by the workgroup (the list-major IVFFLAT scan,
// ivfflat.hip: a persistent kernel, one table for every work unit).  Two steps, so that a reader can put its barriers between
// them: row_pair_codes asks for the row's 16-byte loads and keeps each thread's two dwords of every load (D / 8 registers);
// row_pair_decode_lds turns them into the D / 2 decoded values, 16 elements at a time, each step with four 16-byte LDS reads
// of ITS table entries -- never the whole table in registers in front of the first decode, which is what the compiler made
// of row_pair_load's global table loads in k_pairwise_lds<., 128> (178 VGPRs against 110).
// s_tab: the entries of the D elements at rowp, {step, vmin} pairs, as D / 2 float4.  The values are row_pair_load's.
template <int D>
__device__ __forceinline__ void row_pair_codes(const sq8_t* __restrict__ rowp, int half, uint32_t* c0, uint32_t* c1) {
    const uint4* yp = reinterpret_cast<const uint4*>(rowp);
#pragma unroll
    for (int i = 0; i < D / 16; i++) {
        const uint4 v = yp[i];
        const uint32_t vx = v.x, vy = v.y, vz = v.z, vw = v.w;
        c0[i] = half ? vy : vx;
        c1[i] = half ? vw : vz;
    }
}
template <int D>
__device__ __forceinline__ void row_pair_decode_lds(const uint32_t* c0, const uint32_t* c1, int half, f32x2* yr,
                                                    const float4* s_tab) {
#pragma unroll
    for (int i = 0; i < D / 16; i++) {
        float f[8];
        row_dword_f<sq8_t>(c0[i], f);
        row_dword_f<sq8_t>(c1[i], f + 4);
        // f[0..3]: elements 16 i + 4 half + 0..3 (float4 8 i + 2 half of the table), f[4..7]: 8 elements further on
        const float4* tp = s_tab + 8 * i + 2 * half;
        const float4 t0 = tp[0], t1 = tp[1], t2 = tp[4], t3 = tp[5];
        f[0] = sq8_dec(f[0], t0.x, t0.y); f[1] = sq8_dec(f[1], t0.z, t0.w);
        f[2] = sq8_dec(f[2], t1.x, t1.y); f[3] = sq8_dec(f[3], t1.z, t1.w);
        f[4] = sq8_dec(f[4], t2.x, t2.y); f[5] = sq8_dec(f[5], t2.z, t2.w);
        f[6] = sq8_dec(f[6], t3.x, t3.y); f[7] = sq8_dec(f[7], t3.z, t3.w);
        // one step's 16 table registers at a time.  The empty statement makes the step's values exist HERE: left to itself the
        // compiler keeps every step's LDS reads where they are and sinks the arithmetic behind the reader's next barrier, the
        // whole table in registers in between (k_ivfflat_lm<., 128, sq8_t>: 182 VGPRs); the fence keeps the next step's reads
        // behind this one
        asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]));
        __builtin_amdgcn_sched_barrier(0);
        yr[4 * i] = f32x2{f[0], f[1]};
        yr[4 * i + 1] = f32x2{f[2], f[3]};
        yr[4 * i + 2] = f32x2{f[4], f[5]};
        yr[4 * i + 3] = f32x2{f[6], f[7]};
    }
}

// ---- the decode-table entries of 8 consecutive elements (the matrix-pipe filters: a lane's elements of a k step) ----
// Empty and free for the other row types.  j0 % 8 == 0: the 8 entries are 64 aligned bytes.
template <class Row> struct Tab8 {};
template <> struct Tab8<sq8_t> { float4 a, b, c, d; };
// entries j0 .. j0 + 7 of which the first n (<= 0: none) exist; the others are {0, 0}, which decodes a (masked, 0) code to +0
template <class Row>
__device__ __forceinline__ Tab8<Row> tab8_load(RowTab<Row> tab, int j0, int n = 8) {
    Tab8<Row> r;
    if constexpr (RowKind<Row>::sq8) {
        const float2* p = tab.t + j0;
        if (n >= 8) {   // (the common case: four 16-byte loads)
            const float4* p4 = reinterpret_cast<const float4*>(p);
            r.a = p4[0]; r.b = p4[1]; r.c = p4[2]; r.d = p4[3];
        } else {
            const float2 z = make_float2(0.f, 0.f);
            const float2 e0 = n > 0 ? p[0] : z, e1 = n > 1 ? p[1] : z, e2 = n > 2 ? p[2] : z, e3 = n > 3 ? p[3] : z;
            const float2 e4 = n > 4 ? p[4] : z, e5 = n > 5 ? p[5] : z, e6 = n > 6 ? p[6] : z;
            r.a = make_float4(e0.x, e0.y, e1.x, e1.y); r.b = make_float4(e2.x, e2.y, e3.x, e3.y);
            r.c = make_float4(e4.x, e4.y, e5.x, e5.y); r.d = make_float4(e6.x, e6.y, 0.f, 0.f);
        }
    }
    return r;
}
// f[0..7]: 8 widened elements -> for sq8 rows the decoded values; nothing for the other types
template <class Row>
__device__ __forceinline__ void row_decode8(float* f, const Tab8<Row>& t) {
    if constexpr (RowKind<Row>::sq8) {
        f[0] = sq8_dec(f[0], t.a.x, t.a.y); f[1] = sq8_dec(f[1], t.a.z, t.a.w);
        f[2] = sq8_dec(f[2], t.b.x, t.b.y); f[3] = sq8_dec(f[3], t.b.z, t.b.w);
        f[4] = sq8_dec(f[4], t.c.x, t.c.y); f[5] = sq8_dec(f[5], t.c.z, t.c.w);
        f[6] = sq8_dec(f[6], t.d.x, t.d.y); f[7] = sq8_dec(f[7], t.d.z, t.d.w);
    }
}

}  // namespace gh
