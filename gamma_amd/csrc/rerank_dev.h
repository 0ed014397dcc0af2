// rerank_dev.h -- exact fvec_L2sqr / fvec_inner_product of one (query, raw vector) pair by EIGHT
// consecutive threads, which play the eight AVX lane accumulators of the reference's kernels
// (faiss:utils/distances_simd.cpp:366-437; device_math.h fvec_dist is the one-thread form): thread l8
// runs the k-ascending fma chain over elements l8, l8 + 8, ...; then s[l] = acc[l+4] + acc[l], the
// 4-lane and masked tails, (s0+s1)+(s2+s3).  All 8 threads of a group call it together (shuffles);
// the result is valid on thread l8 == 0.  live == false: no loads, result unspecified.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace gh {

template <bool L2>
__device__ __forceinline__ float rerank_dist8(const float* __restrict__ xq, const float* __restrict__ v, int d,
                                              int l, bool live) {
    const int d8 = d & ~7;
    float a = 0.f;
    if (live) {
        // 16 row elements (and 16 query elements) are requested before the dependent fma chain
        // starts: the chain is sequential by construction, the loads need not be
        int i = l;
        for (; i + 15 * 8 < d8; i += 16 * 8) {
            float vv[16], xx[16];
#pragma unroll
            for (int u = 0; u < 16; u++) vv[u] = v[i + 8 * u];
#pragma unroll
            for (int u = 0; u < 16; u++) xx[u] = xq[i + 8 * u];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                if (L2) {
                    const float t = xx[u] - vv[u];
                    a = __builtin_fmaf(t, t, a);
                } else {
                    a = __builtin_fmaf(xx[u], vv[u], a);
                }
            }
        }
        for (; i < d8; i += 8) {
            if (L2) {
                const float t = xq[i] - v[i];
                a = __builtin_fmaf(t, t, a);
            } else {
                a = __builtin_fmaf(xq[i], v[i], a);
            }
        }
    }
    float s = __shfl_down(a, 4, 8) + a;   // s[l] = acc[l+4] + acc[l] for l < 4
    int rem = d - d8, i = d8;
    if (live && rem >= 4) {
        if (l < 4) {
            if (L2) {
                const float t = xq[i + l] - v[i + l];
                s = __builtin_fmaf(t, t, s);
            } else {
                s = __builtin_fmaf(xq[i + l], v[i + l], s);
            }
        }
        i += 4;
        rem -= 4;
    }
    if (live && l < rem) {
        if (L2) {
            const float t = xq[i + l] - v[i + l];
            s = __builtin_fmaf(t, t, s);
        } else {
            s = __builtin_fmaf(xq[i + l], v[i + l], s);
        }
    }
    const float t01 = s + __shfl_down(s, 1, 8);   // lane 0: s0+s1, lane 2: s2+s3
    return t01 + __shfl_down(t01, 2, 8);          // lane 0: (s0+s1)+(s2+s3)
}

// ---- rows of IEEE binary16 (gamma_hip_raw_init_f16) ------------------------------------------------------------------
// The same distance over float(half row): the widening is exact, so the value is fvec_L2sqr / fvec_inner_product of the
// fp32 query and the widened row, operation for operation.
__device__ __forceinline__ float half_bits_f(uint32_t b) { return __half2float(__ushort_as_half((unsigned short)b)); }

// d % 8 == 0 (rows are 16-byte aligned): lane m of the group loads 16 bytes = the 8 consecutive halves 64c + 8m .. + 7 of each
// 64-element chunk c -- one full 128-byte line per candidate and request, where "lane l loads element l + 8u" with 2-byte
// loads would ask for a quarter line per request.  Accumulator lane j needs the elements 64c + 8m + j, m = 0..7, in this order:
// column j of the 8 x 8 matrix whose row m lane m holds.  Three butterfly exchanges transpose it (xor 4: 4-element blocks,
// xor 2: element pairs = dwords, xor 1: the halves of a dword, packed two to a dword), six shuffles per 64 elements.
__device__ __forceinline__ void half_rows_transpose8(const uint4 w, int l, uint32_t e[8]) {
    const bool b4 = l & 4, b2 = l & 2, b1 = l & 1;
    // xor 4: lanes 0-3 keep columns 0-3 of their row and get columns 0-3 of row l + 4; lanes 4-7 the other way round
    const uint32_t r0 = __shfl_xor(b4 ? w.x : w.z, 4, 8), r1 = __shfl_xor(b4 ? w.y : w.w, 4, 8);
    const uint32_t A0 = b4 ? r0 : w.x, A1 = b4 ? r1 : w.y;   // row (l & 3),     column pairs 0, 1 of the lane's column block
    const uint32_t B0 = b4 ? w.z : r0, B1 = b4 ? w.w : r1;   // row (l & 3) + 4
    // xor 2: one column pair of rows r, r + 2, r + 4, r + 6 (r = l & 1)
    const uint32_t rA = __shfl_xor(b2 ? A0 : A1, 2, 8), rB = __shfl_xor(b2 ? B0 : B1, 2, 8);
    const uint32_t P0 = b2 ? rA : A0, P1 = b2 ? A1 : rA, P2 = b2 ? rB : B0, P3 = b2 ? B1 : rB;
    // xor 1: the even lane keeps the low halves (its column) and sends the high ones, the odd lane the other way round
    const uint32_t k0 = b1 ? P0 >> 16 : P0 & 0xffffu, k1 = b1 ? P1 >> 16 : P1 & 0xffffu;
    const uint32_t k2 = b1 ? P2 >> 16 : P2 & 0xffffu, k3 = b1 ? P3 >> 16 : P3 & 0xffffu;
    const uint32_t s0 = b1 ? P0 & 0xffffu : P0 >> 16, s1 = b1 ? P1 & 0xffffu : P1 >> 16;
    const uint32_t s2 = b1 ? P2 & 0xffffu : P2 >> 16, s3 = b1 ? P3 & 0xffffu : P3 >> 16;
    const uint32_t R0 = __shfl_xor(s0 | (s1 << 16), 1, 8), R1 = __shfl_xor(s2 | (s3 << 16), 1, 8);
    const uint32_t g0 = R0 & 0xffffu, g1 = R0 >> 16, g2 = R1 & 0xffffu, g3 = R1 >> 16;   // the partner's rows r' + 2i, r' = 1 - r
    e[0] = b1 ? g0 : k0; e[1] = b1 ? k0 : g0;
    e[2] = b1 ? g1 : k1; e[3] = b1 ? k1 : g1;
    e[4] = b1 ? g2 : k2; e[5] = b1 ? k2 : g2;
    e[6] = b1 ? g3 : k3; e[7] = b1 ? k3 : g3;
}

// Same contract as rerank_dist8 above (all 8 threads of a group call it together, result on thread l == 0).
template <bool L2>
__device__ __forceinline__ float rerank_dist8(const float* __restrict__ xq, const uint16_t* __restrict__ v, int d,
                                              int l, bool live) {
    const int d8 = d & ~7;
    float a = 0.f;
    if ((d & 7) == 0) {   // (uniform) wide loads
        // the row loads of four chunks (256 elements) are requested before the first transpose: the chains are sequential by
        // construction, the loads need not be (d = 128: both of its loads at once, d = 768: three rounds instead of twelve)
        for (int c0 = 0; c0 < d; c0 += 256) {
            uint4 w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                w[u] = make_uint4(0u, 0u, 0u, 0u);
                if (live && c0 + 64 * u + 8 * l < d) w[u] = *reinterpret_cast<const uint4*>(v + c0 + 64 * u + 8 * l);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int cu = c0 + 64 * u;
                if (cu < d) {   // (uniform)
                    float xx[8];
#pragma unroll
                    for (int m = 0; m < 8; m++) xx[m] = (live && cu + 8 * m < d) ? xq[cu + 8 * m + l] : 0.f;
                    uint32_t e[8];
                    half_rows_transpose8(w[u], l, e);
#pragma unroll
                    for (int m = 0; m < 8; m++) {
                        if (cu + 8 * m < d) {   // (uniform) the last chunk of a d that is no multiple of 64 is short
                            const float y = half_bits_f(e[m]);
                            if (L2) {
                                const float t = xx[m] - y;
                                a = __builtin_fmaf(t, t, a);
                            } else {
                                a = __builtin_fmaf(xx[m], y, a);
                            }
                        }
                    }
                }
            }
        }
    } else if (live) {   // rows aligned to 2 bytes only: element loads, lane l takes l, l + 8, ..
        for (int i = l; i < d8; i += 8) {
            const float y = half_bits_f(v[i]);
            if (L2) {
                const float t = xq[i] - y;
                a = __builtin_fmaf(t, t, a);
            } else {
                a = __builtin_fmaf(xq[i], y, a);
            }
        }
    }
    float s = __shfl_down(a, 4, 8) + a;   // s[l] = acc[l+4] + acc[l] for l < 4
    int rem = d - d8, i = d8;
    if (live && rem >= 4) {
        if (l < 4) {
            const float y = half_bits_f(v[i + l]);
            if (L2) {
                const float t = xq[i + l] - y;
                s = __builtin_fmaf(t, t, s);
            } else {
                s = __builtin_fmaf(xq[i + l], y, s);
            }
        }
        i += 4;
        rem -= 4;
    }
    if (live && l < rem) {
        const float y = half_bits_f(v[i + l]);
        if (L2) {
            const float t = xq[i + l] - y;
            s = __builtin_fmaf(t, t, s);
        } else {
            s = __builtin_fmaf(xq[i + l], y, s);
        }
    }
    const float t01 = s + __shfl_down(s, 1, 8);
    return t01 + __shfl_down(t01, 2, 8);
}

// ---- rows of one byte per element (gamma_hip_raw_init_i8) ------------------------------------------------------------
// The same distance over float(byte row): uint8 and int8 widen exactly.  b = the byte as an unsigned value; for int8 the byte
// with its sign bit flipped is value + 128, converted as an unsigned byte and shifted back (both steps exact).
template <bool SIGNED>
__device__ __forceinline__ float byte_row_f(uint32_t b) {
    return SIGNED ? (float)(b ^ 0x80u) - 128.0f : (float)b;
}

// Same contract as rerank_dist8 above.  Lane l's elements l + 8u are byte l & 3 of the row's dwords (l >> 2) + 2u, so no lane
// needs another lane's bytes and nothing is transposed:
//   d % 16 == 0 (rows 16-byte aligned): the eight lanes of a group load the SAME 16 bytes (one request per candidate, half
//                the load instructions of the fp32 rows) and each takes its two elements out of them, selected on scalars as
//                the chunk arrives; a span of 128 elements is eight such loads in front of the chain;
//   d % 4 == 0  (rows 4-byte aligned): one dword load per element;
//   other d:     byte loads.
template <bool L2, bool SIGNED>
__device__ __forceinline__ float rerank_dist8_bytes(const float* __restrict__ xq, const uint8_t* __restrict__ v, int d,
                                                    int l, bool live) {
    const int d8 = d & ~7;
    const int sh = 8 * (l & 3);
    float a = 0.f;
    auto step = [&](float x, float y) {
        if (L2) {
            const float t = x - y;
            a = __builtin_fmaf(t, t, a);
        } else {
            a = __builtin_fmaf(x, y, a);
        }
    };
    if (live) {
        if ((d & 15) == 0) {   // (uniform)
            const bool hi = l & 4;
            const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(v);
            const int nc = d >> 4;   // chunks of 16 elements
            int c = 0;
            for (; c + 8 <= nc; c += 8) {
                // the lane's two dwords of each chunk are picked as the chunk arrives (value selects on scalars: a select
                // between members of an array of uint4 becomes an indexed read of a private array, i.e. scratch)
                uint32_t e0[8], e1[8];
                float xx[16];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = v4[c + u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    e0[u] = hi ? wy : wx;
                    e1[u] = hi ? ww : wz;
                }
#pragma unroll
                for (int u = 0; u < 16; u++) xx[u] = xq[16 * c + 8 * u + l];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    step(xx[2 * u], byte_row_f<SIGNED>((e0[u] >> sh) & 0xffu));
                    step(xx[2 * u + 1], byte_row_f<SIGNED>((e1[u] >> sh) & 0xffu));
                }
            }
            for (; c < nc; c++) {
                const uint4 w = v4[c];
                const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                step(xq[16 * c + l], byte_row_f<SIGNED>(((hi ? wy : wx) >> sh) & 0xffu));
                step(xq[16 * c + 8 + l], byte_row_f<SIGNED>(((hi ? ww : wz) >> sh) & 0xffu));
            }
        } else if ((d & 3) == 0) {   // (uniform)
            const uint32_t* __restrict__ v1 = reinterpret_cast<const uint32_t*>(v);
            for (int i = l; i < d8; i += 8) step(xq[i], byte_row_f<SIGNED>((v1[i >> 2] >> sh) & 0xffu));
        } else {
            for (int i = l; i < d8; i += 8) step(xq[i], byte_row_f<SIGNED>(v[i]));
        }
    }
    float s = __shfl_down(a, 4, 8) + a;   // s[l] = acc[l+4] + acc[l] for l < 4
    int rem = d - d8, i = d8;
    if (live && rem >= 4) {
        if (l < 4) {
            const float y = byte_row_f<SIGNED>(v[i + l]);
            if (L2) {
                const float t = xq[i + l] - y;
                s = __builtin_fmaf(t, t, s);
            } else {
                s = __builtin_fmaf(xq[i + l], y, s);
            }
        }
        i += 4;
        rem -= 4;
    }
    if (live && l < rem) {
        const float y = byte_row_f<SIGNED>(v[i + l]);
        if (L2) {
            const float t = xq[i + l] - y;
            s = __builtin_fmaf(t, t, s);
        } else {
            s = __builtin_fmaf(xq[i + l], y, s);
        }
    }
    const float t01 = s + __shfl_down(s, 1, 8);
    return t01 + __shfl_down(t01, 2, 8);
}
template <bool L2>
__device__ __forceinline__ float rerank_dist8(const float* __restrict__ xq, const uint8_t* __restrict__ v, int d, int l,
                                              bool live) {
    return rerank_dist8_bytes<L2, false>(xq, v, d, l, live);
}
template <bool L2>
__device__ __forceinline__ float rerank_dist8(const float* __restrict__ xq, const int8_t* __restrict__ v, int d, int l,
                                              bool live) {
    return rerank_dist8_bytes<L2, true>(xq, reinterpret_cast<const uint8_t*>(v), d, l, live);
}

// ---- rows of one scalar-quantised byte per element (gamma_hip_raw_init_sq8) ---------------------------------------------
// The same distance over the DECODED row: element j of a row is w = vmin[j] + float(code) * step[j], a multiply and then an
// add, each rounded in fp32 (the __f*_rn intrinsics never contract into an fma), in front of the unchanged fma chain.  The
// decode is not folded into the query: that would change bits.  tab[j] = {step[j], vmin[j]}: one 8-byte load per element beside
// the query's 4-byte load, the same 64 consecutive bytes for the eight lanes of every group (a table of 8 d bytes, resident in
// the caches).  sq8_t is the row type the kernels are instantiated over.
struct sq8_t {
    uint8_t code;
};
__device__ __forceinline__ float sq8_row_f(uint32_t b, const float2 t) { return __fadd_rn(t.y, __fmul_rn((float)b, t.x)); }

// Same contract as rerank_dist8 above; the byte rows' loads (rerank_dist8_bytes): d % 16 == 0 shares 16-byte loads in the group,
// d % 4 == 0 dword loads, other d byte loads.
template <bool L2>
__device__ __forceinline__ float rerank_dist8_sq8(const float* __restrict__ xq, const uint8_t* __restrict__ v,
                                                  const float2* __restrict__ tab, int d, int l, bool live) {
    const int d8 = d & ~7;
    const int sh = 8 * (l & 3);
    float a = 0.f;
    auto step = [&](float x, float y) {
        if (L2) {
            const float t = x - y;
            a = __builtin_fmaf(t, t, a);
        } else {
            a = __builtin_fmaf(x, y, a);
        }
    };
    if (live) {
        if ((d & 15) == 0) {   // (uniform)
            const bool hi = l & 4;
            const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(v);
            const int nc = d >> 4;   // chunks of 16 elements
            int c = 0;
            for (; c + 8 <= nc; c += 8) {
                uint32_t e0[8], e1[8];
                float xx[16];
                float2 tt[16];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = v4[c + u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    e0[u] = hi ? wy : wx;
                    e1[u] = hi ? ww : wz;
                }
#pragma unroll
                for (int u = 0; u < 16; u++) xx[u] = xq[16 * c + 8 * u + l];
#pragma unroll
                for (int u = 0; u < 16; u++) tt[u] = tab[16 * c + 8 * u + l];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    step(xx[2 * u], sq8_row_f((e0[u] >> sh) & 0xffu, tt[2 * u]));
                    step(xx[2 * u + 1], sq8_row_f((e1[u] >> sh) & 0xffu, tt[2 * u + 1]));
                }
            }
            for (; c < nc; c++) {
                const uint4 w = v4[c];
                const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                step(xq[16 * c + l], sq8_row_f(((hi ? wy : wx) >> sh) & 0xffu, tab[16 * c + l]));
                step(xq[16 * c + 8 + l], sq8_row_f(((hi ? ww : wz) >> sh) & 0xffu, tab[16 * c + 8 + l]));
            }
        } else if ((d & 3) == 0) {   // (uniform)
            const uint32_t* __restrict__ v1 = reinterpret_cast<const uint32_t*>(v);
            for (int i = l; i < d8; i += 8) step(xq[i], sq8_row_f((v1[i >> 2] >> sh) & 0xffu, tab[i]));
        } else {
            for (int i = l; i < d8; i += 8) step(xq[i], sq8_row_f(v[i], tab[i]));
        }
    }
    float s = __shfl_down(a, 4, 8) + a;   // s[l] = acc[l+4] + acc[l] for l < 4
    int rem = d - d8, i = d8;
    if (live && rem >= 4) {
        if (l < 4) {
            const float y = sq8_row_f(v[i + l], tab[i + l]);
            if (L2) {
                const float t = xq[i + l] - y;
                s = __builtin_fmaf(t, t, s);
            } else {
                s = __builtin_fmaf(xq[i + l], y, s);
            }
        }
        i += 4;
        rem -= 4;
    }
    if (live && l < rem) {
        const float y = sq8_row_f(v[i + l], tab[i + l]);
        if (L2) {
            const float t = xq[i + l] - y;
            s = __builtin_fmaf(t, t, s);
        } else {
            s = __builtin_fmaf(xq[i + l], y, s);
        }
    }
    const float t01 = s + __shfl_down(s, 1, 8);
    return t01 + __shfl_down(t01, 2, 8);
}

// positions in a row's candidate segment -> vector ids, by the 256 threads of a workgroup (k_map_candidates, rerank.hip; the
// listed launches of the unfiltered selection, select.hip)
__device__ __forceinline__ void map_candidates_row(const int* __restrict__ pos, int R, int P,
                                                   const int* __restrict__ probe_list,
                                                   const int* __restrict__ pair_off,
                                                   const int64_t* __restrict__ list_off,
                                                   const int64_t* __restrict__ ids,
                                                   int64_t* __restrict__ cand_ids, int q) {
    const int* off = pair_off + (int64_t)q * (P + 1);
    for (int r = threadIdx.x; r < R; r += 256) {
        const int ps = pos[(int64_t)q * R + r];
        int64_t id = -1;
        if (ps >= 0) {
            // last p with off[p] <= ps
            int lo = 0, hi = P - 1;
            while (lo < hi) {
                int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= ps) lo = mid; else hi = mid - 1;
            }
            const int l = probe_list[(int64_t)q * P + lo];
            id = ids[list_off[l] + (ps - off[lo])] & 0x7fffffffffffffffLL;
        }
        cand_ids[(int64_t)q * R + r] = id;
    }
}

}  // namespace gh
