// ivfflat.hip -- IVFFLAT list scan, list-major (GammaIVFFlatScanner1::scan_codes, index/impl/gamma_index_ivfflat.h:52-75).
//
// k_ivfflat_scan (kernels.hip) takes one (query, probe) pair per workgroup and gathers the list's rows for that one
// query: every row of a list is fetched once per query that probes the list (32 times at 4096 queries, nlist 4096,
// nprobe 32).  Here the work is turned around: one workgroup per LIST keeps 128 of its rows in registers (two
// threads per row, as k_pairwise_lds) and runs every query that probes the list past them, 32 queries per LDS tile.
// The (query, probe) pairs of a list come from an inverse index built per call (count / scan / fill: a counting
// sort of the coarse assignment by list).  Distances are the exact fvec_L2sqr / fvec_inner_product of the
// reference (eight AVX lane accumulators: four per thread of the pair, packed fp32), written to the same slab
// positions as the pair kernel, so everything downstream is unchanged.  d in {16, 32, 64, 96, 128}: k_ivfflat_lm, the whole row
// in registers; every other d % 16 == 0 up to 4096: k_ivfflat_lms below, the row walked in slabs.
// Row: the raw store's element type (float; uint16_t = IEEE binary16, uint8_t, int8_t with gamma_hip_set_ivfflat_narrow_rows).  A
// narrow row is widened -- exactly -- as the pair of threads loads it (row_pair_load, flat_rows_dev.h) and is fp32 from then on.
// sq8_t (gamma_hip_set_ivfflat_sq8_rows): rows of scalar-quantised codes, loaded like uint8 rows and DECODED as they are loaded,
// w = vmin[j] + code * step[j], from the store's table (tab: RowTab<Row>, empty for every other type) staged in LDS: once per
// workgroup in k_ivfflat_lm, per piece beside the query elements in k_ivfflat_lms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_math.h"
#include "filter_dev.h"
#include "flat_rows_dev.h"
#include "kernels.h"

namespace gh {

namespace {
constexpr int FL_QT = 32;   // queries per LDS tile
constexpr int FL_UT = 1;    // tiles per work unit (4: no gain at 16384 queries, -12 % at 4096: fewer, longer units)
constexpr int FL_UQ = FL_QT * FL_UT;
constexpr int FS_QT = 16;      // row-sliced kernel: queries per LDS tile = per work unit (their partial sums stay in registers)
constexpr int FS_SLAB = 128;   // row-sliced kernel: elements of a row a pair of threads holds at a time
}  // namespace

__global__ __launch_bounds__(256) void k_inv_count(const int* __restrict__ probe, int npairs, int nlist,
                                                   const int* __restrict__ list_len, int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int l = probe[i];
    if (l >= 0 && l < nlist && list_len[l] > 0) atomicAdd(&cnt[l], 1);
}
// start[l] = exclusive prefix of cnt; cur[l] = 0; ustart[l] = exclusive prefix of the list's work units
// (query tiles x 128-row chunks), ustart[nlist] = their total.  One block.
template <int UQ>
__device__ __forceinline__ void inv_scan_body(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                              int* __restrict__ start, int* __restrict__ cur, int* __restrict__ ustart) {
    __shared__ int s_w[2][16];
    __shared__ int s_run[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 2) s_run[tid] = 0;
    __syncthreads();
    for (int b = 0; b < nlist; b += 1024) {
        const int i = b + tid;
        const int v = i < nlist ? cnt[i] : 0;
        const int u = (i < nlist && v > 0) ? ((v + UQ - 1) / UQ) * ((list_len[i] + 127) / 128) : 0;
        int incl = v, uincl = u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64), tu = __shfl_up(uincl, o, 64);
            if (lane >= o) {
                incl += t;
                uincl += tu;
            }
        }
        if (lane == 63) {
            s_w[0][w] = incl;
            s_w[1][w] = uincl;
        }
        __syncthreads();
        int basew = s_run[0], baseu = s_run[1];
        for (int k = 0; k < w; k++) {
            basew += s_w[0][k];
            baseu += s_w[1][k];
        }
        if (i < nlist) {
            start[i] = basew + incl - v;
            cur[i] = 0;
            ustart[i] = baseu + uincl - u;
        }
        __syncthreads();
        if (tid == 1023) {
            s_run[0] = basew + incl;
            s_run[1] = baseu + uincl;
        }
        __syncthreads();
    }
    if (tid == 0) ustart[nlist] = s_run[1];
}
__global__ __launch_bounds__(1024) void k_inv_scan(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                                   int* __restrict__ start, int* __restrict__ cur,
                                                   int* __restrict__ ustart) {
    inv_scan_body<FL_UQ>(cnt, list_len, nlist, start, cur, ustart);
}
// the same prefix with the row-sliced kernel's query tile (k_ivfflat_lms below)
__global__ __launch_bounds__(1024) void k_inv_scan_s(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                                     int* __restrict__ start, int* __restrict__ cur,
                                                     int* __restrict__ ustart) {
    inv_scan_body<FS_QT>(cnt, list_len, nlist, start, cur, ustart);
}
__global__ __launch_bounds__(256) void k_inv_fill(const int* __restrict__ probe, int npairs, int nlist,
                                                  const int* __restrict__ list_len, const int* __restrict__ start,
                                                  int* __restrict__ cur, int* __restrict__ inv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int l = probe[i];
    if (l >= 0 && l < nlist && list_len[l] > 0) inv[start[l] + atomicAdd(&cur[l], 1)] = i;
}

// SPARSE: the rows of a sparse store through its vid -> row table (entry_row, filter_dev.h); the dense kernels pass false
template <bool L2, int D, class Row, bool SPARSE>
__device__ __forceinline__ void ivfflat_lm_body(const float* __restrict__ x, int P, const int* __restrict__ pair_off,
                                                const int64_t* __restrict__ list_off,
                                                const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                const Row* __restrict__ raw, int64_t nraw,
                                                const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                const int* __restrict__ inv, const int* __restrict__ ustart,
                                                int nlist, int64_t q_stride,
                                                float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                int need_filter, float min_score, float max_score, RowTab<Row> tab,
                                                const int32_t* __restrict__ slot, int64_t nslot) {
    __shared__ float4 s_x[FL_QT * D / 4];
    __shared__ int s_q[FL_QT];
    __shared__ int s_off[FL_QT];
    const int tid = threadIdx.x, half = tid & 1;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const int nunits = ustart[nlist];
    // sq8 rows: the decode table -- D {step, vmin} pairs, the same for every unit of this persistent kernel -- is staged in
    // LDS once per workgroup; every unit's row decodes from there, 16 elements per step (row_pair_decode_lds)
    const float4* s_tab = nullptr;
    if constexpr (RowKind<Row>::sq8) {
        __shared__ float4 s_t[D / 2];
        for (int e = tid; e < D / 2; e += 256) s_t[e] = reinterpret_cast<const float4*>(tab.t)[e];
        s_tab = s_t;
        __syncthreads();
    }
    // a work unit = (list, 128-row chunk, FL_UT tiles of 32 of the queries probing the list): popular and long lists are cut
    // into many units, so the launch is balanced whatever the data looks like
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        int lo = 0, hi = nlist - 1;
        while (lo < hi) {   // last list with ustart[l] <= u
            const int mid = (lo + hi + 1) >> 1;
            if (ustart[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const int l = lo;
        const int len = list_len[l], n = inv_cnt[l];
        const int chunks = (len + 127) / 128, rel = u - ustart[l];
        const int tq0 = (rel / chunks) * FL_UQ, tq1 = min(n, tq0 + FL_UQ), r0 = (rel - (rel / chunks) * chunks) * 128;
        const int64_t base = list_off[l];
        const int st = inv_start[l];
        {
        const int j = r0 + (tid >> 1);
        const bool inrow = j < len;
        int64_t id = -1;
        if (inrow) id = ids[base + j];
        int64_t rw;
        const bool live = entry_row<SPARSE>(id, inrow, nraw, slot, nslot, need_filter, ftab, &rw);
        f32x2 yr[D / 4];
        if constexpr (RowKind<Row>::sq8) {
            uint32_t c0[D / 16], c1[D / 16];
            row_pair_codes<D>(raw + rw * D, half, c0, c1);
            row_pair_decode_lds<D>(c0, c1, half, yr, s_tab);   // (codes decode here: a multiply, then an add, fp32 from then on)
        } else {
            row_pair_load<Row, D>(raw + rw * D, half, yr);   // (narrow rows widen here, exactly: flat_rows_dev.h)
        }
        for (int t0 = tq0; t0 < tq1; t0 += FL_QT) {
            const int nqt = min(FL_QT, tq1 - t0);
            __syncthreads();   // the previous tile has been consumed
            if (tid < nqt) {
                const int pr = inv[st + t0 + tid];
                const int q = pr / P;
                s_q[tid] = q;
                s_off[tid] = pair_off[(int64_t)q * (P + 1) + (pr - q * P)];
            }
            __syncthreads();
            for (int e = tid; e < nqt * (D / 4); e += 256) {
                const int qi = e / (D / 4), c = e - qi * (D / 4);
                s_x[e] = reinterpret_cast<const float4*>(x + (int64_t)s_q[qi] * D)[c];
            }
            __syncthreads();
            for (int qi = 0; qi < nqt; qi++) {
                const float4* xq = s_x + qi * (D / 4) + half;
                f32x2 acc[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
#pragma unroll
                for (int i0 = 0; i0 < D / 8; i0 += 8) {
                    float4 xa[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) xa[u] = (i0 + u) < D / 8 ? xq[2 * (i0 + u)] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int i = i0 + u;
                        if (i < D / 8) {
                            const f32x2 xv[2] = {f32x2{xa[u].x, xa[u].y}, f32x2{xa[u].z, xa[u].w}};
#pragma unroll
                            for (int k = 0; k < 2; k++) {
                                if (L2) {
                                    const f32x2 t = xv[k] - yr[2 * i + k];
                                    acc[k] = __builtin_elementwise_fma(t, t, acc[k]);
                                } else {
                                    acc[k] = __builtin_elementwise_fma(xv[k], yr[2 * i + k], acc[k]);
                                }
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // even thread: AVX lanes 0..3, odd thread: lanes 4..7;  s[l] = acc[l+4] + acc[l]
                float s0, s1, s2, s3;
                add_xor1_x4(acc[0].x, acc[0].y, acc[1].x, acc[1].y, s0, s1, s2, s3);
                float dis = hsum4(s0, s1, s2, s3);
                if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
                if (inrow && half == 0) out[(int64_t)s_q[qi] * q_stride + s_off[qi] + j] = dis;
            }
        }
        }
    }
}
template <bool L2, int D, class Row = float>
__global__ __launch_bounds__(256) void k_ivfflat_lm(const float* __restrict__ x, int P, const int* __restrict__ pair_off,
                                                    const int64_t* __restrict__ list_off,
                                                    const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                    const Row* __restrict__ raw, int64_t nraw,
                                                    const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                    const int* __restrict__ inv, const int* __restrict__ ustart,
                                                    int nlist, int64_t q_stride,
                                                    float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                    int need_filter, float min_score, float max_score, RowTab<Row> tab) {
    ivfflat_lm_body<L2, D, Row, false>(x, P, pair_off, list_off, list_len, ids, raw, nraw, inv_start, inv_cnt, inv, ustart, nlist,
                                       q_stride, out, ftab, need_filter, min_score, max_score, tab, nullptr, 0);
}
// the rows of a sparse store (the list shards of a group whose rows live with their lists): float, or float16 / uint8 / int8
// widened as they are loaded; never sq8
template <bool L2, int D, class Row = float>
__global__ __launch_bounds__(256) void k_ivfflat_lm_sp(const float* __restrict__ x, int P, const int* __restrict__ pair_off,
                                                       const int64_t* __restrict__ list_off,
                                                       const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                       const Row* __restrict__ raw, int64_t nraw,
                                                       const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                       const int* __restrict__ inv, const int* __restrict__ ustart,
                                                       int nlist, int64_t q_stride,
                                                       float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                       int need_filter, float min_score, float max_score,
                                                       const int32_t* __restrict__ slot, int64_t nslot) {
    ivfflat_lm_body<L2, D, Row, true>(x, P, pair_off, list_off, list_len, ids, raw, nraw, inv_start, inv_cnt, inv, ustart, nlist,
                                      q_stride, out, ftab, need_filter, min_score, max_score, RowTab<Row>{}, slot, nslot);
}

// ---- rows of any d % 16 == 0 up to 4096: the row-sliced list-major kernel ------------------------------------------------
// A row of d floats does not fit in the registers of two threads (768 floats: 384 each), so the pair of threads walks it in
// slabs of FS_SLAB = 128 elements -- 64 registers each, the load of k_ivfflat_lm<.., 128> -- and the last d % 128 elements in
// pieces of 64 / 32 / 16 (every type keeps its 16-byte loads: d % 16 == 0).  What crosses a slab is the partial sums: the
// eight AVX lane accumulators of every query of the tile, four per thread as two packed pairs, FS_QT x 2 f32x2 = 64 registers
// at FS_QT = 16.  So a work unit is (list, 128-row chunk, ONE tile of 16 of the queries probing the list) and a row is read
// once per tile, ceil(n / 16) times for n probing queries (k_ivfflat_lm: once; the pair kernel: n times).  Per slab the
// tile's query elements are staged in LDS (16 x 128 floats, 8 KB) and every query's fma chain runs on from where the slab
// before left it: each lane accumulator is ONE chain over its elements in ascending order, exactly fvec_L2sqr /
// fvec_inner_product's, and the epilogue is k_ivfflat_lm's.  The slab loop is a run-time loop over d; the query loop is
// unrolled so that the accumulators are registers (a branch per query on the wave-uniform tile length).
template <bool L2, class Row, int LEN>
__device__ __forceinline__ void lms_piece(const Row* __restrict__ rowp, const float* __restrict__ x, int d, int e0, int half,
                                          int tid, int nqt, const int* s_q, float4* s_x, f32x2 (&acc)[FS_QT][2],
                                          RowTab<Row> tab, float4* s_tab) {
    f32x2 yr[LEN / 4];
    constexpr bool SQ8 = RowKind<Row>::sq8;
    // sq8 rows: the codes are in flight while the tile's queries AND the piece's table entries (elements e0 .. e0 + LEN - 1,
    // LEN / 2 float4) are staged under the same two barriers; the decode reads the entries from LDS behind the second one
    uint32_t c0[SQ8 ? LEN / 16 : 1], c1[SQ8 ? LEN / 16 : 1];
    if constexpr (SQ8) row_pair_codes<LEN>(rowp + e0, half, c0, c1);
    else row_pair_load<Row, LEN>(rowp + e0, half, yr);   // in flight while the tile's queries are staged
    __syncthreads();   // the previous piece has been consumed (first piece: s_q is written)
    for (int e = tid; e < nqt * (LEN / 4); e += 256) {
        const int qi = e / (LEN / 4), c = e - qi * (LEN / 4);
        s_x[e] = reinterpret_cast<const float4*>(x + (int64_t)s_q[qi] * d + e0)[c];
    }
    if constexpr (SQ8) {
        for (int e = tid; e < LEN / 2; e += 256) s_tab[e] = reinterpret_cast<const float4*>(tab.t + e0)[e];
    }
    __syncthreads();
    if constexpr (SQ8) row_pair_decode_lds<LEN>(c0, c1, half, yr, s_tab);
#pragma unroll
    for (int qi = 0; qi < FS_QT; qi++) {
        if (qi < nqt) {
            const float4* xq = s_x + qi * (LEN / 4) + half;
#pragma unroll
            for (int i0 = 0; i0 < LEN / 8; i0 += 8) {
                float4 xa[8];
#pragma unroll
                for (int u = 0; u < 8; u++) xa[u] = (i0 + u) < LEN / 8 ? xq[2 * (i0 + u)] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int i = i0 + u;
                    if (i < LEN / 8) {
                        const f32x2 xv[2] = {f32x2{xa[u].x, xa[u].y}, f32x2{xa[u].z, xa[u].w}};
#pragma unroll
                        for (int k = 0; k < 2; k++) {
                            if (L2) {
                                const f32x2 t = xv[k] - yr[2 * i + k];
                                acc[qi][k] = __builtin_elementwise_fma(t, t, acc[qi][k]);
                            } else {
                                acc[qi][k] = __builtin_elementwise_fma(xv[k], yr[2 * i + k], acc[qi][k]);
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

template <bool L2, class Row, bool SPARSE>
__device__ __forceinline__ void ivfflat_lms_body(const float* __restrict__ x, int d, int P, const int* __restrict__ pair_off,
                                                 const int64_t* __restrict__ list_off,
                                                 const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                 const Row* __restrict__ raw, int64_t nraw,
                                                 const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                 const int* __restrict__ inv, const int* __restrict__ ustart,
                                                 int nlist, int64_t q_stride,
                                                 float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                 int need_filter, float min_score, float max_score, RowTab<Row> tab,
                                                 const int32_t* __restrict__ slot, int64_t nslot) {
    __shared__ float4 s_x[FS_QT * FS_SLAB / 4];
    __shared__ int s_q[FS_QT];
    __shared__ int s_off[FS_QT];
    float4* s_tab = nullptr;   // sq8 rows: the table entries of the piece at hand (lms_piece), 1 KB
    if constexpr (RowKind<Row>::sq8) {
        __shared__ float4 s_t[FS_SLAB / 2];
        s_tab = s_t;
    }
    const int tid = threadIdx.x, half = tid & 1;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const int nunits = ustart[nlist];
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        int lo = 0, hi = nlist - 1;
        while (lo < hi) {   // last list with ustart[l] <= u
            const int mid = (lo + hi + 1) >> 1;
            if (ustart[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const int l = lo;
        const int len = list_len[l], n = inv_cnt[l];
        const int chunks = (len + 127) / 128, rel = u - ustart[l];
        const int tq0 = (rel / chunks) * FS_QT, nqt = min(FS_QT, n - tq0), r0 = (rel - (rel / chunks) * chunks) * 128;
        const int64_t base = list_off[l];
        const int j = r0 + (tid >> 1);
        const bool inrow = j < len;
        int64_t id = -1;
        if (inrow) id = ids[base + j];
        int64_t rw;
        const bool live = entry_row<SPARSE>(id, inrow, nraw, slot, nslot, need_filter, ftab, &rw);
        const Row* rowp = raw + rw * d;
        __syncthreads();   // the previous unit has stored its distances: s_q, s_off are free
        if (tid < nqt) {
            const int pr = inv[inv_start[l] + tq0 + tid];
            const int q = pr / P;
            s_q[tid] = q;
            s_off[tid] = pair_off[(int64_t)q * (P + 1) + (pr - q * P)];
        }
        f32x2 acc[FS_QT][2];
#pragma unroll
        for (int qi = 0; qi < FS_QT; qi++) acc[qi][0] = acc[qi][1] = f32x2{0.f, 0.f};
        int e0 = 0;
        for (; e0 + FS_SLAB <= d; e0 += FS_SLAB) lms_piece<L2, Row, FS_SLAB>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc, tab, s_tab);
        if (d - e0 >= 64) {
            lms_piece<L2, Row, 64>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc, tab, s_tab);
            e0 += 64;
        }
        if (d - e0 >= 32) {
            lms_piece<L2, Row, 32>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc, tab, s_tab);
            e0 += 32;
        }
        if (d - e0 >= 16) lms_piece<L2, Row, 16>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc, tab, s_tab);
#pragma unroll
        for (int qi = 0; qi < FS_QT; qi++) {
            if (qi < nqt) {
                // even thread: AVX lanes 0..3, odd thread: lanes 4..7;  s[l] = acc[l+4] + acc[l]
                float s0, s1, s2, s3;
                add_xor1_x4(acc[qi][0].x, acc[qi][0].y, acc[qi][1].x, acc[qi][1].y, s0, s1, s2, s3);
                float dis = hsum4(s0, s1, s2, s3);
                if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
                if (inrow && half == 0) out[(int64_t)s_q[qi] * q_stride + s_off[qi] + j] = dis;
            }
        }
    }
}
template <bool L2, class Row>
__global__ __launch_bounds__(256) void k_ivfflat_lms(const float* __restrict__ x, int d, int P, const int* __restrict__ pair_off,
                                                     const int64_t* __restrict__ list_off,
                                                     const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                     const Row* __restrict__ raw, int64_t nraw,
                                                     const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                     const int* __restrict__ inv, const int* __restrict__ ustart,
                                                     int nlist, int64_t q_stride,
                                                     float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                     int need_filter, float min_score, float max_score, RowTab<Row> tab) {
    ivfflat_lms_body<L2, Row, false>(x, d, P, pair_off, list_off, list_len, ids, raw, nraw, inv_start, inv_cnt, inv, ustart, nlist,
                                     q_stride, out, ftab, need_filter, min_score, max_score, tab, nullptr, 0);
}
template <bool L2, class Row = float>
__global__ __launch_bounds__(256) void k_ivfflat_lms_sp(const float* __restrict__ x, int d, int P, const int* __restrict__ pair_off,
                                                        const int64_t* __restrict__ list_off,
                                                        const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                                                        const Row* __restrict__ raw, int64_t nraw,
                                                        const int* __restrict__ inv_start, const int* __restrict__ inv_cnt,
                                                        const int* __restrict__ inv, const int* __restrict__ ustart,
                                                        int nlist, int64_t q_stride,
                                                        float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                        int need_filter, float min_score, float max_score,
                                                        const int32_t* __restrict__ slot, int64_t nslot) {
    ivfflat_lms_body<L2, Row, true>(x, d, P, pair_off, list_off, list_len, ids, raw, nraw, inv_start, inv_cnt, inv, ustart, nlist,
                                    q_stride, out, ftab, need_filter, min_score, max_score, RowTab<Row>{}, slot, nslot);
}

// list_len with the lists a shard's mask does not own set to 0: to the list-major launch an unowned list is an empty list
__global__ __launch_bounds__(256) void k_masked_list_len(const int* __restrict__ list_len, const uint8_t* __restrict__ mask,
                                                         int nlist, int* __restrict__ out) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < nlist) out[l] = (!mask || mask[l]) ? list_len[l] : 0;
}
void launch_masked_list_len(hipStream_t s, const int* list_len, const uint8_t* mask, int nlist, int* out) {
    if (nlist > 0) hipLaunchKernelGGL(k_masked_list_len, dim3((nlist + 255) / 256), dim3(256), 0, s, list_len, mask, nlist, out);
}

bool ivfflat_lm_supported(int d) { return d == 16 || d == 32 || d == 64 || d == 96 || d == 128; }

int ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile) {
    const int k = ivfflat_lm_supported(d) ? 1 : (d >= 16 && d <= 4096 && d % 16 == 0) ? 2 : 0;
    *kind = k;
    *slab = k == 1 ? d : k == 2 ? FS_SLAB : 0;
    *qtile = k == 1 ? FL_QT : k == 2 ? FS_QT : 0;
    return k;
}

// scratch: inv [nq * P] ints, then cnt | start | cur [nlist] ints each
size_t ivfflat_lm_scratch_bytes(int nq, int P, int nlist) { return ((size_t)nq * P + 4 * (size_t)nlist + 1) * sizeof(int); }

namespace {
template <class Row>
void launch_ivfflat_lm_t(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                         const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const Row* raw,
                         int64_t nraw, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter, float min_score,
                         float max_score, void* scratch, RowTab<Row> tab = RowTab<Row>{}, const int32_t* slot = nullptr,
                         int64_t nslot = 0) {
    if (nq <= 0 || P <= 0) return;
    int* inv = static_cast<int*>(scratch);
    int* cnt = inv + (size_t)nq * P;
    int* start = cnt + nlist;
    int* cur = start + nlist;
    int* ustart = cur + nlist;
    const int npairs = nq * P;
    (void)hipMemsetAsync(cnt, 0, (size_t)nlist * sizeof(int), s);
    hipLaunchKernelGGL(k_inv_count, dim3((npairs + 255) / 256), dim3(256), 0, s, probe, npairs, nlist, list_len, cnt);
    const bool sliced = !ivfflat_lm_supported(d);   // (the caller asked ivfflat_lm_shape: d % 16 == 0, d <= 4096)
    if (sliced) hipLaunchKernelGGL(k_inv_scan_s, dim3(1), dim3(1024), 0, s, cnt, list_len, nlist, start, cur, ustart);
    else hipLaunchKernelGGL(k_inv_scan, dim3(1), dim3(1024), 0, s, cnt, list_len, nlist, start, cur, ustart);
    hipLaunchKernelGGL(k_inv_fill, dim3((npairs + 255) / 256), dim3(256), 0, s, probe, npairs, nlist, list_len, start, cur, inv);
    const int grid = 256 * 8;   // persistent: every workgroup walks the unit list with stride gridDim.x
    if constexpr (!RowKind<Row>::sq8) {
        if (slot) {   // a sparse store: the same two kernels with the vid -> row table (launch_ivfflat_lm_sparse)
#define GH_FLSP(LL, DD)                                                                                                       \
    hipLaunchKernelGGL((k_ivfflat_lm_sp<LL, DD, Row>), dim3(grid), dim3(256), 0, s, x, P, pair_off, list_off, list_len, ids, raw, nraw, \
                       start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score, max_score, slot, nslot)
#define GH_FLSPD(LL)                      \
    switch (d) {                          \
        case 128: GH_FLSP(LL, 128); break; \
        case 96: GH_FLSP(LL, 96); break;   \
        case 64: GH_FLSP(LL, 64); break;   \
        case 32: GH_FLSP(LL, 32); break;   \
        default: GH_FLSP(LL, 16); break;   \
    }
            if (sliced) {
                if (l2)
                    hipLaunchKernelGGL((k_ivfflat_lms_sp<true, Row>), dim3(grid), dim3(256), 0, s, x, d, P, pair_off, list_off, list_len,
                                       ids, raw, nraw, start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score,
                                       max_score, slot, nslot);
                else
                    hipLaunchKernelGGL((k_ivfflat_lms_sp<false, Row>), dim3(grid), dim3(256), 0, s, x, d, P, pair_off, list_off, list_len,
                                       ids, raw, nraw, start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score,
                                       max_score, slot, nslot);
            } else if (l2) {
                GH_FLSPD(true)
            } else {
                GH_FLSPD(false)
            }
#undef GH_FLSPD
#undef GH_FLSP
            return;
        }
    }
    if (sliced) {
        if (l2)
            hipLaunchKernelGGL((k_ivfflat_lms<true, Row>), dim3(grid), dim3(256), 0, s, x, d, P, pair_off, list_off, list_len, ids,
                               raw, nraw, start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score, max_score, tab);
        else
            hipLaunchKernelGGL((k_ivfflat_lms<false, Row>), dim3(grid), dim3(256), 0, s, x, d, P, pair_off, list_off, list_len, ids,
                               raw, nraw, start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score, max_score, tab);
        return;
    }
#define GH_FL(LL, DD)                                                                                                   \
    hipLaunchKernelGGL((k_ivfflat_lm<LL, DD, Row>), dim3(grid), dim3(256), 0, s, x, P, pair_off, list_off, list_len, ids, \
                       raw, nraw, start, cnt, inv, ustart, nlist, q_stride, out, ftab, need_filter, min_score, max_score, tab)
#define GH_FLD(LL)                    \
    switch (d) {                      \
        case 128: GH_FL(LL, 128); break; \
        case 96: GH_FL(LL, 96); break;   \
        case 64: GH_FL(LL, 64); break;   \
        case 32: GH_FL(LL, 32); break;   \
        default: GH_FL(LL, 16); break;   \
    }
    if (l2) { GH_FLD(true) } else { GH_FLD(false) }
#undef GH_FLD
#undef GH_FL
}
}  // namespace

void launch_ivfflat_lm(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                       const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const float* raw,
                       int64_t nraw, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter, float min_score,
                       float max_score, void* scratch) {
    launch_ivfflat_lm_t<float>(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw, nraw, q_stride, out, ftab,
                               need_filter, min_score, max_score, scratch);
}
// fp32 rows of a sparse store: slot [nslot] = vector id -> row of `raw` (nraw rows), -1 = not held here
void launch_ivfflat_lm_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                              const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const float* raw,
                              int64_t nraw, const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                              int need_filter, float min_score, float max_score, void* scratch) {
    if (!slot) return;   // (a sparse store without a table holds no row: the caller fills the slab with the sentinel)
    launch_ivfflat_lm_t<float>(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw, nraw, q_stride, out, ftab,
                               need_filter, min_score, max_score, scratch, RowTab<float>{}, slot, nslot);
}
// ... of any element type but sq8 (a sparse sq8 store is refused before it gets here: nothing is launched for one)
void launch_ivfflat_lm_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                              const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const RowsRef& raw,
                              int64_t nraw, const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                              int need_filter, float min_score, float max_score, void* scratch) {
    if (!slot) return;
#define GH_FLRS(T)                                                                                                             \
    launch_ivfflat_lm_t<T>(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw.as<T>(), nraw, q_stride, out, \
                           ftab, need_filter, min_score, max_score, scratch, RowTab<T>{}, slot, nslot)
    switch (raw.et) {
        case 0: GH_FLRS(float); break;
        case 1: GH_FLRS(uint16_t); break;
        case 2: GH_FLRS(uint8_t); break;
        case 3: GH_FLRS(int8_t); break;
        default: break;
    }
#undef GH_FLRS
}
// rows of any element type (gamma_hip_set_ivfflat_narrow_rows, _sq8_rows); fp32 rows: the launch above, the kernels it always ran
void launch_ivfflat_lm(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                       const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const RowsRef& raw,
                       int64_t nraw, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter, float min_score,
                       float max_score, void* scratch) {
#define GH_FLR(T)                                                                                                              \
    launch_ivfflat_lm_t<T>(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw.as<T>(), nraw, q_stride, out, \
                           ftab, need_filter, min_score, max_score, scratch)
    switch (raw.et) {
        case 0:
            launch_ivfflat_lm(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw.as<float>(), nraw, q_stride,
                              out, ftab, need_filter, min_score, max_score, scratch);
            break;
        case 1: GH_FLR(uint16_t); break;
        case 2: GH_FLR(uint8_t); break;
        case 3: GH_FLR(int8_t); break;
        case 4:   // (codes are never numbers: an sq8 store goes to the decoding kernels or nowhere)
            launch_ivfflat_lm_t<sq8_t>(s, l2, x, nq, d, P, probe, pair_off, list_off, list_len, nlist, ids, raw.as<sq8_t>(), nraw,
                                       q_stride, out, ftab, need_filter, min_score, max_score, scratch, row_tab<sq8_t>(raw.tab));
            break;
        default: break;
    }
#undef GH_FLR
}

}  // namespace gh
