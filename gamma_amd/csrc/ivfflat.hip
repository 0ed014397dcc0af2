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

#include "binivf.h"
#include "device_math.h"
#include "filter_dev.h"
#include "flat_rows_dev.h"
#include "ivfflat_plan.h"   // FL_QT, FS_QT, FS_SLAB
#include "kernels.h"
#include "pq4.h"   // kPq4LmQueryTile, kPq4LmSlab

namespace gh {

namespace {
constexpr int FL_UT = 1;    // tiles per work unit (4: no gain at 16384 queries, -12 % at 4096: fewer, longer units)
constexpr int FL_UQ = FL_QT * FL_UT;
}  // namespace

__global__ __launch_bounds__(256) void k_inv_count(const int* __restrict__ probe, int npairs, int nlist,
                                                   const int* __restrict__ list_len, int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int l = probe[i];
    if (l >= 0 && l < nlist && list_len[l] > 0) atomicAdd(&cnt[l], 1);
}
// start[l] = exclusive prefix of cnt; cur[l] = 0; ustart[l] = exclusive prefix of the list's work units
// (query tiles x ROWS-row chunks), ustart[nlist] = their total.  One block.
template <int UQ, int ROWS = 128>
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
        const int u = (i < nlist && v > 0) ? ((v + UQ - 1) / UQ) * ((list_len[i] + ROWS - 1) / ROWS) : 0;
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
// the same prefix with the binary list-major scan's unit: kBinLmQueryTile queries x kBinSpreadChunk rows (binivf_lm.hip)
__global__ __launch_bounds__(1024) void k_inv_scan_b(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                                     int* __restrict__ start, int* __restrict__ cur,
                                                     int* __restrict__ ustart) {
    inv_scan_body<kBinLmQueryTile, kBinSpreadChunk>(cnt, list_len, nlist, start, cur, ustart);
}
// the same prefix with the 4-bit list-major scan's unit: kPq4LmQueryTile pairs x kPq4LmSlab codes (pq4.hip)
__global__ __launch_bounds__(1024) void k_inv_scan_p(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                                     int* __restrict__ start, int* __restrict__ cur,
                                                     int* __restrict__ ustart) {
    inv_scan_body<kPq4LmQueryTile, kPq4LmSlab>(cnt, list_len, nlist, start, cur, ustart);
}
// the same prefix with the wide list-major scan's unit: kWideLmQueryTile pairs x kWideLmSlab codes (pqwide_lm.hip)
__global__ __launch_bounds__(1024) void k_inv_scan_w(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist,
                                                     int* __restrict__ start, int* __restrict__ cur,
                                                     int* __restrict__ ustart) {
    inv_scan_body<kWideLmQueryTile, kWideLmSlab>(cnt, list_len, nlist, start, cur, ustart);
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

// ---- rows of every other length up to 4096 (d % 16 != 0): the row-sliced kernel with the scanner's tail steps -------------
// fvec_L2sqr / fvec_inner_product end, behind the 8-wide loop, in a 4-lane step and a masked step that run AFTER the eight
// accumulators are folded to four (rerank_dist8, rerank_dev.h: the arithmetic restated here operation for operation).  With
// d16 = d & ~15 and r = d - d16 (1..15): elements 0 .. d16 - 1 run in k_ivfflat_lms's pieces; r >= 8: one more 8-wide step into
// the same chains (4 elements per thread); the fold; d & 4: s[l] = fma(.., s[l]) over the next four elements; l < (d & 3): the
// masked step; hsum4.  The work split, the inverse index and the slab positions are k_ivfflat_lms's.
// What differs beside the tail: a row of such a d is aligned to LOADB = gcd(16, d * sizeof(Row)) bytes only, a query row to
// gcd(16, 4 d), so both are read with loads of that width (chosen on the host, a template argument here), and nothing is read
// at or beyond rowp + d: the tail's (at most 11) row values per thread come from whole groups of four inside the row and from
// predicated element loads.  The tail's query elements are staged once per unit, 16 queries x 16 floats, absent ones zero.
// The kernels carry the no-packed-fp32-ops target attribute: their subtractions and fmas are single-lane instructions.
namespace {
// 4 consecutive elements at p, widened; p is aligned to LOADB bytes or to the four elements, whichever is less
template <class Row, int LOADB>
__device__ __forceinline__ void lmt_load4(const Row* __restrict__ p, float* f) {
    constexpr int B4 = 4 * (int)sizeof(Row), LB = LOADB < B4 ? LOADB : B4;
    if constexpr (RowKind<Row>::fp32) {
        if constexpr (LB == 16) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else if constexpr (LB == 8) {
            const float2 a = reinterpret_cast<const float2*>(p)[0], b = reinterpret_cast<const float2*>(p)[1];
            f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
        } else {
            f[0] = p[0]; f[1] = p[1]; f[2] = p[2]; f[3] = p[3];
        }
    } else if constexpr (RowKind<Row>::half) {
        uint32_t w0, w1;
        if constexpr (LB == 8) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            w0 = v.x; w1 = v.y;
        } else if constexpr (LB == 4) {
            w0 = reinterpret_cast<const uint32_t*>(p)[0]; w1 = reinterpret_cast<const uint32_t*>(p)[1];
        } else {
            w0 = (uint32_t)p[0] | ((uint32_t)p[1] << 16); w1 = (uint32_t)p[2] | ((uint32_t)p[3] << 16);
        }
        row_dword_f<Row>(w0, f);
        row_dword_f<Row>(w1, f + 2);
    } else {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
        uint32_t w;
        if constexpr (LB == 4) {
            w = *reinterpret_cast<const uint32_t*>(b);
        } else if constexpr (LB == 2) {
            w = (uint32_t)reinterpret_cast<const uint16_t*>(b)[0] | ((uint32_t)reinterpret_cast<const uint16_t*>(b)[1] << 16);
        } else {
            w = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        row_dword_f<Row>(w, f);
    }
}
// LEN elements at p (a multiple of 16 elements into the row) for the pair of threads: the registers row_pair_load fills.
// 16-byte rows: row_pair_load itself; byte rows aligned to 8: both threads ask for the same 8 bytes = one element group and each
// keeps its dword; every other class: each thread's own four elements of a group, in loads of LOADB bytes
template <class Row, int LEN, int LOADB>
__device__ __forceinline__ void lmt_row_load(const Row* __restrict__ p, int half, f32x2* yr) {
    if constexpr (LOADB == 16) {
        row_pair_load<Row, LEN>(p, half, yr);
    } else {
#pragma unroll
        for (int i = 0; i < LEN / 8; i++) {
            float f[4];
            if constexpr (RowKind<Row>::b8 && LOADB == 8) {
                const uint2 v = reinterpret_cast<const uint2*>(p)[i];
                const uint32_t vx = v.x, vy = v.y;
                row_dword_f<Row>(half ? vy : vx, f);
            } else {
                lmt_load4<Row, LOADB>(p + 8 * i + 4 * half, f);
            }
            yr[2 * i] = f32x2{f[0], f[1]};
            yr[2 * i + 1] = f32x2{f[2], f[3]};
        }
    }
}
template <bool L2>
__device__ __forceinline__ float lmt_step(float x, float y, float a) {
    if (L2) {
        const float t = x - y;
        return __builtin_fmaf(t, t, a);
    }
    return __builtin_fmaf(x, y, a);
}

// lms_piece with the row loads above and the query elements staged QE = min(4, LOADB / sizeof(Row)) at a time (a query row is
// aligned to QE floats); what lands in LDS, and the fma loop behind it, are lms_piece's
template <bool L2, class Row, int LEN, int LOADB>
__device__ __forceinline__ void lmt_piece(const Row* __restrict__ rowp, const float* __restrict__ x, int d, int e0, int half,
                                          int tid, int nqt, const int* s_q, float4* s_x, f32x2 (&acc)[FS_QT][2]) {
    constexpr int EL = LOADB / (int)sizeof(Row), QE = EL < 4 ? EL : 4;
    f32x2 yr[LEN / 4];
    lmt_row_load<Row, LEN, LOADB>(rowp + e0, half, yr);   // in flight while the tile's queries are staged
    __syncthreads();   // the previous piece has been consumed
    for (int e = tid; e < nqt * (LEN / QE); e += 256) {
        const int qi = e / (LEN / QE), c = e - qi * (LEN / QE);
        const float* src = x + (int64_t)s_q[qi] * d + e0 + c * QE;
        if constexpr (QE == 4) s_x[e] = *reinterpret_cast<const float4*>(src);
        else if constexpr (QE == 2) reinterpret_cast<float2*>(s_x)[e] = *reinterpret_cast<const float2*>(src);
        else reinterpret_cast<float*>(s_x)[e] = *src;
    }
    __syncthreads();
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
}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#define GH_SINGLE_LANE_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define GH_SINGLE_LANE_F32   // (the host pass does not know the feature)
#endif
template <bool L2, class Row, int LOADB>
__global__ __launch_bounds__(256) GH_SINGLE_LANE_F32
void k_ivfflat_lmt(const float* __restrict__ x, int d, int P, const int* __restrict__ pair_off,
                   const int64_t* __restrict__ list_off, const int* __restrict__ list_len, const int64_t* __restrict__ ids,
                   const Row* __restrict__ raw, int64_t nraw, const int* __restrict__ inv_start,
                   const int* __restrict__ inv_cnt, const int* __restrict__ inv, const int* __restrict__ ustart, int nlist,
                   int64_t q_stride, float* __restrict__ out, const FilterDesc* __restrict__ ftab, int need_filter,
                   float min_score, float max_score) {
    static_assert(LOADB >= (int)sizeof(Row) && LOADB <= 16 && (LOADB & (LOADB - 1)) == 0, "a power of two, a whole element");
    __shared__ float4 s_x[FS_QT * FS_SLAB / 4];
    __shared__ float4 s_xt[FS_QT * 4];   // the tail's query elements d16 .. d16 + 15 of every query of the tile, absent ones 0
    __shared__ int s_q[FS_QT];
    __shared__ int s_off[FS_QT];
    const int tid = threadIdx.x, half = tid & 1;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const int nunits = ustart[nlist];
    const int d16 = d & ~15, r = d - d16;      // r: 1 .. 15
    const int i4 = (d & ~7) - d16;             // the 4-lane step's first element, from d16: 0 or 8
    const int i1 = (d & ~3) - d16, rem = d & 3;   // the masked step's
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
        const bool live = entry_row<false>(id, inrow, nraw, nullptr, 0, need_filter, ftab, &rw);
        const Row* rowp = raw + rw * d;
        __syncthreads();   // the previous unit has stored its distances: s_q, s_off, s_xt are free
        if (tid < nqt) {
            const int pr = inv[inv_start[l] + tq0 + tid];
            const int q = pr / P;
            s_q[tid] = q;
            s_off[tid] = pair_off[(int64_t)q * (P + 1) + (pr - q * P)];
        }
        // the tail's row values, in flight from here: the thread's four of the 8-wide step, the four of the 4-lane step and the
        // masked step's (both threads of a row ask for the same ones; only the even thread's sum is stored)
        float y8[4] = {0.f, 0.f, 0.f, 0.f}, y4[4] = {0.f, 0.f, 0.f, 0.f}, y1[3] = {0.f, 0.f, 0.f};
        if (r >= 8) lmt_load4<Row, LOADB>(rowp + d16 + 4 * half, y8);
        if (d & 4) lmt_load4<Row, LOADB>(rowp + d16 + i4, y4);
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (m < rem) y1[m] = row_elem_f<Row>(rowp[d16 + i1 + m]);
        __syncthreads();   // s_q is written
        {
            const int qi = tid >> 4, c = tid & 15;   // 256 threads: 16 queries x 16 elements
            reinterpret_cast<float*>(s_xt)[tid] = (qi < nqt && c < r) ? x[(int64_t)s_q[qi] * d + d16 + c] : 0.f;
        }
        f32x2 acc[FS_QT][2];
#pragma unroll
        for (int qi = 0; qi < FS_QT; qi++) acc[qi][0] = acc[qi][1] = f32x2{0.f, 0.f};
        int e0 = 0;
        for (; e0 + FS_SLAB <= d16; e0 += FS_SLAB) lmt_piece<L2, Row, FS_SLAB, LOADB>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc);
        if (d16 - e0 >= 64) {
            lmt_piece<L2, Row, 64, LOADB>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc);
            e0 += 64;
        }
        if (d16 - e0 >= 32) {
            lmt_piece<L2, Row, 32, LOADB>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc);
            e0 += 32;
        }
        if (d16 - e0 >= 16) lmt_piece<L2, Row, 16, LOADB>(rowp, x, d, e0, half, tid, nqt, s_q, s_x, acc);
        __syncthreads();   // s_xt is written (d < 16: no piece has put a barrier behind it)
#pragma unroll
        for (int qi = 0; qi < FS_QT; qi++) {
            if (qi < nqt) {
                const float4* xt = s_xt + 4 * qi;
                float a0 = acc[qi][0].x, a1 = acc[qi][0].y, a2 = acc[qi][1].x, a3 = acc[qi][1].y;
                if (r >= 8) {   // lane l takes element d16 + l into its chain: the even thread lanes 0-3, the odd one 4-7
                    const float4 xv = xt[half];
                    a0 = lmt_step<L2>(xv.x, y8[0], a0);
                    a1 = lmt_step<L2>(xv.y, y8[1], a1);
                    a2 = lmt_step<L2>(xv.z, y8[2], a2);
                    a3 = lmt_step<L2>(xv.w, y8[3], a3);
                }
                // even thread: AVX lanes 0..3, odd thread: lanes 4..7;  s[l] = acc[l+4] + acc[l]
                float s0, s1, s2, s3;
                add_xor1_x4(a0, a1, a2, a3, s0, s1, s2, s3);
                if (d & 4) {   // the 4-lane step, on the folded sums
                    const float4 xv = xt[i4 >> 2];
                    s0 = lmt_step<L2>(xv.x, y4[0], s0);
                    s1 = lmt_step<L2>(xv.y, y4[1], s1);
                    s2 = lmt_step<L2>(xv.z, y4[2], s2);
                    s3 = lmt_step<L2>(xv.w, y4[3], s3);
                }
                if (rem) {   // the masked step: lanes at or beyond rem are left alone
                    const float4 xv = xt[i1 >> 2];
                    s0 = lmt_step<L2>(xv.x, y1[0], s0);
                    if (rem > 1) s1 = lmt_step<L2>(xv.y, y1[1], s1);
                    if (rem > 2) s2 = lmt_step<L2>(xv.z, y1[2], s2);
                }
                float dis = hsum4(s0, s1, s2, s3);
                if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
                if (inrow && half == 0) out[(int64_t)s_q[qi] * q_stride + s_off[qi] + j] = dis;
            }
        }
    }
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

namespace {
// The inverse index of a list-major launch, carved from a.scratch (ivfflat_lm_scratch_bytes): inv [nq * P] the pairs sorted by
// list, then cnt | start | cur [nlist], ustart [nlist + 1] the lists' work units.  sliced: units of FS_QT queries (the
// row-sliced kernels), else of FL_UQ.
struct LmIndex {
    const int *start, *cnt, *inv, *ustart;
};
LmIndex lm_inverse_index(hipStream_t s, const IvfflatScanArgs& a, bool sliced) {
    int* inv = static_cast<int*>(a.scratch);
    int* cnt = inv + (size_t)a.nq * a.P;
    int* start = cnt + a.nlist;
    int* cur = start + a.nlist;
    int* ustart = cur + a.nlist;
    const int npairs = a.nq * a.P;
    (void)hipMemsetAsync(cnt, 0, (size_t)a.nlist * sizeof(int), s);
    hipLaunchKernelGGL(k_inv_count, dim3((npairs + 255) / 256), dim3(256), 0, s, a.probe, npairs, a.nlist, a.list_len, cnt);
    if (sliced) hipLaunchKernelGGL(k_inv_scan_s, dim3(1), dim3(1024), 0, s, cnt, a.list_len, a.nlist, start, cur, ustart);
    else hipLaunchKernelGGL(k_inv_scan, dim3(1), dim3(1024), 0, s, cnt, a.list_len, a.nlist, start, cur, ustart);
    hipLaunchKernelGGL(k_inv_fill, dim3((npairs + 255) / 256), dim3(256), 0, s, a.probe, npairs, a.nlist, a.list_len, start, cur, inv);
    return LmIndex{start, cnt, inv, ustart};
}

constexpr int LM_GRID = 256 * 8;   // persistent: every workgroup walks the unit list with stride gridDim.x

// what every list-major kernel takes behind its leading (x[, d], P) and in front of its trailing tab or (slot, nslot)
#define GH_LM_ARGS                                                                                                               \
    a.pair_off, a.list_off, a.list_len, a.ids, raw, a.nraw, ix.start, ix.cnt, ix.inv, ix.ustart, a.nlist, a.q_stride, a.out, a.ftab, \
        a.need_filter, a.min_score, a.max_score

// LM_FIXED (d in {16, 32, 64, 96, 128}) and LM_SLICED, dense or -- a.slot -- sparse
template <class Row>
void launch_lm_t(hipStream_t s, const IvfflatScanArgs& a, bool sliced) {
    const LmIndex ix = lm_inverse_index(s, a, sliced);
    const Row* raw = a.rows.as<Row>();
    if constexpr (!RowKind<Row>::sq8) {
        if (a.slot) {   // a sparse store: the same two kernels with the vid -> row table
#define GH_FLSP(LL, DD) \
    hipLaunchKernelGGL((k_ivfflat_lm_sp<LL, DD, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.P, GH_LM_ARGS, a.slot, a.nslot)
#define GH_FLSPD(LL)                       \
    switch (a.d) {                         \
        case 128: GH_FLSP(LL, 128); break; \
        case 96: GH_FLSP(LL, 96); break;   \
        case 64: GH_FLSP(LL, 64); break;   \
        case 32: GH_FLSP(LL, 32); break;   \
        case 16: GH_FLSP(LL, 16); break;   \
        default: break;                    \
    }
            if (sliced) {
                if (a.l2)
                    hipLaunchKernelGGL((k_ivfflat_lms_sp<true, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS, a.slot,
                                       a.nslot);
                else
                    hipLaunchKernelGGL((k_ivfflat_lms_sp<false, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS, a.slot,
                                       a.nslot);
            } else if (a.l2) {
                GH_FLSPD(true)
            } else {
                GH_FLSPD(false)
            }
#undef GH_FLSPD
#undef GH_FLSP
            return;
        }
    }
    const RowTab<Row> tab = row_tab<Row>(a.rows.tab);
    if (sliced) {
        if (a.l2) hipLaunchKernelGGL((k_ivfflat_lms<true, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS, tab);
        else hipLaunchKernelGGL((k_ivfflat_lms<false, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS, tab);
        return;
    }
#define GH_FL(LL, DD) hipLaunchKernelGGL((k_ivfflat_lm<LL, DD, Row>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.P, GH_LM_ARGS, tab)
#define GH_FLD(LL)                       \
    switch (a.d) {                       \
        case 128: GH_FL(LL, 128); break; \
        case 96: GH_FL(LL, 96); break;   \
        case 64: GH_FL(LL, 64); break;   \
        case 32: GH_FL(LL, 32); break;   \
        case 16: GH_FL(LL, 16); break;   \
        default: break;                  \
    }
    if (a.l2) { GH_FLD(true) } else { GH_FLD(false) }
#undef GH_FLD
#undef GH_FL
}

// LM_TAIL (d % 16 != 0): the row-sliced kernel's inverse index, then k_ivfflat_lmt with the load width the row length allows
template <class Row, int LOADB>
void launch_lmt_k(hipStream_t s, const IvfflatScanArgs& a) {
    const LmIndex ix = lm_inverse_index(s, a, true);
    const Row* raw = a.rows.as<Row>();
    if (a.l2) hipLaunchKernelGGL((k_ivfflat_lmt<true, Row, LOADB>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS);
    else hipLaunchKernelGGL((k_ivfflat_lmt<false, Row, LOADB>), dim3(LM_GRID), dim3(256), 0, s, a.x, a.d, a.P, GH_LM_ARGS);
}
#undef GH_LM_ARGS
}  // namespace

void launch_ivfflat_lm(hipStream_t s, IvfflatScanPlan::Kind kind, const IvfflatScanArgs& a) {
    if (a.nq <= 0 || a.P <= 0) return;
    const int et = a.rows.et;
    if (kind == IvfflatScanPlan::LM_FIXED || kind == IvfflatScanPlan::LM_SLICED) {
        const bool sliced = kind == IvfflatScanPlan::LM_SLICED;
        switch (et) {
            case ROW_F32: launch_lm_t<float>(s, a, sliced); break;
            case ROW_F16: launch_lm_t<uint16_t>(s, a, sliced); break;
            case ROW_U8: launch_lm_t<uint8_t>(s, a, sliced); break;
            case ROW_I8: launch_lm_t<int8_t>(s, a, sliced); break;
            case ROW_SQ8:   // (codes are never numbers: an sq8 store goes to the decoding kernels or, sparse, nowhere)
                if (!a.slot) launch_lm_t<sq8_t>(s, a, sliced);
                break;
            default: break;
        }
        return;
    }
    if (kind != IvfflatScanPlan::LM_TAIL) return;
    int k3 = 0, lb = 0, qtile = 0;
    // (dense rows that are numbers, of a length with a tail: an sq8 or a sparse store has no such kernel)
    if (et < ROW_F32 || et > ROW_I8 || a.slot || ivfflat_lm_tail_shape(a.d, (int)a.rows.esz(), &k3, &lb, &qtile) != 3) return;
#define GH_FLT(T, B) \
    case B: launch_lmt_k<T, B>(s, a); break;
    switch (et) {
        case ROW_F32:
            switch (lb) { GH_FLT(float, 16) GH_FLT(float, 8) GH_FLT(float, 4) }
            break;
        case ROW_F16:
            switch (lb) { GH_FLT(uint16_t, 16) GH_FLT(uint16_t, 8) GH_FLT(uint16_t, 4) GH_FLT(uint16_t, 2) }
            break;
        case ROW_U8:
            switch (lb) { GH_FLT(uint8_t, 8) GH_FLT(uint8_t, 4) GH_FLT(uint8_t, 2) GH_FLT(uint8_t, 1) }
            break;
        default:
            switch (lb) { GH_FLT(int8_t, 8) GH_FLT(int8_t, 4) GH_FLT(int8_t, 2) GH_FLT(int8_t, 1) }
            break;
    }
#undef GH_FLT
}

}  // namespace gh
