// rerank.hip -- a9: candidate positions -> ids, exact re-rank (compute_dis), the IVFFLAT pair scan, result finalisation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "block_utils.h"
#include "device_math.h"
#include "filter_dev.h"
#include "flat_rows_dev.h"
#include "kernels.h"
#include "rerank_dev.h"
#include "rerank_topk_dev.h"
#include "scan_dev.h"

namespace gh {

// ------------------------------------------------------------------------------------
// positions in a query's candidate segment -> vector ids (KnnSearchResults::add stores
// ids[j], gamma_index_ivfpq.h:363-369).  grid = nq.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_map_candidates(const int* __restrict__ pos, int R, int P,
                                                        const int* __restrict__ probe_list,
                                                        const int* __restrict__ pair_off,
                                                        const int64_t* __restrict__ list_off,
                                                        const int64_t* __restrict__ ids,
                                                        int64_t* __restrict__ cand_ids) {
    map_candidates_row(pos, R, P, probe_list, pair_off, list_off, ids, cand_ids, (int)blockIdx.x);
}
void launch_map_candidates(hipStream_t s, const int* pos, int nq, int R, int P,
                           const int* probe_list, const int* pair_off, const int64_t* list_off,
                           const int64_t* ids, int64_t* cand_ids) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_map_candidates, dim3(nq), dim3(256), 0, s, pos, R, P, probe_list, pair_off,
                       list_off, ids, cand_ids);
}

// ------------------------------------------------------------------------------------
// a9: exact re-rank distances (compute_dis, gamma_index_ivfpq.cc:642-680).  8 threads
// per candidate = the 8 lane accumulators of fvec_L2sqr / fvec_inner_product; the
// cross-lane reduction mirrors extractf128 + add + 2x haddps.  grid = nq, block = 256
// (32 candidates in flight).  Out-of-window scores and empty slots get the sentinel.
// ROW = uint16_t: a float16 raw store (rerank_dev.h: the same arithmetic over the widened row).
// ROW = uint8_t / int8_t: a store of byte rows (gamma_hip_raw_init_i8), likewise.
// ROW = sq8_t: scalar-quantised byte rows (gamma_hip_raw_init_sq8), decoded through tab (rerank_dev.h); tab is null and unread
// for every other row type.
// ------------------------------------------------------------------------------------
template <bool L2, typename ROW = float>
__global__ __launch_bounds__(256) void k_rerank_dist(const float* __restrict__ x, int d,
                                                     const ROW* __restrict__ raw, int64_t nraw,
                                                     const int64_t* __restrict__ cand_ids, int R,
                                                     float min_score, float max_score,
                                                     float* __restrict__ out, const int32_t* __restrict__ slot, int64_t nslot,
                                                     const float2* __restrict__ tab) {
    const int q = blockIdx.x;
    const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
    const float* xq = x + (int64_t)q * d;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    for (int r0 = blockIdx.y * 32; r0 < R; r0 += gridDim.y * 32) {
        const int r = r0 + g;
        int64_t id = -1;
        if (r < R) id = cand_ids[(int64_t)q * R + r];
        if (slot) id = (id >= 0 && id < nslot) ? (int64_t)slot[id] : -1;   // sharded raw store: the row of this vector HERE
        const bool live = id >= 0 && id < nraw;
        float dis;
        if constexpr (std::is_same<ROW, sq8_t>::value)
            dis = rerank_dist8_sq8<L2>(xq, reinterpret_cast<const uint8_t*>(raw) + (live ? id : 0) * d, tab, d, l, live);
        else
            dis = rerank_dist8<L2>(xq, raw + (live ? id : 0) * d, d, l, live);
        if (l == 0 && r < R) {
            if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
            out[(int64_t)q * R + r] = dis;
        }
    }
}
namespace {
template <typename ROW>
void launch_rerank_dist_t(hipStream_t s, bool l2, const float* x, int nq, int d, const ROW* raw, const float* tab, int64_t nraw,
                          const int64_t* cand_ids, int R, float min_score, float max_score, float* out, const int32_t* slot,
                          int64_t nslot) {
    const int gy = (R + 31) / 32;   // 32 candidates (8 lanes each) per workgroup
    const float2* t = reinterpret_cast<const float2*>(tab);
    if (l2)
        hipLaunchKernelGGL((k_rerank_dist<true, ROW>), dim3(nq, gy), dim3(256), 0, s, x, d, raw, nraw, cand_ids, R, min_score,
                           max_score, out, slot, nslot, t);
    else
        hipLaunchKernelGGL((k_rerank_dist<false, ROW>), dim3(nq, gy), dim3(256), 0, s, x, d, raw, nraw, cand_ids, R, min_score,
                           max_score, out, slot, nslot, t);
}
}  // namespace
void launch_rerank_dist(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& raw, int64_t nraw,
                        const int64_t* cand_ids, int R, float min_score, float max_score, float* out, const int32_t* slot,
                        int64_t nslot) {
    if (nq <= 0) return;
    switch (raw.et) {   // (slot: a sparse store's table, rows of any element type)
        case ROW_F32:
            launch_rerank_dist_t(s, l2, x, nq, d, raw.as<float>(), nullptr, nraw, cand_ids, R, min_score, max_score, out, slot, nslot);
            break;
        case ROW_F16:
            launch_rerank_dist_t(s, l2, x, nq, d, raw.as<uint16_t>(), nullptr, nraw, cand_ids, R, min_score, max_score, out, slot, nslot);
            break;
        case ROW_U8:
            launch_rerank_dist_t(s, l2, x, nq, d, raw.as<uint8_t>(), nullptr, nraw, cand_ids, R, min_score, max_score, out, slot, nslot);
            break;
        case ROW_I8:
            launch_rerank_dist_t(s, l2, x, nq, d, raw.as<int8_t>(), nullptr, nraw, cand_ids, R, min_score, max_score, out, slot, nslot);
            break;
        case ROW_SQ8:   // (codes are never numbers: an sq8 store goes to the decoding kernel or nowhere)
            launch_rerank_dist_t(s, l2, x, nq, d, raw.as<sq8_t>(), raw.tab, nraw, cand_ids, R, min_score, max_score, out, slot, nslot);
            break;
        default: launch_refused("launch_rerank_dist: unknown row element type"); break;
    }
}

// Exact distances of the entries of an exported candidate stream that can still be members of the recall_num-heap: ADC value
// within the query's bound and vector held on this shard.  One workgroup per exported row: the entries that qualify are
// compacted 256 at a time (ballot), then scored 32 at a time, 8 lanes each (rerank_dist8: the arithmetic of k_rerank_topk).
// ROW: the sparse store's element type, as in k_rerank_dist -- a narrow row is widened exactly as it is loaded (rerank_dev.h),
// an sq8_t row decoded through tab (null and unread for every other row type).
template <bool L2, typename ROW>
__global__ __launch_bounds__(256) void k_export_exact(const float* __restrict__ xf, int d, const ROW* __restrict__ raw,
                                                      const float2* __restrict__ tab, const int32_t* __restrict__ slot, int64_t nslot,
                                                      const float* __restrict__ vals, const int64_t* __restrict__ ids, int64_t stride,
                                                      const int32_t* __restrict__ off, int P, const float* __restrict__ bound,
                                                      float* __restrict__ ex) {
    __shared__ int s_pos[256];
    __shared__ int s_row[256];
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l8 = tid & 7, g = tid >> 3;
    const int n = (int)min((int64_t)off[(int64_t)f * (P + 1) + P], stride);
    const float b = bound[f];
    const float* xq = xf + (int64_t)f * d;
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + tid;
        bool want = false;
        int row = -1;
        if (j < n) {
            const float v = vals[(int64_t)f * stride + j];
            const int64_t id = ids[(int64_t)f * stride + j];
            // (a filtered entry carries the sentinel: never within a finite bound; NaN bound = every entry)
            const bool in = (b != b) || (L2 ? v <= b : v >= b);
            row = (id >= 0 && id < nslot) ? slot[id] : -1;
            want = in && row >= 0 && fabsf(v) != INFINITY;
            if (!want) ex[(int64_t)f * stride + j] = qnan;
        }
        if (tid == 0) s_n = 0;
        __syncthreads();
        const unsigned long long bal = __ballot(want);
        int base = 0;
        if (lane == 0 && bal) base = atomicAdd(&s_n, __popcll(bal));
        base = __shfl(base, 0, 64);
        if (want) {
            const int at = base + __popcll(bal & ((1ull << lane) - 1ull));
            s_pos[at] = j;
            s_row[at] = row;
        }
        __syncthreads();
        const int m = s_n;
        for (int c0 = 0; c0 < m; c0 += 32) {   // uniform trip count
            const int c = c0 + g;
            const bool live = c < m;
            const int64_t rw = live ? s_row[c] : 0;
            float dis;
            if constexpr (std::is_same<ROW, sq8_t>::value)
                dis = rerank_dist8_sq8<L2>(xq, reinterpret_cast<const uint8_t*>(raw) + rw * d, tab, d, l8, live);
            else
                dis = rerank_dist8<L2>(xq, raw + rw * d, d, l8, live);
            if (l8 == 0 && live) ex[(int64_t)f * stride + s_pos[c]] = dis;
        }
        __syncthreads();
        (void)wv;
    }
}
namespace {
template <typename ROW>
void launch_export_exact_t(hipStream_t s, bool l2, const float* xf, int nf, int d, const ROW* raw, const float* tab, const int32_t* slot,
                           int64_t nslot, const float* vals, const int64_t* ids, int64_t stride, const int32_t* off, int P,
                           const float* bound, float* ex) {
    const float2* t = reinterpret_cast<const float2*>(tab);
    if (l2)
        hipLaunchKernelGGL((k_export_exact<true, ROW>), dim3(nf), dim3(256), 0, s, xf, d, raw, t, slot, nslot, vals, ids, stride, off, P,
                           bound, ex);
    else
        hipLaunchKernelGGL((k_export_exact<false, ROW>), dim3(nf), dim3(256), 0, s, xf, d, raw, t, slot, nslot, vals, ids, stride, off, P,
                           bound, ex);
}
}  // namespace
void launch_export_exact(hipStream_t s, bool l2, const float* xf, int nf, int d, const RowsRef& raw, const int32_t* slot, int64_t nslot,
                         const float* vals, const int64_t* ids, int64_t stride, const int32_t* off, int P, const float* bound, float* ex) {
    if (nf <= 0) return;
    switch (raw.et) {
        case ROW_F32:
            launch_export_exact_t(s, l2, xf, nf, d, raw.as<float>(), nullptr, slot, nslot, vals, ids, stride, off, P, bound, ex);
            break;
        case ROW_F16:
            launch_export_exact_t(s, l2, xf, nf, d, raw.as<uint16_t>(), nullptr, slot, nslot, vals, ids, stride, off, P, bound, ex);
            break;
        case ROW_U8:
            launch_export_exact_t(s, l2, xf, nf, d, raw.as<uint8_t>(), nullptr, slot, nslot, vals, ids, stride, off, P, bound, ex);
            break;
        case ROW_I8:
            launch_export_exact_t(s, l2, xf, nf, d, raw.as<int8_t>(), nullptr, slot, nslot, vals, ids, stride, off, P, bound, ex);
            break;
        case ROW_SQ8:   // (codes are never numbers: an sq8 store goes to the decoding kernel or nowhere)
            launch_export_exact_t(s, l2, xf, nf, d, raw.as<sq8_t>(), raw.tab, slot, nslot, vals, ids, stride, off, P, bound, ex);
            break;
        default: launch_refused("launch_export_exact: unknown row element type"); break;
    }
}

// The exact distance that travelled with each candidate of the merged table: every shard's table row is sorted by ADC value, a
// candidate's (ADC value, id) pair sits in exactly one of them -- lower bound on the value, then the run of equal values.
template <bool L2>
__global__ __launch_bounds__(256) void k_lookup_exact(const float* __restrict__ all_dis, const int64_t* __restrict__ all_ids,
                                                      const float* __restrict__ all_exact, int W, int nq, int R, int q0, int nql,
                                                      const float* __restrict__ cand_dis, const int64_t* __restrict__ cand_ids,
                                                      float* __restrict__ cand_exact) {
    const int ql = blockIdx.x;
    if (ql >= nql) return;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    for (int r = threadIdx.x; r < R; r += 256) {
        const int64_t id = cand_ids[(int64_t)ql * R + r];
        const float v = cand_dis[(int64_t)ql * R + r];
        float out = sentinel;
        if (id >= 0) {
            bool found = false;
            for (int w = 0; w < W && !found; w++) {
                const int64_t rb = ((int64_t)w * nq + q0 + ql) * R;
                int lo = 0, hi = R;   // first position whose value is not better than v (rows are best first)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const float t = all_dis[rb + mid];
                    const bool before = all_ids[rb + mid] >= 0 && (L2 ? t < v : t > v);
                    if (before) lo = mid + 1; else hi = mid;
                }
                for (int j = lo; j < R && all_ids[rb + j] >= 0 && all_dis[rb + j] == v; j++)
                    if (all_ids[rb + j] == id) {
                        out = all_exact[rb + j];
                        found = true;
                        break;
                    }
            }
        }
        cand_exact[(int64_t)ql * R + r] = out;
    }
}
void launch_lookup_exact(hipStream_t s, bool l2, const float* all_dis, const int64_t* all_ids, const float* all_exact, int W, int nq, int R,
                         int q0, int nql, const float* cand_dis, const int64_t* cand_ids, float* cand_exact) {
    if (nql <= 0) return;
    if (l2) hipLaunchKernelGGL((k_lookup_exact<true>), dim3(nql), dim3(256), 0, s, all_dis, all_ids, all_exact, W, nq, R, q0, nql, cand_dis, cand_ids, cand_exact);
    else hipLaunchKernelGGL((k_lookup_exact<false>), dim3(nql), dim3(256), 0, s, all_dis, all_ids, all_exact, W, nq, R, q0, nql, cand_dis, cand_ids, cand_exact);
}

// ------------------------------------------------------------------------------------
// a9, fused: exact re-rank distances + top-k + output in ONE kernel (compute_dis with
// has_rank, gamma_index_ivfpq.cc:646-680).  One workgroup per query: the R exact distances
// become (key, candidate rank) items in LDS, a block rank sort orders them -- equal exact
// distances keep the ADC order of the candidates -- and the first k go out with their ids
// (empty slots: -1 / heap neutral).  R <= 1024.
// ------------------------------------------------------------------------------------
// ROW = uint16_t: a float16 raw store (eight lanes per candidate as for fp32 rows; the row loads: rerank_dev.h).
// ROW = uint8_t / int8_t: byte rows, eight lanes per candidate; d = 128 keeps the query in registers as the fp32 rows do.
// ROW = sq8_t: scalar-quantised byte rows decoded through tab (null and unread for every other row type); d = 128 keeps the
// lane's 16 {step, vmin} pairs in registers beside its query elements.
template <bool L2, typename ROW = float>
__global__ __launch_bounds__(256) void k_rerank_topk(const float* __restrict__ x, int d,
                                                     const ROW* __restrict__ raw, int64_t nraw,
                                                     const int64_t* __restrict__ cand_ids, int R, int k,
                                                     float min_score, float max_score, float neutral,
                                                     float* __restrict__ distances,
                                                     int64_t* __restrict__ labels, int nq,
                                                     const int* __restrict__ qperm, TieFlags tf,
                                                     const float2* __restrict__ tab) {
    __shared__ unsigned long long s_it[1024];
    __shared__ int64_t s_id[1024];
    __shared__ int s_tie;
    // With the scan's query order (qperm: queries sorted by the spatial rank of their nearest list) XCD x takes
    // the x-th eighth of that order: queries running together share candidates (a batch references every raw
    // row ~3 times), so their rows are served by that XCD's L2 instead of HBM.  Results do not depend on it.
    int q = blockIdx.x;
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
    // all candidate ids first (one coalesced pass): the row gathers below then start without a
    // dependent id load in front of each of them
    for (int r = threadIdx.x; r < R; r += 256) s_id[r] = cand_ids[(int64_t)q * R + r];
    __syncthreads();
    auto put = [&](int r, bool live, float dis) {
        if (l == 0 && r < R) {
            if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
            const uint32_t key = L2 ? f2key(dis) : ~f2key(dis);
            s_it[r] = ((unsigned long long)key << 32) | (unsigned)r;
        }
    };
    // every d of half rows, and the fp32 rows of a d other than 128: 32 candidates per round, eight lanes each
    auto rounds_of_32 = [&]() {
        for (int r0 = 0; r0 < R; r0 += 32) {
            const int r = r0 + g;
            int64_t id = -1;
            if (r < R) id = s_id[r];
            const bool live = id >= 0 && id < nraw;
            if constexpr (std::is_same<ROW, sq8_t>::value)
                put(r, live, rerank_dist8_sq8<L2>(xq, reinterpret_cast<const uint8_t*>(raw) + (live ? id : 0) * d, tab, d, l, live));
            else
                put(r, live, rerank_dist8<L2>(xq, raw + (live ? id : 0) * d, d, l, live));
        }
    };
    if constexpr (std::is_same<ROW, sq8_t>::value) {
        if (d == 128 && nraw > 0) {
            // the byte rows' d = 128 form with the decode in front of the chain: the lane's 16 query elements and its 16
            // {step, vmin} pairs in registers, two candidates per group in flight, a row = eight 16-byte loads the group shares
            const uint8_t* rows = reinterpret_cast<const uint8_t*>(raw);
            const int sh = 8 * (l & 3);
            const bool hi = l & 4;
            float xx[16];
            float2 tt[16];
#pragma unroll
            for (int u = 0; u < 16; u++) xx[u] = xq[l + 8 * u];
#pragma unroll
            for (int u = 0; u < 16; u++) tt[u] = tab[l + 8 * u];
            for (int r0 = 0; r0 < R; r0 += 64) {
                const int ra = r0 + g, rb = r0 + 32 + g;
                const int64_t ida = ra < R ? s_id[ra] : -1, idb = rb < R ? s_id[rb] : -1;
                const bool la = ida >= 0 && ida < nraw, lb = idb >= 0 && idb < nraw;
                const uint4* va = reinterpret_cast<const uint4*>(rows + (la ? ida : 0) * 128);
                const uint4* vb = reinterpret_cast<const uint4*>(rows + (lb ? idb : 0) * 128);
                uint32_t ea[16], eb[16];   // the lane's dword of every 8 elements, picked as the chunk arrives
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = va[u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    ea[2 * u] = hi ? wy : wx;
                    ea[2 * u + 1] = hi ? ww : wz;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = vb[u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    eb[2 * u] = hi ? wy : wx;
                    eb[2 * u + 1] = hi ? ww : wz;
                }
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const float fa = sq8_row_f((ea[u] >> sh) & 0xffu, tt[u]), fb = sq8_row_f((eb[u] >> sh) & 0xffu, tt[u]);
                    if (L2) {
                        const float ta = xx[u] - fa, tb = xx[u] - fb;
                        a = __builtin_fmaf(ta, ta, a);
                        b = __builtin_fmaf(tb, tb, b);
                    } else {
                        a = __builtin_fmaf(xx[u], fa, a);
                        b = __builtin_fmaf(xx[u], fb, b);
                    }
                }
                if (!la) a = 0.f;
                if (!lb) b = 0.f;
                const float sa = __shfl_down(a, 4, 8) + a, sb_ = __shfl_down(b, 4, 8) + b;
                const float ta = sa + __shfl_down(sa, 1, 8), tb = sb_ + __shfl_down(sb_, 1, 8);
                put(ra, la, ta + __shfl_down(ta, 2, 8));
                put(rb, lb, tb + __shfl_down(tb, 2, 8));
            }
        } else {
            rounds_of_32();
        }
    } else if constexpr (std::is_same<ROW, uint8_t>::value || std::is_same<ROW, int8_t>::value) {
        if (d == 128 && nraw > 0) {
            // the fp32 rows' d = 128 form over byte rows: the lane's 16 query elements in registers, two candidates per group in
            // flight, a row = eight 16-byte loads that the group's lanes share (rerank_dev.h, rerank_dist8_bytes: lane l's elements
            // l + 8u are byte l & 3 of the dwords (l >> 2) + 2u).  Same chain, same reduction.
            constexpr bool SG = std::is_same<ROW, int8_t>::value;
            const int sh = 8 * (l & 3);
            const bool hi = l & 4;
            float xx[16];
#pragma unroll
            for (int u = 0; u < 16; u++) xx[u] = xq[l + 8 * u];
            for (int r0 = 0; r0 < R; r0 += 64) {
                const int ra = r0 + g, rb = r0 + 32 + g;
                const int64_t ida = ra < R ? s_id[ra] : -1, idb = rb < R ? s_id[rb] : -1;
                const bool la = ida >= 0 && ida < nraw, lb = idb >= 0 && idb < nraw;
                const uint4* va = reinterpret_cast<const uint4*>(raw + (la ? ida : 0) * 128);
                const uint4* vb = reinterpret_cast<const uint4*>(raw + (lb ? idb : 0) * 128);
                uint32_t ea[16], eb[16];   // the lane's dword of every 8 elements, picked as the chunk arrives
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = va[u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    ea[2 * u] = hi ? wy : wx;
                    ea[2 * u + 1] = hi ? ww : wz;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint4 w = vb[u];
                    const uint32_t wx = w.x, wy = w.y, wz = w.z, ww = w.w;
                    eb[2 * u] = hi ? wy : wx;
                    eb[2 * u + 1] = hi ? ww : wz;
                }
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const float fa = byte_row_f<SG>((ea[u] >> sh) & 0xffu), fb = byte_row_f<SG>((eb[u] >> sh) & 0xffu);
                    if (L2) {
                        const float ta = xx[u] - fa, tb = xx[u] - fb;
                        a = __builtin_fmaf(ta, ta, a);
                        b = __builtin_fmaf(tb, tb, b);
                    } else {
                        a = __builtin_fmaf(xx[u], fa, a);
                        b = __builtin_fmaf(xx[u], fb, b);
                    }
                }
                if (!la) a = 0.f;
                if (!lb) b = 0.f;
                const float sa = __shfl_down(a, 4, 8) + a, sb_ = __shfl_down(b, 4, 8) + b;
                const float ta = sa + __shfl_down(sa, 1, 8), tb = sb_ + __shfl_down(sb_, 1, 8);
                put(ra, la, ta + __shfl_down(ta, 2, 8));
                put(rb, lb, tb + __shfl_down(tb, 2, 8));
            }
        } else {
            rounds_of_32();
        }
    } else if constexpr (!std::is_same<ROW, float>::value) {
        rounds_of_32();
    } else if (d == 128 && nraw > 0) {   // (nraw == 0: row 0 of the reserved range may not be mapped yet -- the predicated path below never touches it)
        // d = 128 (C3, C4): the lane's 16 query elements stay in registers for all candidates (they were half of the loads), and TWO
        // candidates per group of 8 lanes are in flight -- the rows are 512 bytes from all over the raw store, the workgroup's seven
        // rounds of dependent row loads were what it waited for.  Same arithmetic as rerank_dist8 (rerank_dev.h): the lane's fma chain
        // over its elements l, l + 8, .., then (a[l] + a[l + 4]), (s0 + s1) + (s2 + s3).
        float xx[16];
#pragma unroll
        for (int u = 0; u < 16; u++) xx[u] = xq[l + 8 * u];
        for (int r0 = 0; r0 < R; r0 += 64) {
            const int ra = r0 + g, rb = r0 + 32 + g;
            const int64_t ida = ra < R ? s_id[ra] : -1, idb = rb < R ? s_id[rb] : -1;
            const bool la = ida >= 0 && ida < nraw, lb = idb >= 0 && idb < nraw;
            const float* va = raw + (la ? ida : 0) * 128 + l;
            const float* vb = raw + (lb ? idb : 0) * 128 + l;
            float fa[16], fb[16];
#if GH_RERANK_TIMING == 1   // timing build (results invalid): the row loads replaced by a constant
#pragma unroll
            for (int u = 0; u < 16; u++) fa[u] = (float)(ra + u), fb[u] = (float)(rb + u);
            (void)va, (void)vb;
#else
#pragma unroll
            for (int u = 0; u < 16; u++) fa[u] = va[8 * u];
#pragma unroll
            for (int u = 0; u < 16; u++) fb[u] = vb[8 * u];
#endif
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int u = 0; u < 16; u++) {
                if (L2) {
                    const float ta = xx[u] - fa[u], tb = xx[u] - fb[u];
                    a = __builtin_fmaf(ta, ta, a);
                    b = __builtin_fmaf(tb, tb, b);
                } else {
                    a = __builtin_fmaf(xx[u], fa[u], a);
                    b = __builtin_fmaf(xx[u], fb[u], b);
                }
            }
            if (!la) a = 0.f;
            if (!lb) b = 0.f;
            const float sa = __shfl_down(a, 4, 8) + a, sb_ = __shfl_down(b, 4, 8) + b;
            const float ta = sa + __shfl_down(sa, 1, 8), tb = sb_ + __shfl_down(sb_, 1, 8);
            put(ra, la, ta + __shfl_down(ta, 2, 8));
            put(rb, lb, tb + __shfl_down(tb, 2, 8));
        }
    } else {
        rounds_of_32();
    }
    if (tf.list && threadIdx.x == 0) s_tie = tf.cut ? tf.cut[q] : 0;
    rerank_first_k(s_it, R, min(k + 1, R));
    rerank_topk_out<L2>(s_it, s_id, &s_tie, q, R, k, neutral, distances, labels, tf);
}
namespace {
template <typename ROW>
void launch_rerank_topk_t(hipStream_t s, bool l2, const float* x, int nq, int d, const ROW* raw, const float* tab, int64_t nraw,
                          const int64_t* cand_ids, int R, int k, float min_score, float max_score, float neutral, float* distances,
                          int64_t* labels, const int* qperm, const TieFlags& tf) {
    const dim3 grid((unsigned)(8 * ((nq + 7) / 8)));
    const float2* t = reinterpret_cast<const float2*>(tab);
    if (l2)
        hipLaunchKernelGGL((k_rerank_topk<true, ROW>), grid, dim3(256), 0, s, x, d, raw, nraw, cand_ids, R, k, min_score,
                           max_score, neutral, distances, labels, nq, qperm, tf, t);
    else
        hipLaunchKernelGGL((k_rerank_topk<false, ROW>), grid, dim3(256), 0, s, x, d, raw, nraw, cand_ids, R, k, min_score,
                           max_score, neutral, distances, labels, nq, qperm, tf, t);
}
}  // namespace
void launch_rerank_topk(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& raw, int64_t nraw,
                        const int64_t* cand_ids, int R, int k, float min_score, float max_score, float neutral, float* distances,
                        int64_t* labels, const int* qperm, const TieFlags* ties) {
    if (nq <= 0) return;
    const TieFlags tf = ties ? *ties : TieFlags{};
    switch (raw.et) {
        case ROW_F32:
            launch_rerank_topk_t(s, l2, x, nq, d, raw.as<float>(), nullptr, nraw, cand_ids, R, k, min_score, max_score, neutral,
                                 distances, labels, qperm, tf);
            break;
        case ROW_F16:
            launch_rerank_topk_t(s, l2, x, nq, d, raw.as<uint16_t>(), nullptr, nraw, cand_ids, R, k, min_score, max_score, neutral,
                                 distances, labels, qperm, tf);
            break;
        case ROW_U8:
            launch_rerank_topk_t(s, l2, x, nq, d, raw.as<uint8_t>(), nullptr, nraw, cand_ids, R, k, min_score, max_score, neutral,
                                 distances, labels, qperm, tf);
            break;
        case ROW_I8:
            launch_rerank_topk_t(s, l2, x, nq, d, raw.as<int8_t>(), nullptr, nraw, cand_ids, R, k, min_score, max_score, neutral,
                                 distances, labels, qperm, tf);
            break;
        case ROW_SQ8:
            launch_rerank_topk_t(s, l2, x, nq, d, raw.as<sq8_t>(), raw.tab, nraw, cand_ids, R, k, min_score, max_score, neutral,
                                 distances, labels, qperm, tf);
            break;
        default: launch_refused("launch_rerank_topk: unknown row element type"); break;
    }
}

// ------------------------------------------------------------------------------------
// IVFFLAT list scan (GammaIVFFlatScanner1::scan_codes, index/impl/gamma_index_ivfflat.h:52-75): the reference's
// lists hold the vectors themselves; here a list holds vector ids and the rows come from the raw store (the same
// floats).  One workgroup per (query, probe) pair, eight threads per list entry = the eight AVX lane accumulators
// of fvec_L2sqr / fvec_inner_product (rerank_dev.h).  Entries with bit 63, filtered docs and scores outside the
// window get the sentinel; one fp32 per entry into the query's slab at the pair's offset.
// ------------------------------------------------------------------------------------
// Row: the raw store's element type (float; uint16_t = IEEE binary16, uint8_t, int8_t with gamma_hip_set_ivfflat_narrow_rows):
// the row access is rerank_dist8, which widens a narrow row exactly and runs the same fma chain (rerank_dev.h), any d.
// sq8_t (gamma_hip_set_ivfflat_sq8_rows): rerank_dist8_sq8 with the store's decode table (tab: RowTab<Row>, flat_rows_dev.h --
// empty for every other type), the byte rows' loads and the decode in front of the same chain.
// SPARSE: the rows of a sparse store through its vid -> row table (entry_row, filter_dev.h); the dense kernels pass false.
template <bool L2, class Row, bool SPARSE>
__device__ __forceinline__ void ivfflat_scan_body(const float* __restrict__ x, int d, int P,
                                                  const int* __restrict__ pair_off,
                                                  const int64_t* __restrict__ pair_base,
                                                  const int64_t* __restrict__ ids,
                                                  const Row* __restrict__ raw, int64_t nraw, int64_t q_stride,
                                                  float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                  int need_filter, float min_score, float max_score, RowTab<Row> tab,
                                                  const int32_t* __restrict__ slot, int64_t nslot) {
    const int q = blockIdx.x / P, p = blockIdx.x - q * P;
    const int off = pair_off[(int64_t)q * (P + 1) + p], len = pair_off[(int64_t)q * (P + 1) + p + 1] - off;
    if (len <= 0) return;   // uniform
    const int64_t base = pair_base[(int64_t)q * P + p];
    const float* xq = x + (int64_t)q * d;
    const int l8 = threadIdx.x & 7, g = threadIdx.x >> 3;
    const float sentinel = L2 ? INFINITY : -INFINITY;
    for (int j0 = 0; j0 < len; j0 += 32) {
        const int j = j0 + g;
        int64_t id = -1;
        if (j < len) id = ids[base + j];
        int64_t rw;
        const bool live = entry_row<SPARSE>(id, j < len, nraw, slot, nslot, need_filter, ftab, &rw);
        float dis;
        if constexpr (RowKind<Row>::sq8)
            dis = rerank_dist8_sq8<L2>(xq, reinterpret_cast<const uint8_t*>(raw) + rw * d, tab.t, d, l8, live);
        else
            dis = rerank_dist8<L2>(xq, raw + rw * d, d, l8, live);
        if (l8 == 0 && j < len) {
            if (!live || !(dis <= max_score && dis >= min_score)) dis = sentinel;
            out[(int64_t)q * q_stride + off + j] = dis;
        }
    }
}
template <bool L2, class Row = float>
__global__ __launch_bounds__(256) void k_ivfflat_scan(const float* __restrict__ x, int d, int P,
                                                      const int* __restrict__ pair_off,
                                                      const int64_t* __restrict__ pair_base,
                                                      const int64_t* __restrict__ ids,
                                                      const Row* __restrict__ raw, int64_t nraw, int64_t q_stride,
                                                      float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                      int need_filter, float min_score, float max_score, RowTab<Row> tab) {
    ivfflat_scan_body<L2, Row, false>(x, d, P, pair_off, pair_base, ids, raw, nraw, q_stride, out, ftab, need_filter, min_score,
                                      max_score, tab, nullptr, 0);
}
template <bool L2, class Row = float>
__global__ __launch_bounds__(256) void k_ivfflat_scan_sp(const float* __restrict__ x, int d, int P,
                                                         const int* __restrict__ pair_off,
                                                         const int64_t* __restrict__ pair_base,
                                                         const int64_t* __restrict__ ids,
                                                         const Row* __restrict__ raw, int64_t nraw, int64_t q_stride,
                                                         float* __restrict__ out, const FilterDesc* __restrict__ ftab,
                                                         int need_filter, float min_score, float max_score,
                                                         const int32_t* __restrict__ slot, int64_t nslot) {
    ivfflat_scan_body<L2, Row, true>(x, d, P, pair_off, pair_base, ids, raw, nraw, q_stride, out, ftab, need_filter, min_score,
                                     max_score, RowTab<Row>{}, slot, nslot);
}
// fp32 rows of a sparse store: slot [nslot] = vector id -> row of `raw` (nraw rows), -1 = not held here
void launch_ivfflat_scan_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                                const int64_t* pair_base, const int64_t* ids, const float* raw, int64_t nraw, const int32_t* slot,
                                int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter,
                                float min_score, float max_score) {
    if (nq <= 0 || P <= 0 || !slot) return;
    const dim3 grid((unsigned)((int64_t)nq * P));
    if (l2)
        hipLaunchKernelGGL((k_ivfflat_scan_sp<true>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw, q_stride,
                           out, ftab, need_filter, min_score, max_score, slot, nslot);
    else
        hipLaunchKernelGGL((k_ivfflat_scan_sp<false>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw, q_stride,
                           out, ftab, need_filter, min_score, max_score, slot, nslot);
}
namespace {
template <class Row>
void launch_ivfflat_scan_sparse_t(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                                  const int64_t* pair_base, const int64_t* ids, const Row* raw, int64_t nraw, const int32_t* slot,
                                  int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter,
                                  float min_score, float max_score) {
    if (nq <= 0 || P <= 0 || !slot) return;
    const dim3 grid((unsigned)((int64_t)nq * P));
    if (l2)
        hipLaunchKernelGGL((k_ivfflat_scan_sp<true, Row>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, slot, nslot);
    else
        hipLaunchKernelGGL((k_ivfflat_scan_sp<false, Row>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, slot, nslot);
}
}  // namespace
// ... of any element type but sq8 (a sparse sq8 store is refused before it gets here: nothing is launched for one)
void launch_ivfflat_scan_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                                const int64_t* pair_base, const int64_t* ids, const RowsRef& raw, int64_t nraw,
                                const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                                int need_filter, float min_score, float max_score) {
    switch (raw.et) {
        case 0:
            launch_ivfflat_scan_sparse(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<float>(), nraw, slot, nslot, q_stride,
                                       out, ftab, need_filter, min_score, max_score);
            break;
        case 1:
            launch_ivfflat_scan_sparse_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<uint16_t>(), nraw, slot, nslot,
                                         q_stride, out, ftab, need_filter, min_score, max_score);
            break;
        case 2:
            launch_ivfflat_scan_sparse_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<uint8_t>(), nraw, slot, nslot,
                                         q_stride, out, ftab, need_filter, min_score, max_score);
            break;
        case 3:
            launch_ivfflat_scan_sparse_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<int8_t>(), nraw, slot, nslot,
                                         q_stride, out, ftab, need_filter, min_score, max_score);
            break;
        default: break;
    }
}
void launch_ivfflat_scan(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                         const int64_t* pair_base, const int64_t* ids, const float* raw, int64_t nraw, int64_t q_stride,
                         float* out, const FilterDesc* ftab, int need_filter, float min_score, float max_score) {
    if (nq <= 0 || P <= 0) return;
    const dim3 grid((unsigned)((int64_t)nq * P));
    if (l2)
        hipLaunchKernelGGL((k_ivfflat_scan<true>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, RowTab<float>{});
    else
        hipLaunchKernelGGL((k_ivfflat_scan<false>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, RowTab<float>{});
}
namespace {
template <class Row>
void launch_ivfflat_scan_t(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                           const int64_t* pair_base, const int64_t* ids, const Row* raw, int64_t nraw, int64_t q_stride,
                           float* out, const FilterDesc* ftab, int need_filter, float min_score, float max_score,
                           RowTab<Row> tab = RowTab<Row>{}) {
    if (nq <= 0 || P <= 0) return;
    const dim3 grid((unsigned)((int64_t)nq * P));
    if (l2)
        hipLaunchKernelGGL((k_ivfflat_scan<true, Row>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, tab);
    else
        hipLaunchKernelGGL((k_ivfflat_scan<false, Row>), grid, dim3(256), 0, s, x, d, P, pair_off, pair_base, ids, raw, nraw,
                           q_stride, out, ftab, need_filter, min_score, max_score, tab);
}
}  // namespace
// rows of any element type (gamma_hip_set_ivfflat_narrow_rows, _sq8_rows); fp32 rows: the launch above, the kernels it always ran
void launch_ivfflat_scan(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                         const int64_t* pair_base, const int64_t* ids, const RowsRef& raw, int64_t nraw, int64_t q_stride,
                         float* out, const FilterDesc* ftab, int need_filter, float min_score, float max_score) {
    switch (raw.et) {
        case 0:
            launch_ivfflat_scan(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<float>(), nraw, q_stride, out, ftab,
                                need_filter, min_score, max_score);
            break;
        case 1:
            launch_ivfflat_scan_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<uint16_t>(), nraw, q_stride, out, ftab,
                                  need_filter, min_score, max_score);
            break;
        case 2:
            launch_ivfflat_scan_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<uint8_t>(), nraw, q_stride, out, ftab,
                                  need_filter, min_score, max_score);
            break;
        case 3:
            launch_ivfflat_scan_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<int8_t>(), nraw, q_stride, out, ftab,
                                  need_filter, min_score, max_score);
            break;
        case 4:   // (codes are never numbers: an sq8 store goes to the decoding kernel or nowhere)
            launch_ivfflat_scan_t(s, l2, x, nq, d, P, pair_off, pair_base, ids, raw.as<sq8_t>(), nraw, q_stride, out, ftab,
                                  need_filter, min_score, max_score, row_tab<sq8_t>(raw.tab));
            break;
        default: break;
    }
}

// final outputs from a top-k selection over re-ranked (or flat) candidates:
//   labels = src_ids ? src_ids[q][pos] : id_base + pos ; empty -> -1 / heap neutral
__global__ __launch_bounds__(256) void k_finalize_topk(const float* __restrict__ sel_vals,
                                                       const int* __restrict__ sel_pos, int k,
                                                       const int64_t* __restrict__ src_ids,
                                                       int64_t src_stride, int64_t id_base,
                                                       float neutral,
                                                       float* __restrict__ distances,
                                                       int64_t* __restrict__ labels, int n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * k) return;
    const int q = (int)(i / k);
    const int ps = sel_pos[i];
    if (ps < 0) {
        distances[i] = neutral;
        labels[i] = -1;
    } else {
        distances[i] = sel_vals[i];
        labels[i] = src_ids ? src_ids[(int64_t)q * src_stride + ps] : id_base + (int64_t)ps;
    }
}
void launch_finalize_topk(hipStream_t s, const float* sel_vals, const int* sel_pos, int nq, int k,
                          const int64_t* src_ids, int64_t src_stride, int64_t id_base,
                          float neutral, float* distances, int64_t* labels) {
    if (nq <= 0 || k <= 0) return;
    int64_t tot = (int64_t)nq * k;
    hipLaunchKernelGGL(k_finalize_topk, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, sel_vals,
                       sel_pos, k, src_ids, src_stride, id_base, neutral, distances, labels, nq);
}

// has_rank == false (gamma_index_ivfpq.cc:681-696): candidates are already sorted by ADC
// distance; copy the first k whose score is inside the window.  grid = nq.
__global__ __launch_bounds__(256) void k_finalize_norank(const float* __restrict__ cand_dis,
                                                         const int64_t* __restrict__ cand_ids, int R,
                                                         int k, float min_score, float max_score,
                                                         float neutral, float* __restrict__ distances,
                                                         int64_t* __restrict__ labels, TieFlags tf) {
    __shared__ int s_w[4];
    __shared__ int s_tie;
    const int q = blockIdx.x;
    int running = 0;
    if (tf.list && threadIdx.x == 0) s_tie = tf.cut ? tf.cut[q] : 0;
    for (int r0 = 0; r0 < R && running < k; r0 += 256) {
        const int r = r0 + threadIdx.x;
        float dis = 0.f;
        int64_t id = -1;
        if (r < R) {
            dis = cand_dis[(int64_t)q * R + r];
            id = cand_ids[(int64_t)q * R + r];
        }
        const int flag = (id != -1 && dis <= max_score && dis >= min_score) ? 1 : 0;
        int tot;
        const int ex = block_excl_scan256(flag, s_w, tot);
        const int slot = running + ex;
        if (flag && slot < k) {
            distances[(int64_t)q * k + slot] = dis;
            labels[(int64_t)q * k + slot] = id;
            // exact ties (ties.hip): an entry that is taken and its successor at the same ADC distance -- their
            // order, or which of them is the k-th, is whatever heap_reorder of the reference's R-heap leaves
            if (tf.list && r + 1 < R && cand_ids[(int64_t)q * R + r + 1] != -1 &&
                cand_dis[(int64_t)q * R + r + 1] == dis)
                s_tie = 1;
        }
        running += tot;
    }
    if (tf.list) {
        __syncthreads();
        if (threadIdx.x == 0 && s_tie) {
            tf.list[atomicAdd(tf.count, 1)] = q;
            if (tf.stats) atomicAdd(tf.stats + 2, 1ull);
        }
    }
    for (int i = min(running, k) + threadIdx.x; i < k; i += 256) {
        distances[(int64_t)q * k + i] = neutral;
        labels[(int64_t)q * k + i] = -1;
    }
}
void launch_finalize_norank(hipStream_t s, const float* cand_dis, const int64_t* cand_ids, int nq,
                            int R, int k, float min_score, float max_score, float neutral,
                            float* distances, int64_t* labels, const TieFlags* ties) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_finalize_norank, dim3(nq), dim3(256), 0, s, cand_dis, cand_ids, R, k,
                       min_score, max_score, neutral, distances, labels, ties ? *ties : TieFlags{});
}

}  // namespace gh
