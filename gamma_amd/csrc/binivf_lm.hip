// binivf_lm.hip -- the spread chain's two heavy passes turned list-major, for large batches.
//
// The chain of binivf_spread.hip gives a workgroup to every (query, chunk): each pair reads its rows twice and shares them
// with no other query.  Here a workgroup owns a chunk of a LIST -- kBinSpreadChunk rows, the same cut as the chain's, so a
// list chunk IS a chunk of every query that probes the list -- keeps its rows in registers and runs a tile of
// kBinLmQueryTile of those queries past them.  The (query, probe) pairs of a list come from the counting sort IVFFLAT builds
// per call (k_inv_count / k_inv_scan_b / k_inv_fill, ivfflat.hip).  What the two kernels write is what k_bin_sp_hist and
// k_bin_sp_collect write, to the same places -- hist[q][chunk][0 .. nbits], the query's candidate segment from off[q][chunk]
// on in row order -- so k_bin_sp_table, k_bin_sp_bounds and k_bin_sp_replay run unchanged and the chain's exactness argument
// (section 23) holds word for word.
//   k_bin_lm_prep     per query: the chunk index of its every probe's first chunk (k_bin_sp_table's prefix); clears the
//                     inverse index's counters
//   k_bin_lm_hist     per unit: the valid rows inside the score window at every distance, for every query of the tile
//   k_bin_lm_collect  per unit: the rows with dis < B_c of every query of the tile as (arena position, dis), in row order
// A unit = (list, chunk, tile); a persistent grid walks the unit list, whose length stays on the device.  A (query, chunk)
// pair belongs to exactly one unit: plain vector stores, no global atomics but one profiling counter.
//
// Rows in registers: a wave owns a contiguous quarter of the chunk (256 rows), which it walks in four steps of 64 rows, lane
// = row.  A thread holds R rows of W words: 4 x 8 up to 256 bits, 2 x 16, 1 x 32, 1 x 64 beyond -- 32 VGPRs (64 at 2048
// bits) -- and a chunk takes 4 / R passes.  Validity that does not depend on the query (id >= 0, is_valid_doc under the
// call's one filter context) is one bit per row, evaluated as the row is loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bin_dev.h"
#include "binivf.h"
#include "filter_dev.h"

namespace gh {

namespace {
// (the kernels' only fp32 work is the score window's compares; they carry the single-lane attribute of ivfflat.hip all the same)
#if defined(__HIP_DEVICE_COMPILE__)
#define GH_LM_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__
#else
#define GH_LM_KERNEL __global__   // (the host pass does not know the feature)
#endif
constexpr int kLmThreads = 256;
constexpr int kLmWaves = kLmThreads / 64;
constexpr int kLmSteps = kBinSpreadChunk / kLmThreads;   // 64-row steps of a wave's quarter
constexpr int kLmQt = kBinLmQueryTile;
// LDS counters of k_bin_lm_hist: the whole tile's histograms up to 263 bits per code, sub-tiles of fewer queries beyond (4
// at 2048 bits)
constexpr int kLmHistWords = kLmQt * 264;
constexpr int kLmGrid = 256 * 8;   // persistent, as IVFFLAT's list-major kernels
static_assert(kLmSteps == 4 && kLmQt <= 64, "a wave's quarter is four steps; a tile is staged by one wave's worth of threads");

struct LmUnit {
    int c;          // chunk of the list
    int r0, len;    // its first row, the list's length
    int nqt;        // queries of the tile
    int first;      // the tile's first pair in inv
    int64_t base;   // arena position of the list's row 0
};

// unit u of the call: lists in order, a list's chunks in order, a chunk's tiles in order (neighbouring workgroups read the
// same rows)
__device__ __forceinline__ LmUnit lm_unit(int u, const int* __restrict__ ustart, int nlist, const int* __restrict__ inv_start,
                                          const int* __restrict__ inv_cnt, const int64_t* __restrict__ list_off,
                                          const int* __restrict__ list_len) {
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {   // last list with ustart[l] <= u
        const int mid = (lo + hi + 1) >> 1;
        if (ustart[mid] <= u) lo = mid; else hi = mid - 1;
    }
    LmUnit t;
    const int n = inv_cnt[lo], tiles = (n + kLmQt - 1) / kLmQt, rel = u - ustart[lo];
    t.c = rel / tiles;
    const int tq0 = (rel - t.c * tiles) * kLmQt;
    t.r0 = t.c * kBinSpreadChunk;
    t.len = list_len[lo];
    t.nqt = min(kLmQt, n - tq0);
    t.first = inv_start[lo] + tq0;
    t.base = list_off[lo];
    return t;
}

// the tile's queries: s_qc = q * maxch + the query's index of this chunk (-1: beyond the host's bound, which no query
// reaches), s_qw = their words, W per query, zero beyond nw.  Barriers inside; the caller's LDS reads of the previous unit
// are over when it returns.
template <int W>
__device__ __forceinline__ void lm_stage_tile(const LmUnit& t, const int* __restrict__ inv, int P, const int* __restrict__ pbase,
                                              int maxch, const uint8_t* __restrict__ x, int64_t xs, int cs, int nw, int* s_q,
                                              int64_t* s_qc, uint32_t* s_qw) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < t.nqt) {
        const int pr = inv[t.first + tid];
        const int q = pr / P;
        const int ch = pbase[pr] + t.c;
        s_q[tid] = q;
        s_qc[tid] = ch < maxch ? (int64_t)q * maxch + ch : -1;
    }
    __syncthreads();
    for (int e = tid; e < t.nqt * W; e += kLmThreads) {
        const int qi = e / W, w = e - qi * W;
        s_qw[e] = w < nw ? bin_word_bytes(x + (int64_t)s_q[qi] * xs, w, cs) : 0u;
    }
    __syncthreads();
}

// rows pass * R .. pass * R + R - 1 of this lane's column of its wave's quarter; *fl: bit j = row j passes IsValid
template <int LW, int R, int W>
__device__ __forceinline__ void lm_load_rows(const LmUnit& t, int pass, const uint8_t* __restrict__ codes,
                                             const int64_t* __restrict__ ids, int cs, int nw,
                                             const FilterDesc* __restrict__ ftab, int need_filter, uint32_t (&cw)[R][W],
                                             unsigned* fl) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned f = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int r = t.r0 + wv * (kBinSpreadChunk / kLmWaves) + (pass * R + j) * 64 + lane;
        const bool in = r < t.len;
        bin_row_load<LW, W>(codes + (t.base + r) * cs, in, cs, nw, cw[j]);
        if (in) {
            const int64_t id = ids[t.base + r];
            if (id >= 0 && (!need_filter || is_valid_doc(ftab[0], id))) f |= 1u << j;
        }
    }
    *fl = f;
}

__device__ __forceinline__ bool lm_in_window(int d, float min_score, float max_score) {
    const float dis = (float)d;
    return dis <= max_score && dis >= min_score;   // IsSimilarScoreValid
}
}  // namespace

// one wave per query: pbase [nq][P] = the chunks of the probes before p in the query's scan order (k_bin_sp_table's `first`);
// cnt [nlist] = 0 for k_inv_count
__global__ __launch_bounds__(64) void k_bin_lm_prep(const int* __restrict__ probe, int nq, int P,
                                                    const int* __restrict__ list_len, int* __restrict__ pbase, int nlist,
                                                    int* __restrict__ cnt) {
    const int lane = threadIdx.x;
    for (int i = blockIdx.x * 64 + lane; i < nlist; i += gridDim.x * 64) cnt[i] = 0;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        int run = 0;
        for (int p0 = 0; p0 < P; p0 += 64) {
            const int p = p0 + lane;
            const int l = p < P ? probe[(int64_t)q * P + p] : -1;
            const int len = l >= 0 ? list_len[l] : 0;
            const int n = (len + kBinSpreadChunk - 1) / kBinSpreadChunk;
            int incl = n;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (p < P) pbase[(int64_t)q * P + p] = run + incl - n;
            run += __shfl(incl, 63);
        }
    }
}

// The LDS histograms: one copy per query of the sub-tile, bin b of query i at word i * nb + b.  The distances of a wave's 64
// rows to one query cluster in a few dozen NEIGHBOURING bins, which lie in neighbouring banks, so a ds_add of 64 lanes meets
// only the serialisation of the lanes that share a bin (a handful), beside 16 XOR + 16 v_bcnt per row and query at 256 bits;
// per-wave copies would cut the tile to a quarter (a barrier pair per sub-tile).  Measured, the stage is
// not bound by that arithmetic: the same-bin serialisation is the first suspect, a form that sorts lanes by bin the follow-up.
// Flush: a wave per query, 64 bins per store, the counters cleared as they are read.
template <int LW, int R, int W>
GH_LM_KERNEL __launch_bounds__(kLmThreads) void k_bin_lm_hist(const uint8_t* __restrict__ x, int64_t xs, int cs, int P,
                                                            const int* __restrict__ pbase, int maxch,
                                                            const int* __restrict__ inv, const int* __restrict__ inv_start,
                                                            const int* __restrict__ inv_cnt, const int* __restrict__ ustart,
                                                            int nlist, const int64_t* __restrict__ list_off,
                                                            const int* __restrict__ list_len,
                                                            const uint8_t* __restrict__ codes,
                                                            const int64_t* __restrict__ ids,
                                                            const FilterDesc* __restrict__ ftab, int need_filter,
                                                            float min_score, float max_score, uint32_t* __restrict__ hist,
                                                            unsigned long long* __restrict__ units_stat) {
    __shared__ uint32_t s_h[kLmHistWords];
    __shared__ __align__(16) uint32_t s_qw[kLmQt * W];
    __shared__ int s_q[kLmQt];
    __shared__ int64_t s_qc[kLmQt];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nb = cs * 8 + 1, nw = (cs + 3) >> 2;
    const int qs = min(kLmQt, kLmHistWords / nb);   // queries per sub-tile
    const int nunits = ustart[nlist];
    if (units_stat && blockIdx.x == 0 && tid == 0) atomicAdd(units_stat, (unsigned long long)nunits);
    for (int i = tid; i < kLmHistWords; i += kLmThreads) s_h[i] = 0u;
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        const LmUnit t = lm_unit(u, ustart, nlist, inv_start, inv_cnt, list_off, list_len);
        lm_stage_tile<W>(t, inv, P, pbase, maxch, x, xs, cs, nw, s_q, s_qc, s_qw);
        for (int pass = 0; pass < kLmSteps / R; pass++) {
            uint32_t cw[R][W];
            unsigned fl;
            lm_load_rows<LW, R, W>(t, pass, codes, ids, cs, nw, ftab, need_filter, cw, &fl);
            for (int q0 = 0; q0 < t.nqt; q0 += qs) {
                const int q1 = min(t.nqt, q0 + qs);
                for (int qi = q0; qi < q1; qi++) {
                    int d[R];
                    bin_rows_hamming<R, W>(cw, s_qw + qi * W, nw, d);
                    uint32_t* hq = s_h + (qi - q0) * nb;
#pragma unroll
                    for (int j = 0; j < R; j++)
                        if (((fl >> j) & 1u) && lm_in_window(d[j], min_score, max_score)) atomicAdd(&hq[d[j]], 1u);
                }
                __syncthreads();
                for (int qi = q0 + wv; qi < q1; qi += kLmWaves) {
                    uint32_t* hq = s_h + (qi - q0) * nb;
                    const int64_t qc = s_qc[qi];
                    uint32_t* hc = hist + qc * nb;
                    for (int b = lane; b < nb; b += 64) {
                        const uint32_t v = hq[b];
                        hq[b] = 0u;
                        // a later pass adds to what this lane stored in the pass before
                        if (qc >= 0) hc[b] = pass == 0 ? v : hc[b] + v;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// Two phases per unit, one barrier between them.  Phase 1: every wave runs the tile's queries that have a candidate in this
// chunk (B = 0 for the others: k_bin_sp_bounds counted none) past its rows and leaves the ballot of `dis < B` of each of its
// four steps in LDS.  Phase 2: a row's place in the query's segment is off[q][chunk] + the set bits of the waves before + of
// this wave's steps before + of the lanes before; only the waves and queries with a set bit compute a distance again.
template <int LW, int R, int W>
GH_LM_KERNEL __launch_bounds__(kLmThreads) void k_bin_lm_collect(const uint8_t* __restrict__ x, int64_t xs, int cs, int P,
                                                               const int* __restrict__ pbase, int maxch,
                                                               const int* __restrict__ inv,
                                                               const int* __restrict__ inv_start,
                                                               const int* __restrict__ inv_cnt,
                                                               const int* __restrict__ ustart, int nlist,
                                                               const int64_t* __restrict__ list_off,
                                                               const int* __restrict__ list_len,
                                                               const uint8_t* __restrict__ codes,
                                                               const int64_t* __restrict__ ids,
                                                               const FilterDesc* __restrict__ ftab, int need_filter,
                                                               float min_score, float max_score,
                                                               const int* __restrict__ nchq, const int* __restrict__ bound,
                                                               const uint32_t* __restrict__ off,
                                                               const uint32_t* __restrict__ total, int64_t stride,
                                                               uint2* __restrict__ cand) {
    __shared__ __align__(16) unsigned long long s_mask[kLmQt][kLmWaves][kLmSteps];
    __shared__ __align__(16) uint32_t s_qw[kLmQt * W];
    __shared__ int s_q[kLmQt];
    __shared__ int64_t s_qc[kLmQt];
    __shared__ int s_B[kLmQt];
    __shared__ uint32_t s_o0[kLmQt];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nw = (cs + 3) >> 2;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int nunits = ustart[nlist];
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        const LmUnit t = lm_unit(u, ustart, nlist, inv_start, inv_cnt, list_off, list_len);
        lm_stage_tile<W>(t, inv, P, pbase, maxch, x, xs, cs, nw, s_q, s_qc, s_qw);
        if (tid < t.nqt) {
            const int64_t qc = s_qc[tid];
            int B = 0;
            uint32_t o0 = 0;
            if (qc >= 0) {
                const int q = s_q[tid];
                const int ch = (int)(qc - (int64_t)q * maxch);
                o0 = off[qc];
                B = (ch + 1 < nchq[q] ? off[qc + 1] : total[q]) != o0 ? bound[qc] : 0;
            }
            s_B[tid] = B;
            s_o0[tid] = o0;
        }
        __syncthreads();
        uint32_t cw[R][W];
        unsigned fl = 0;
        for (int pass = 0; pass < kLmSteps / R; pass++) {
            lm_load_rows<LW, R, W>(t, pass, codes, ids, cs, nw, ftab, need_filter, cw, &fl);
            for (int qi = 0; qi < t.nqt; qi++) {
                const int B = s_B[qi];
                if (B == 0) continue;   // (the whole workgroup)
                int d[R];
                bin_rows_hamming<R, W>(cw, s_qw + qi * W, nw, d);
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const bool take = ((fl >> j) & 1u) && lm_in_window(d[j], min_score, max_score) && d[j] < B;
                    const unsigned long long mk = __ballot(take);
                    if (lane == 0) s_mask[qi][wv][pass * R + j] = mk;
                }
            }
        }
        __syncthreads();
        for (int pass = 0; pass < kLmSteps / R; pass++) {
            // (one pass: the rows of phase 1 are still in the registers)
            if (kLmSteps / R > 1) lm_load_rows<LW, R, W>(t, pass, codes, ids, cs, nw, ftab, need_filter, cw, &fl);
            for (int qi = 0; qi < t.nqt; qi++) {
                if (s_B[qi] == 0) continue;
                uint32_t at = s_o0[qi];   // the place of this wave's step pass * R
                unsigned long long own = 0;
#pragma unroll
                for (int w2 = 0; w2 < kLmWaves; w2++)
#pragma unroll
                    for (int st = 0; st < kLmSteps; st++) {
                        const unsigned long long m = s_mask[qi][w2][st];
                        if (w2 < wv || (w2 == wv && st < pass * R)) at += (uint32_t)__popcll(m);
                        if (w2 == wv && st >= pass * R && st < pass * R + R) own |= m;
                    }
                if (own == 0) continue;   // (the whole wave)
                int d[R];
                bin_rows_hamming<R, W>(cw, s_qw + qi * W, nw, d);
                uint2* cq = cand + (int64_t)s_q[qi] * stride;
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const unsigned long long mk = s_mask[qi][wv][pass * R + j];
                    const int64_t pos = (int64_t)at + __popcll(mk & below);
                    const int r = t.r0 + wv * (kBinSpreadChunk / kLmWaves) + (pass * R + j) * 64 + lane;
                    if (((mk >> lane) & 1ull) && pos < stride) cq[pos] = make_uint2((uint32_t)(t.base + r), (uint32_t)d[j]);
                    at += (uint32_t)__popcll(mk);
                }
            }
        }
    }
}

int64_t bin_lm_unit_bound(int nq, int P, int nlist, int max_list_len) {
    const int64_t pairs = (int64_t)std::max(0, nq) * std::max(0, std::min(P, nlist));
    const int64_t chunks = ((int64_t)std::max(0, max_list_len) + kBinSpreadChunk - 1) / kBinSpreadChunk;
    return (pairs / kLmQt + std::min<int64_t>(pairs, std::max(0, nlist))) * chunks;
}

size_t bin_lm_meta_bytes(int nq, int P, int maxch) {
    return ((bin_spread_meta_bytes(nq, maxch) + 15) & ~(size_t)15) + (size_t)nq * P * sizeof(int);
}

// inv [nq * P] | cnt | start | cur [nlist] | ustart [nlist + 1]
size_t bin_lm_inv_bytes(int nq, int P, int nlist) { return ((size_t)nq * P + 4 * (size_t)nlist + 1) * sizeof(int); }

namespace {
struct LmArgs {
    hipStream_t s;
    const uint8_t* x;
    int64_t xs;
    int cs, P;
    const int* pbase;
    int maxch;
    const int *inv, *start, *cnt, *ustart;
    int nlist;
    const int64_t* list_off;
    const int* list_len;
    const uint8_t* codes;
    const int64_t* ids;
    const FilterDesc* ftab;
    int need_filter;
    float min_score, max_score;
    int grid;
};

template <int LW, int R, int W>
void lm_hist(const LmArgs& a, uint32_t* hist, unsigned long long* units_stat) {
    hipLaunchKernelGGL((k_bin_lm_hist<LW, R, W>), dim3(a.grid), dim3(kLmThreads), 0, a.s, a.x, a.xs, a.cs, a.P, a.pbase, a.maxch,
                       a.inv, a.start, a.cnt, a.ustart, a.nlist, a.list_off, a.list_len, a.codes, a.ids, a.ftab, a.need_filter,
                       a.min_score, a.max_score, hist, units_stat);
}

template <int LW, int R, int W>
void lm_collect(const LmArgs& a, const int* nchq, const int* bound, const uint32_t* off, const uint32_t* total, int64_t stride,
                uint2* cand) {
    hipLaunchKernelGGL((k_bin_lm_collect<LW, R, W>), dim3(a.grid), dim3(kLmThreads), 0, a.s, a.x, a.xs, a.cs, a.P, a.pbase,
                       a.maxch, a.inv, a.start, a.cnt, a.ustart, a.nlist, a.list_off, a.list_len, a.codes, a.ids, a.ftab,
                       a.need_filter, a.min_score, a.max_score, nchq, bound, off, total, stride, cand);
}

// the load width the code size allows x the register shape the word count needs
#define GH_LM_SHAPES(FN, ...)                                   \
    do {                                                        \
        const int nw_ = (a.cs + 3) >> 2;                        \
        const int lw_ = a.cs % 16 == 0 ? 16 : a.cs % 4 == 0 ? 4 : 1; \
        if (nw_ <= 8) GH_LM_LW(FN, 4, 8, __VA_ARGS__);          \
        else if (nw_ <= 16) GH_LM_LW(FN, 2, 16, __VA_ARGS__);   \
        else if (nw_ <= 32) GH_LM_LW(FN, 1, 32, __VA_ARGS__);   \
        else GH_LM_LW(FN, 1, 64, __VA_ARGS__);                  \
    } while (0)
#define GH_LM_LW(FN, R, W, ...)                         \
    do {                                                \
        if (lw_ == 16) FN<16, R, W>(a, __VA_ARGS__);    \
        else if (lw_ == 4) FN<4, R, W>(a, __VA_ARGS__); \
        else FN<1, R, W>(a, __VA_ARGS__);               \
    } while (0)
}  // namespace

void launch_bin_lm(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P, int nlist,
                   int max_list_len, const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                   const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, int maxch,
                   int64_t stride, uint32_t* hist, void* meta, void* inv_ws, uint2* cand, float* D, int64_t* I,
                   unsigned long long* stats, unsigned long long* lm_stats, int stage) {
    if (nq <= 0 || k <= 0) return;
    const int64_t ub = bin_lm_unit_bound(nq, P, nlist, max_list_len);
    if (k > kBinMaxK || cs <= 0 || cs > kBinMaxCodeSize || P <= 0 || nlist <= 0 || maxch < 0 || stride < 0 ||
        (int64_t)nq * P > 2147483647 || ub > 2147483647)
        return launch_refused("bin_lm: k / code size / nq x nprobe");
    const int nb = cs * 8 + 1;
    // meta: the chain's block (launch_bin_spread), then pbase [nq][P]
    char* mp = static_cast<char*>(meta);
    int2* cmap = reinterpret_cast<int2*>(mp);
    int* bound = reinterpret_cast<int*>(mp + (size_t)nq * maxch * sizeof(int2));
    uint32_t* off = reinterpret_cast<uint32_t*>(bound + (size_t)nq * maxch);
    int* nchq = reinterpret_cast<int*>(off + (size_t)nq * maxch);
    uint32_t* total = reinterpret_cast<uint32_t*>(nchq + nq);
    int* pbase = reinterpret_cast<int*>(mp + ((bin_spread_meta_bytes(nq, maxch) + 15) & ~(size_t)15));
    int* inv = static_cast<int*>(inv_ws);
    int* cnt = inv + (size_t)nq * P;
    int* start = cnt + nlist;
    int* cur = start + nlist;
    int* ustart = cur + nlist;
    const int npairs = nq * P;
    const LmArgs a = {s, x, xs, cs, P, pbase, maxch, inv, start, cnt, ustart, nlist, list_off, list_len, codes, ids, ftab,
                      need_filter, min_score, max_score, (int)std::max<int64_t>(1, std::min<int64_t>(ub, kLmGrid))};
    if (stage == 0 || stage == 1) {
        hipLaunchKernelGGL(k_bin_lm_prep, dim3(nq), dim3(64), 0, s, probe, nq, P, list_len, pbase, nlist, cnt);
        hipLaunchKernelGGL(k_inv_count, dim3((npairs + 255) / 256), dim3(256), 0, s, probe, npairs, nlist, list_len, cnt);
        hipLaunchKernelGGL(k_inv_scan_b, dim3(1), dim3(1024), 0, s, cnt, list_len, nlist, start, cur, ustart);
        hipLaunchKernelGGL(k_inv_fill, dim3((npairs + 255) / 256), dim3(256), 0, s, probe, npairs, nlist, list_len, start, cur,
                           inv);
        hipLaunchKernelGGL(k_bin_sp_table, dim3(nq), dim3(64), 0, s, probe, nq, P, list_len, maxch, cmap, nchq);
        if (maxch > 0) GH_LM_SHAPES(lm_hist, hist, lm_stats ? lm_stats + 3 : nullptr);
        hipLaunchKernelGGL(k_bin_sp_bounds, dim3(nq), dim3(64), (size_t)nb * sizeof(uint32_t), s, hist, nq, nchq, maxch, nb,
                           k, bound, off, total);
    }
    if (stage == 0 || stage == 2) {
        if (maxch > 0) GH_LM_SHAPES(lm_collect, nchq, bound, off, total, stride, cand);
    }
    if (stage == 0 || stage == 3) {
        const size_t lds = ((size_t)(k + 2) * 8 + 15) & ~(size_t)15;
        hipLaunchKernelGGL(k_bin_sp_replay, dim3(nq), dim3(64), lds, s, cand, stride, total, nchq, nq, k, ids, D, I, stats,
                           lm_stats);
    }
}

}  // namespace gh
