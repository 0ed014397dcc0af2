// binflat.hip -- exact Hamming search over every stored code (faiss:IndexBinaryFlat.cpp, utils/hamming.cpp:230-265), answered
// as GammaIVFBinaryScannerL2::scan_codes (gamma_index_binary_ivf.cc:333-448) answers one list that holds every code in vid
// order: IsValid, the Hamming distance, IsSimilarScoreValid, `dis < simi[0] -> heap_pop + heap_push`, heap_reorder.
//
// The heap's final array depends on every admission, in order (binivf.hip), so the admissions are replayed by one wave
// per query -- but over a small part of the rows only, and that part is found by the whole device:
//   * the heap holds the k smallest valid distances seen so far, so its top before row i is the k-th smallest valid
//     distance of the rows before i (the sentinel while fewer than k are valid), and the top never rises;
//   * cut the rows into chunks of kBinFlatChunk and let B_c be the k-th smallest valid distance of the rows before chunk c:
//     every row of chunk c that the heap admits has dis < B_c (top <= B_c inside the chunk);
//   * replaying only the rows with dis < B_c, in vid order, with the replay's own `dis < top` test performs the same
//     sequence of heap operations: the rows left out are exactly rows the serial scan would have rejected.
// k_binflat_hist counts, per (query, chunk), the valid rows at every distance 0..nbits; k_binflat_bounds walks a query's
// chunk histograms and yields B_c and the number of candidates per (query, chunk), hence segment offsets without atomics;
// k_binflat_collect recomputes the distances and writes the candidates (vid, dis) in vid order by ballot-ordered
// compaction; k_binflat_replay is the scan of binivf.hip over the candidates.  Distances are integers <= 2048: exact as
// floats, and the same in both passes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bin_dev.h"
#include "binflat.h"
#include "filter_dev.h"
#include "heap_dev.h"

namespace gh {

namespace {
constexpr int kBfThreads = 256;                 // hist / collect: four waves
constexpr size_t kBfLdsCap = 64 * 1024;         // a workgroup's LDS (two or more workgroups per CU of 160 KB)

__device__ __forceinline__ uint32_t bf_word_bytes(const uint8_t* p, int w, int cs) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int i = 4 * w + b;
        if (i < cs) v |= (uint32_t)p[i] << (8 * b);
    }
    return v;
}

// the words of the tile's QT queries -> qw [QT][nwq] (nwq: nw rounded up to 4; zero beyond the code and beyond nq)
template <int QT>
__device__ __forceinline__ void bf_load_queries(const uint8_t* x, int nq, int64_t xs, int q0, int cs, int nw, int nwq,
                                                uint32_t* qw) {
    for (int i = (int)threadIdx.x; i < QT * nwq; i += kBfThreads) {
        const int t = i / nwq, w = i - t * nwq, q = q0 + t;
        qw[i] = (q < nq && w < nw) ? bf_word_bytes(x + (int64_t)q * xs, w, cs) : 0u;
    }
}

// popcount(q_t ^ c) for the QT queries of the tile over ONE read of the row: 16-byte loads when cs % 16 == 0, dwords
// when cs % 4 == 0, bytes otherwise (rows are cs bytes apart from a 256-byte aligned base); the query words are LDS
// broadcasts
// MASKED: only the queries whose bit is set in act (wave-uniform) are scored; the others' acc stays 0
template <int QT, bool MASKED = false>
__device__ __forceinline__ void bf_dist(const uint32_t* qw, int nwq, const uint8_t* c, int cs, int nw, int (&acc)[QT],
                                        unsigned act = ~0u) {
#pragma unroll
    for (int t = 0; t < QT; t++) acc[t] = 0;
    if ((cs & 15) == 0) {
        const uint4* c4 = reinterpret_cast<const uint4*>(c);
        for (int i = 0; i < (nw >> 2); i++) {
            const uint4 v = c4[i];
#pragma unroll
            for (int t = 0; t < QT; t++) {
                if (MASKED && !((act >> t) & 1u)) continue;
                const uint4 q = *reinterpret_cast<const uint4*>(qw + t * nwq + 4 * i);
                acc[t] += __popc(v.x ^ q.x) + __popc(v.y ^ q.y) + __popc(v.z ^ q.z) + __popc(v.w ^ q.w);
            }
        }
    } else if ((cs & 3) == 0) {
        const uint32_t* c32 = reinterpret_cast<const uint32_t*>(c);
        for (int w = 0; w < nw; w++) {
            const uint32_t v = c32[w];
#pragma unroll
            for (int t = 0; t < QT; t++) {
                if (MASKED && !((act >> t) & 1u)) continue;
                acc[t] += __popc(v ^ qw[t * nwq + w]);
            }
        }
    } else {
        for (int w = 0; w < nw; w++) {
            const uint32_t v = bf_word_bytes(c, w, cs);
#pragma unroll
            for (int t = 0; t < QT; t++) {
                if (MASKED && !((act >> t) & 1u)) continue;
                acc[t] += __popc(v ^ qw[t * nwq + w]);
            }
        }
    }
}

inline size_t bf_align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t bf_hist_lds(int qt, int cs) {
    const int nw = (cs + 3) >> 2, nwq = (nw + 3) & ~3;
    return bf_align16((size_t)qt * (cs * 8 + 1) * sizeof(uint32_t)) + (size_t)qt * nwq * sizeof(uint32_t);
}
}  // namespace

// grid (chunk, query tile); LDS: QT histograms of nbits + 1 counters, the tile's query words
template <int QT>
__global__ __launch_bounds__(kBfThreads) void k_binflat_hist(const uint8_t* __restrict__ x, int nq, int64_t xs,
                                                             const uint8_t* __restrict__ codes, int64_t n, int cs,
                                                             const FilterDesc* __restrict__ ftab, int need_filter,
                                                             float min_score, float max_score, uint32_t* __restrict__ hist) {
    extern __shared__ __align__(16) char smem[];
    const int nb = cs * 8 + 1, nw = (cs + 3) >> 2, nwq = (nw + 3) & ~3;
    uint32_t* sh = reinterpret_cast<uint32_t*>(smem);
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem + (((size_t)QT * nb * sizeof(uint32_t) + 15) & ~(size_t)15));
    const int64_t c = blockIdx.x, nch = gridDim.x;
    const int q0 = (int)blockIdx.y * QT;
    for (int i = (int)threadIdx.x; i < QT * nb; i += kBfThreads) sh[i] = 0u;
    bf_load_queries<QT>(x, nq, xs, q0, cs, nw, nwq, qw);
    __syncthreads();
    const int64_t r0 = c * kBinFlatChunk, r1 = min(n, r0 + (int64_t)kBinFlatChunk);
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBfThreads) {
        if (need_filter && !is_valid_doc(ftab[0], r)) continue;   // IsValid
        int acc[QT];
        bf_dist<QT>(qw, nwq, codes + r * cs, cs, nw, acc);
#pragma unroll
        for (int t = 0; t < QT; t++) {
            const float dis = (float)acc[t];
            if (q0 + t < nq && dis <= max_score && dis >= min_score) atomicAdd(&sh[t * nb + acc[t]], 1u);   // IsSimilarScoreValid
        }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < QT * nb; i += kBfThreads) {
        const int t = i / nb, b = i - t * nb, q = q0 + t;
        if (q < nq) hist[((int64_t)q * nch + c) * nb + b] = sh[i];
    }
}

// one wave per query; LDS: the running histogram (bins above the bound are never needed again: the bound never rises)
__global__ __launch_bounds__(64) void k_binflat_bounds(const uint32_t* __restrict__ hist, int nq, int64_t nch, int nb, int k,
                                                       int* __restrict__ bound, uint32_t* __restrict__ off,
                                                       uint32_t* __restrict__ total) {
    extern __shared__ __align__(16) char smem[];
    uint32_t* cum = reinterpret_cast<uint32_t*>(smem);
    const int lane = threadIdx.x;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const uint32_t run = bin_bound_walk(hist + (int64_t)q * nch * nb, nch, nb, k, cum, bound + (int64_t)q * nch,
                                            off + (int64_t)q * nch);
        if (lane == 0) total[q] = run;
    }
}

// grid (chunk, query tile), as k_binflat_hist; rows in steps of 256 in vid order, the four waves' counts of a step
// exchanged through LDS (double buffered: one barrier per step).  Beyond chunk 0 few (query, chunk) pairs hold a candidate:
// a query without one in this chunk is not scored again, a tile without one ends at once.
template <int QT>
__global__ __launch_bounds__(kBfThreads) void k_binflat_collect(const uint8_t* __restrict__ x, int nq, int64_t xs,
                                                                const uint8_t* __restrict__ codes, int64_t n, int cs,
                                                                const FilterDesc* __restrict__ ftab, int need_filter,
                                                                float min_score, float max_score,
                                                                const int* __restrict__ bound,
                                                                const uint32_t* __restrict__ off,
                                                                const uint32_t* __restrict__ total,
                                                                const int64_t* __restrict__ base, uint2* __restrict__ cand) {
    extern __shared__ __align__(16) char smem[];
    __shared__ uint32_t s_cnt[2][kBfThreads / 64][QT];
    const int nw = (cs + 3) >> 2, nwq = (nw + 3) & ~3;
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem);
    const int64_t c = blockIdx.x, nch = gridDim.x;
    const int q0 = (int)blockIdx.y * QT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int bq[QT];
    int64_t wp[QT];
    unsigned act = 0;   // the queries of the tile with a candidate in this chunk (k_binflat_bounds counted them)
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const int q = q0 + t;
        uint32_t cnt = 0;
        if (q < nq) {
            const int64_t qc = (int64_t)q * nch + c;
            cnt = (c + 1 < nch ? off[qc + 1] : total[q]) - off[qc];
            wp[t] = base[q] + (int64_t)off[qc];
        } else {
            wp[t] = 0;
        }
        bq[t] = cnt ? bound[(int64_t)q * nch + c] : -1;   // no distance is < -1: such a query collects nothing
        act |= cnt ? 1u << t : 0u;
    }
    act = (unsigned)__builtin_amdgcn_readfirstlane((int)act);
    if (act == 0) return;   // (the whole workgroup: nothing of this chunk is a candidate of the tile)
    bf_load_queries<QT>(x, nq, xs, q0, cs, nw, nwq, qw);
    __syncthreads();
    const int64_t r0 = c * kBinFlatChunk, r1 = min(n, r0 + (int64_t)kBinFlatChunk);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int step = 0;
    for (int64_t rs = r0; rs < r1; rs += kBfThreads, step ^= 1) {
        const int64_t r = rs + threadIdx.x;
        bool ok = r < r1;
        if (ok && need_filter) ok = is_valid_doc(ftab[0], r);
        int acc[QT];
#pragma unroll
        for (int t = 0; t < QT; t++) acc[t] = 0;
        if (ok) bf_dist<QT, true>(qw, nwq, codes + r * cs, cs, nw, acc, act);
        unsigned long long m[QT];
        bool take[QT];
#pragma unroll
        for (int t = 0; t < QT; t++) {
            const float dis = (float)acc[t];
            take[t] = ok && dis <= max_score && dis >= min_score && acc[t] < bq[t];
            m[t] = __ballot(take[t]);
            if (lane == 0) s_cnt[step][wv][t] = (uint32_t)__popcll(m[t]);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < QT; t++) {
            uint32_t pre = 0, tot = 0;
#pragma unroll
            for (int w2 = 0; w2 < kBfThreads / 64; w2++) {
                const uint32_t v = s_cnt[step][w2][t];
                pre += w2 < wv ? v : 0u;
                tot += v;
            }
            if (take[t]) cand[wp[t] + pre + __popcll(m[t] & below)] = make_uint2((uint32_t)r, (uint32_t)acc[t]);
            wp[t] += tot;
        }
    }
}

// one wave per query: k_bin_scan's heap loop (binivf.hip) over the query's candidates; payload = vid
__global__ __launch_bounds__(64) void k_binflat_replay(const uint2* __restrict__ cand, const int64_t* __restrict__ base,
                                                       const uint32_t* __restrict__ total, int nq, int k,
                                                       float* __restrict__ D, int64_t* __restrict__ I,
                                                       unsigned long long* __restrict__ stats) {
    extern __shared__ __align__(16) char smem[];
    const int lane = threadIdx.x;
    uint2* hK = reinterpret_cast<uint2*>(smem);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t tot = total ? (int64_t)total[q] : 0;
        const unsigned long long nadm = bin_replay_segment(cand + (total ? base[q] : 0), tot, k, hK);
        for (int i = lane; i < k; i += 64) {
            const uint2 e = hK[1 + i];
            const bool empty = e.y == 0xffffffffu;
            D[(int64_t)q * k + i] = empty ? 2147483648.f : __uint_as_float(e.x);   // (float)INT32_MAX
            I[(int64_t)q * k + i] = empty ? -1 : (int64_t)e.y;
        }
        if (stats && lane == 0) {
            atomicAdd(stats, 1ull);
            atomicAdd(stats + 1, (unsigned long long)tot);
            atomicAdd(stats + 2, nadm);
        }
    }
}

int binflat_query_tile(int nq, int cs) {
    if (nq <= 1) return 1;
    if (nq > 4 && bf_hist_lds(8, cs) <= kBfLdsCap) return 8;
    return 4;
}

namespace {
inline bool bf_shape_ok(int64_t n, int cs) { return cs > 0 && cs <= kBinMaxCodeSize && n >= 0 && n < ((int64_t)1 << 31); }
inline int64_t bf_chunks(int64_t n) { return (n + kBinFlatChunk - 1) / kBinFlatChunk; }
}  // namespace

void launch_binflat_hist(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* codes, int64_t n, int cs,
                         const FilterDesc* ftab, int need_filter, float min_score, float max_score, uint32_t* hist) {
    if (nq <= 0 || n <= 0) return;
    if (!bf_shape_ok(n, cs)) return launch_refused("binflat_hist: rows / code size");
    const int qt = binflat_query_tile(nq, cs);
    const int tiles = (nq + qt - 1) / qt;
    if (tiles > 65535) return launch_refused("binflat_hist: too many query tiles");
    const dim3 grid((unsigned)bf_chunks(n), (unsigned)tiles);
    const size_t lds = bf_hist_lds(qt, cs);
#define GH_BF_HIST(QT) \
    hipLaunchKernelGGL(k_binflat_hist<QT>, grid, dim3(kBfThreads), lds, s, x, nq, xs, codes, n, cs, ftab, need_filter, \
                       min_score, max_score, hist)
    if (qt == 8) GH_BF_HIST(8);
    else if (qt == 4) GH_BF_HIST(4);
    else GH_BF_HIST(1);
#undef GH_BF_HIST
}

void launch_binflat_bounds(hipStream_t s, const uint32_t* hist, int nq, int64_t n, int cs, int k, int* bound, uint32_t* off,
                           uint32_t* total) {
    if (nq <= 0 || n <= 0 || k <= 0) return;
    if (!bf_shape_ok(n, cs)) return launch_refused("binflat_bounds: rows / code size");
    const int nb = cs * 8 + 1;
    hipLaunchKernelGGL(k_binflat_bounds, dim3(std::min(nq, 65535)), dim3(64), (size_t)nb * sizeof(uint32_t), s, hist, nq,
                       bf_chunks(n), nb, k, bound, off, total);
}

void launch_binflat_collect(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* codes, int64_t n, int cs,
                            const FilterDesc* ftab, int need_filter, float min_score, float max_score, const int* bound,
                            const uint32_t* off, const uint32_t* total, const int64_t* base, uint2* cand) {
    if (nq <= 0 || n <= 0) return;
    if (!bf_shape_ok(n, cs)) return launch_refused("binflat_collect: rows / code size");
    const int qt = binflat_query_tile(nq, cs);
    const int tiles = (nq + qt - 1) / qt;
    if (tiles > 65535) return launch_refused("binflat_collect: too many query tiles");
    const dim3 grid((unsigned)bf_chunks(n), (unsigned)tiles);
    const int nw = (cs + 3) >> 2, nwq = (nw + 3) & ~3;
    const size_t lds = (size_t)qt * nwq * sizeof(uint32_t);
#define GH_BF_COLLECT(QT) \
    hipLaunchKernelGGL(k_binflat_collect<QT>, grid, dim3(kBfThreads), lds, s, x, nq, xs, codes, n, cs, ftab, need_filter, \
                       min_score, max_score, bound, off, total, base, cand)
    if (qt == 8) GH_BF_COLLECT(8);
    else if (qt == 4) GH_BF_COLLECT(4);
    else GH_BF_COLLECT(1);
#undef GH_BF_COLLECT
}

void launch_binflat_replay(hipStream_t s, const uint2* cand, const int64_t* base, const uint32_t* total, int nq, int k,
                           float* D, int64_t* I, unsigned long long* stats) {
    if (nq <= 0 || k <= 0) return;
    if (k > kBinMaxK) return launch_refused("binflat_replay: k");
    const size_t lds = ((size_t)(k + 2) * 8 + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_binflat_replay, dim3(std::min(nq, 65535)), dim3(64), lds, s, cand, base, total, nq, k, D, I, stats);
}

}  // namespace gh
