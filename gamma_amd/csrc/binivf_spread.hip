// binivf_spread.hip -- the binary IVF scan of ONE query spread over the device.
//
// k_bin_scan (binivf.hip) gives a query to one wave, which walks its nprobe lists alone.  The argument of binflat.hip holds
// for any fixed row sequence, and the sequence GammaIVFBinaryScannerL2::scan_codes (gamma_index_binary_ivf.cc:333-448)
// walks for a query is its probed lists in coarse order, each list in arena order: cut it into chunks of kBinSpreadChunk
// rows that never span two lists, let B_c be the k-th smallest valid distance of the rows before chunk c, and replay only
// the rows with dis < B_c, in sequence order, through the heap -- the same heap_pop / heap_push sequence as the serial scan.
//   k_bin_sp_table    per query: its chunks (list, first row), probe by probe, and their number;
//   k_bin_sp_hist     per (query, chunk): the valid rows inside the score window at every distance 0..nbits;
//   k_bin_sp_bounds   per query: bin_bound_walk (bin_dev.h) over its chunk histograms;
//   k_bin_sp_collect  per (query, chunk): the rows with dis < B_c as (arena position, dis), in sequence order;
//   k_bin_sp_replay   per query: bin_replay_segment (bin_dev.h), then k_bin_scan's output.
// A row is valid exactly as k_bin_scan finds it: id >= 0, is_valid_doc when a filter is present, the score window on the
// float distance (bin_sp_score, shared by the two passes: the distances are integers, the same in both).
// Every (query, chunk) pair is owned by one workgroup: no global atomics but the profiling counters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bin_dev.h"
#include "binivf.h"
#include "filter_dev.h"
#include "heap_dev.h"

namespace gh {

namespace {
constexpr int kBsThreads = 256;   // hist / collect: four waves

// IsValid + the Hamming distance + IsSimilarScoreValid of the entry at arena position pos: its distance, -1 if the scan
// skips it
template <bool AL>
__device__ __forceinline__ int bin_sp_score(const uint32_t* qw, const uint8_t* __restrict__ codes,
                                            const int64_t* __restrict__ ids, int64_t pos, int cs, int nw,
                                            const FilterDesc* __restrict__ ftab, int need_filter, float min_score,
                                            float max_score) {
    const int64_t id = ids[pos];
    if (id < 0) return -1;
    if (need_filter && !is_valid_doc(ftab[0], id)) return -1;   // IsValid
    const int d = bin_hamming<AL>(qw, codes + pos * cs, cs, nw);
    const float dis = (float)d;
    return (dis <= max_score && dis >= min_score) ? d : -1;   // IsSimilarScoreValid
}
}  // namespace

// one wave per query: cmap [nq][maxch] = (list, first row of the chunk inside the list) of the query's chunks in scan
// order, nchq [nq] = their number (at most maxch: the host's bound on it)
__global__ __launch_bounds__(64) void k_bin_sp_table(const int* __restrict__ probe, int nq, int P,
                                                     const int* __restrict__ list_len, int maxch,
                                                     int2* __restrict__ cmap, int* __restrict__ nchq) {
    const int lane = threadIdx.x;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        int run = 0;   // chunks of the probes before this step (wave uniform)
        for (int p0 = 0; p0 < P; p0 += 64) {
            const int p = p0 + lane;
            const int l = p < P ? probe[(int64_t)q * P + p] : -1;   // -1: not enough centroids for multiprobe
            const int len = l >= 0 ? list_len[l] : 0;
            const int n = (len + kBinSpreadChunk - 1) / kBinSpreadChunk;
            int incl = n;   // inclusive prefix over the lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            const int first = run + incl - n;
            for (int j = 0; j < n; j++)
                if (first + j < maxch) cmap[(int64_t)q * maxch + first + j] = make_int2(l, j * kBinSpreadChunk);
            run += __shfl(incl, 63);
        }
        if (lane == 0) nchq[q] = min(run, maxch);
    }
}

// grid (chunk, query); LDS: nbits + 1 counters, the query's words
template <bool AL>
__global__ __launch_bounds__(kBsThreads) void k_bin_sp_hist(const uint8_t* __restrict__ x, int64_t xs, int cs,
                                                            const int2* __restrict__ cmap, const int* __restrict__ nchq,
                                                            int maxch, const int64_t* __restrict__ list_off,
                                                            const int* __restrict__ list_len,
                                                            const uint8_t* __restrict__ codes,
                                                            const int64_t* __restrict__ ids,
                                                            const FilterDesc* __restrict__ ftab, int need_filter,
                                                            float min_score, float max_score, uint32_t* __restrict__ hist) {
    extern __shared__ __align__(16) char smem[];
    const int q = blockIdx.y, c = blockIdx.x;
    if (c >= nchq[q]) return;   // (the whole workgroup)
    const int nb = cs * 8 + 1, nw = (cs + 3) >> 2;
    uint32_t* sh = reinterpret_cast<uint32_t*>(smem);
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem + bin_align16((size_t)nb * sizeof(uint32_t)));
    for (int i = (int)threadIdx.x; i < nb; i += kBsThreads) sh[i] = 0u;
    bin_load_query(x + (int64_t)q * xs, cs, nw, qw, kBsThreads);
    __syncthreads();
    const int2 m = cmap[(int64_t)q * maxch + c];
    const int r1 = min(list_len[m.x], m.y + kBinSpreadChunk);
    const int64_t base = list_off[m.x];
    for (int r = m.y + (int)threadIdx.x; r < r1; r += kBsThreads) {
        const int d = bin_sp_score<AL>(qw, codes, ids, base + r, cs, nw, ftab, need_filter, min_score, max_score);
        if (d >= 0) atomicAdd(&sh[d], 1u);
    }
    __syncthreads();
    uint32_t* hc = hist + ((int64_t)q * maxch + c) * nb;
    for (int i = (int)threadIdx.x; i < nb; i += kBsThreads) hc[i] = sh[i];
}

// one wave per query; LDS: the running histogram.  bound / off [nq][maxch], total [nq]
__global__ __launch_bounds__(64) void k_bin_sp_bounds(const uint32_t* __restrict__ hist, int nq,
                                                      const int* __restrict__ nchq, int maxch, int nb, int k,
                                                      int* __restrict__ bound, uint32_t* __restrict__ off,
                                                      uint32_t* __restrict__ total) {
    extern __shared__ __align__(16) char smem[];
    uint32_t* cum = reinterpret_cast<uint32_t*>(smem);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const uint32_t run = bin_bound_walk(hist + (int64_t)q * maxch * nb, nchq[q], nb, k, cum,
                                            bound + (int64_t)q * maxch, off + (int64_t)q * maxch);
        if (threadIdx.x == 0) total[q] = run;
    }
}

// grid (chunk, query), as k_bin_sp_hist; rows in steps of 256 in list order, the four waves' counts of a step exchanged
// through LDS (double buffered: one barrier per step).  cand [nq][stride]: the query's segment (stride: the host's bound on
// the rows a query scans, which no candidate count exceeds)
template <bool AL>
__global__ __launch_bounds__(kBsThreads) void k_bin_sp_collect(const uint8_t* __restrict__ x, int64_t xs, int cs,
                                                               const int2* __restrict__ cmap,
                                                               const int* __restrict__ nchq, int maxch,
                                                               const int64_t* __restrict__ list_off,
                                                               const int* __restrict__ list_len,
                                                               const uint8_t* __restrict__ codes,
                                                               const int64_t* __restrict__ ids,
                                                               const FilterDesc* __restrict__ ftab, int need_filter,
                                                               float min_score, float max_score,
                                                               const int* __restrict__ bound,
                                                               const uint32_t* __restrict__ off,
                                                               const uint32_t* __restrict__ total, int64_t stride,
                                                               uint2* __restrict__ cand) {
    extern __shared__ __align__(16) char smem[];
    __shared__ uint32_t s_cnt[2][kBsThreads / 64];
    const int q = blockIdx.y, c = blockIdx.x;
    const int nch = nchq[q];
    if (c >= nch) return;
    const int64_t qc = (int64_t)q * maxch + c;
    const uint32_t o0 = off[qc];
    if ((c + 1 < nch ? off[qc + 1] : total[q]) == o0) return;   // k_bin_sp_bounds counted no candidate in this chunk
    const int B = bound[qc];
    const int nw = (cs + 3) >> 2;
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem);
    bin_load_query(x + (int64_t)q * xs, cs, nw, qw, kBsThreads);
    __syncthreads();
    const int2 m = cmap[qc];
    const int r1 = min(list_len[m.x], m.y + kBinSpreadChunk);
    const int64_t base = list_off[m.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int64_t wp = (int64_t)o0;   // inside the query's segment
    uint2* cq = cand + (int64_t)q * stride;
    int step = 0;
    for (int rs = m.y; rs < r1; rs += kBsThreads, step ^= 1) {
        const int r = rs + (int)threadIdx.x;
        int d = -1;
        if (r < r1) d = bin_sp_score<AL>(qw, codes, ids, base + r, cs, nw, ftab, need_filter, min_score, max_score);
        const bool take = d >= 0 && d < B;
        const unsigned long long mk = __ballot(take);
        if (lane == 0) s_cnt[step][wv] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w2 = 0; w2 < kBsThreads / 64; w2++) {
            const uint32_t v = s_cnt[step][w2];
            pre += w2 < wv ? v : 0u;
            tot += v;
        }
        const int64_t at = wp + pre + __popcll(mk & below);
        if (take && at < stride) cq[at] = make_uint2((uint32_t)(base + r), (uint32_t)d);
        wp += tot;
    }
}

// one wave per query: k_bin_scan's heap loop over the query's candidates (payload = arena position), its output, its
// counters; sp_stats (null unless profiling) += {queries, chunks, candidates}
__global__ __launch_bounds__(64) void k_bin_sp_replay(const uint2* __restrict__ cand, int64_t stride,
                                                      const uint32_t* __restrict__ total, const int* __restrict__ nchq,
                                                      int nq, int k, const int64_t* __restrict__ ids,
                                                      float* __restrict__ D, int64_t* __restrict__ I,
                                                      unsigned long long* __restrict__ stats,
                                                      unsigned long long* __restrict__ sp_stats) {
    extern __shared__ __align__(16) char smem[];
    const int lane = threadIdx.x;
    uint2* hK = reinterpret_cast<uint2*>(smem);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t tot = min((int64_t)total[q], stride);
        const unsigned long long nadm = bin_replay_segment(cand + (int64_t)q * stride, tot, k, hK);
        for (int i = lane; i < k; i += 64) {
            const uint2 e = hK[1 + i];
            const bool empty = e.y == 0xffffffffu;
            D[(int64_t)q * k + i] = empty ? 2147483648.f : __uint_as_float(e.x);   // (float)INT32_MAX
            I[(int64_t)q * k + i] = empty ? -1 : ids[e.y];
        }
        if (lane == 0) {
            if (stats) {
                atomicAdd(stats, 1ull);
                atomicAdd(stats + 1, nadm);
            }
            if (sp_stats) {
                atomicAdd(sp_stats, 1ull);
                atomicAdd(sp_stats + 1, (unsigned long long)nchq[q]);
                atomicAdd(sp_stats + 2, (unsigned long long)tot);
            }
        }
    }
}

void bin_spread_bounds(int P, int nlist, int max_list_len, int* maxch, int64_t* rows) {
    const int64_t probes = std::max(0, std::min(P, nlist));   // the probes of a query are distinct lists
    const int64_t ml = std::max(0, max_list_len);
    *maxch = (int)std::min<int64_t>(probes * ((ml + kBinSpreadChunk - 1) / kBinSpreadChunk), 2147483647);
    *rows = probes * ml;
}

size_t bin_spread_meta_bytes(int nq, int maxch) {
    // cmap, bound, off per (query, chunk); nchq, total per query
    return (size_t)nq * maxch * (sizeof(int2) + sizeof(int) + sizeof(uint32_t)) + (size_t)nq * 2 * sizeof(int) + 64;
}

void launch_bin_spread(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P,
                       const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                       const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, int maxch,
                       int64_t stride, uint32_t* hist, void* meta, uint2* cand, float* D, int64_t* I,
                       unsigned long long* stats, unsigned long long* sp_stats, int stage) {
    if (nq <= 0 || k <= 0) return;
    if (k > kBinMaxK || cs <= 0 || cs > kBinMaxCodeSize || nq > kBinSpreadMaxNq || P <= 0 || maxch < 0 || stride < 0)
        return launch_refused("bin_spread: k / code size / nq");
    const int nb = cs * 8 + 1, nw = (cs + 3) >> 2;
    // meta: cmap [nq][maxch] int2 | bound [nq][maxch] | off [nq][maxch] | nchq [nq] | total [nq]
    char* mp = static_cast<char*>(meta);
    int2* cmap = reinterpret_cast<int2*>(mp);
    int* bound = reinterpret_cast<int*>(mp + (size_t)nq * maxch * sizeof(int2));
    uint32_t* off = reinterpret_cast<uint32_t*>(bound + (size_t)nq * maxch);
    int* nchq = reinterpret_cast<int*>(off + (size_t)nq * maxch);
    uint32_t* total = reinterpret_cast<uint32_t*>(nchq + nq);
    const bool al = (cs & 3) == 0;
    const dim3 grid((unsigned)std::max(1, maxch), (unsigned)nq);
    if (stage == 0 || stage == 1) {
        hipLaunchKernelGGL(k_bin_sp_table, dim3(nq), dim3(64), 0, s, probe, nq, P, list_len, maxch, cmap, nchq);
        if (maxch > 0) {
            const size_t lds = (((size_t)nb * sizeof(uint32_t) + 15) & ~(size_t)15) + (size_t)nw * sizeof(uint32_t);
            if (al)
                hipLaunchKernelGGL(k_bin_sp_hist<true>, grid, dim3(kBsThreads), lds, s, x, xs, cs, cmap, nchq, maxch, list_off,
                                   list_len, codes, ids, ftab, need_filter, min_score, max_score, hist);
            else
                hipLaunchKernelGGL(k_bin_sp_hist<false>, grid, dim3(kBsThreads), lds, s, x, xs, cs, cmap, nchq, maxch, list_off,
                                   list_len, codes, ids, ftab, need_filter, min_score, max_score, hist);
        }
        hipLaunchKernelGGL(k_bin_sp_bounds, dim3(nq), dim3(64), (size_t)nb * sizeof(uint32_t), s, hist, nq, nchq, maxch, nb,
                           k, bound, off, total);
    }
    if (stage == 0 || stage == 2) {
        if (maxch > 0) {
            const size_t lds = (size_t)nw * sizeof(uint32_t);
            if (al)
                hipLaunchKernelGGL(k_bin_sp_collect<true>, grid, dim3(kBsThreads), lds, s, x, xs, cs, cmap, nchq, maxch,
                                   list_off, list_len, codes, ids, ftab, need_filter, min_score, max_score, bound, off, total,
                                   stride, cand);
            else
                hipLaunchKernelGGL(k_bin_sp_collect<false>, grid, dim3(kBsThreads), lds, s, x, xs, cs, cmap, nchq, maxch,
                                   list_off, list_len, codes, ids, ftab, need_filter, min_score, max_score, bound, off, total,
                                   stride, cand);
        }
    }
    if (stage == 0 || stage == 3) {
        const size_t lds = ((size_t)(k + 2) * 8 + 15) & ~(size_t)15;
        hipLaunchKernelGGL(k_bin_sp_replay, dim3(nq), dim3(64), lds, s, cand, stride, total, nchq, nq, k, ids, D, I, stats,
                           sp_stats);
    }
}

}  // namespace gh
