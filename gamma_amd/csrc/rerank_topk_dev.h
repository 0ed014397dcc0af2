// rerank_topk_dev.h -- what k_rerank_topk (rerank.hip) and k_rerank_topk_filt (rerank_filter.hip) do with the R (key, candidate
// rank) items of a query once they stand in LDS: the first k + 1 of them in order, the tie test, the output.  Called by all 256
// threads of the workgroup.  At the end: the tie test and the output for a query that one wave owns, its first k + 1 items one
// per lane (k_rerank_topk_filt_wave).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_utils.h"
#include "device_math.h"
#include "kernels.h"

namespace gh {

// s_it[0 .. K1) = the K1 smallest of the R items s_it[0 .. R), ascending (s_it holds 1024 items; what stands behind the first K1
// afterwards is unspecified).  Barriers in front (the items are complete) and behind (the first K1 are in place) are part of it.
// Up to K1 = 64: every 64-item run of the R items is sorted by a wave (DPP bitonic stages), the first K1 items of a run get
// their rank in the whole -- their index in the run + the number of smaller items in every other run (binary searches) --
// and the items of rank < K1 go to their place: the same first K1 entries the full rank sort leaves.  (The full sort
// ranks all R items against all R: 200 LDS reads and 600 vector instructions per thread, ~100 of the kernel's 283 us at C3.)
__device__ __forceinline__ void rerank_first_k(unsigned long long* s_it, int R, int K1) {
    if (K1 <= 64) {   // (uniform)
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int nruns = (R + 63) >> 6;   // <= 16
        __syncthreads();   // every item is in s_it
        for (int run = w; run < nruns; run += 4) {
            const int idx = run * 64 + lane;
            s_it[idx] = wave_sort64(idx < R ? s_it[idx] : ~0ull);   // (padding sorts last; s_it holds 1024 items)
        }
        __syncthreads();
        unsigned long long xr[4];
        int rkk[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int run = w + 4 * u;
            xr[u] = ~0ull;
            rkk[u] = K1;
            if (run < nruns) {   // (uniform)
                const unsigned long long x = s_it[run * 64 + lane];
                int rank = lane;
                if (lane < K1 && x != ~0ull) {
                    for (int o = 0; o < nruns; o++) {
                        if (o == run) continue;
                        const unsigned long long* ro = s_it + o * 64;
                        int lo = 0, n2 = 64;
#pragma unroll
                        for (int st = 0; st < 7; st++) {   // number of items of run o smaller than x
                            if (n2 > 0) {
                                const int half = n2 >> 1;
                                if (ro[lo + half] < x) {
                                    lo += half + 1;
                                    n2 -= half + 1;
                                } else {
                                    n2 = half;
                                }
                            }
                        }
                        rank += lo;
                        if (rank >= K1) break;
                    }
                    xr[u] = x;
                    rkk[u] = rank;
                }
            }
        }
        __syncthreads();   // every search has read the runs
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (rkk[u] < K1) s_it[rkk[u]] = xr[u];
        __syncthreads();
    } else {
        block_rank_sort<256, 4>(s_it, R);   // R distinct items (the rank field differs)
    }
}

// Only the first k + 1 items are read: the k results; whether two of the first k + 1 exact distances are equal.  *s_tie was set
// by thread 0 in front of rerank_first_k (the query's cut flag) when tf.list is set.
template <bool L2>
__device__ __forceinline__ void rerank_topk_out(const unsigned long long* s_it, const int64_t* s_id, int* s_tie, int q, int R, int k,
                                                float neutral, float* __restrict__ distances, int64_t* __restrict__ labels,
                                                const TieFlags& tf) {
    const float sentinel = L2 ? INFINITY : -INFINITY;
    if (tf.list) {
        // exact ties (ties.hip): two of the first k+1 exact distances equal -- their order, or which of them
        // stays inside the k, is decided by the reference's heaps -- or the top-R cut went through a tie
        for (int i = threadIdx.x; i < k && i + 1 < R; i += 256) {
            const uint32_t ka = (uint32_t)(s_it[i] >> 32), kb = (uint32_t)(s_it[i + 1] >> 32);
            if (ka == kb && ka != (L2 ? f2key(sentinel) : ~f2key(sentinel))) *s_tie = 1;   // benign race: same value
        }
        __syncthreads();
        if (threadIdx.x == 0 && *s_tie) {
            tf.list[atomicAdd(tf.count, 1)] = q;
            if (tf.stats) atomicAdd(tf.stats + 2, 1ull);
        }
    }
    for (int i = threadIdx.x; i < k; i += 256) {
        float val = neutral;
        int64_t id = -1;
        if (i < R) {
            const unsigned long long it = s_it[i];
            const uint32_t key = (uint32_t)(it >> 32);
            const float dv = key2f(L2 ? key : ~key);
            if (dv != sentinel) {
                val = dv;
                id = s_id[(uint32_t)it];
            }
        }
        distances[(int64_t)q * k + i] = val;
        labels[(int64_t)q * k + i] = id;
    }
}

// ---- the same for a query that one wave owns (k_rerank_topk_filt_wave): no workgroup barrier anywhere ----
// LDS that one lane of a wave wrote and another lane of the same wave reads: the wave's DS instructions execute in program
// order, so all that is needed is that the compiler keeps that order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The first K1 = min(k + 1, R) <= 64 items stand one per lane, ascending: `item` of lane i is item i (lanes from K1 on: anything).
// tie: the query's cut flag (uniform over the wave).  Called by all 64 lanes.
template <bool L2>
__device__ __forceinline__ void rerank_topk_out_wave(unsigned long long item, const int64_t* s_id, int tie, int q, int R, int k,
                                                     float neutral, float* __restrict__ distances, int64_t* __restrict__ labels,
                                                     const TieFlags& tf) {
    const float sentinel = L2 ? INFINITY : -INFINITY;
    const int lane = threadIdx.x & 63;
    if (tf.list) {
        const unsigned long long next = __shfl_down(item, 1, 64);
        const uint32_t ka = (uint32_t)(item >> 32), kb = (uint32_t)(next >> 32);
        const bool eq = lane < k && lane + 1 < R && ka == kb && ka != (L2 ? f2key(sentinel) : ~f2key(sentinel));
        if (__ballot(eq)) tie = 1;
        if (lane == 0 && tie) {
            tf.list[atomicAdd(tf.count, 1)] = q;
            if (tf.stats) atomicAdd(tf.stats + 2, 1ull);
        }
    }
    for (int i = lane; i < k; i += 64) {   // (i < k and i < R: i < K1, the lane holds item i)
        float val = neutral;
        int64_t id = -1;
        if (i < R) {
            const uint32_t key = (uint32_t)(item >> 32);
            const float dv = key2f(L2 ? key : ~key);
            if (dv != sentinel) {
                val = dv;
                id = s_id[(uint32_t)item];
            }
        }
        distances[(int64_t)q * k + i] = val;
        labels[(int64_t)q * k + i] = id;
    }
}

}  // namespace gh
