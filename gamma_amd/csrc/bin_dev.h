// bin_dev.h -- device pieces the binary kernels share (binivf.hip, binivf_spread.hip, binflat.hip): the Hamming distance
// of one code, the walk over a query's chunk histograms that yields the candidate bounds, and scan_codes' admission loop
// (gamma_index_binary_ivf.cc:407-448) over a candidate segment.  The argument the last two rest on is in binflat.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "binflat.h"
#include "heap_dev.h"

namespace gh {

__device__ __forceinline__ size_t bin_align16(size_t x) { return (x + 15) & ~(size_t)15; }

// word w of a code: bytes 4w .. 4w + 3, zero beyond cs (the query's padding is zero too: XOR 0)
__device__ __forceinline__ uint32_t bin_word_bytes(const uint8_t* p, int w, int cs) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int i = 4 * w + b;
        if (i < cs) v |= (uint32_t)p[i] << (8 * b);
    }
    return v;
}

// popcount(q ^ c) over a code of cs bytes; q: the query's nw words in LDS (same address on every lane: a broadcast).
// AL: cs % 4 == 0 (rows are dword aligned); 16-byte loads when cs % 16 == 0.
template <bool AL>
__device__ __forceinline__ int bin_hamming(const uint32_t* q, const uint8_t* c, int cs, int nw) {
    int s = 0;
    if (AL) {
        if ((cs & 15) == 0) {
            const uint4* c4 = reinterpret_cast<const uint4*>(c);
            for (int i = 0; i < (nw >> 2); i++) {
                const uint4 v = c4[i];
                s += __popc(v.x ^ q[4 * i]) + __popc(v.y ^ q[4 * i + 1]) + __popc(v.z ^ q[4 * i + 2]) +
                     __popc(v.w ^ q[4 * i + 3]);
            }
        } else {
            const uint32_t* c32 = reinterpret_cast<const uint32_t*>(c);
            for (int w = 0; w < nw; w++) s += __popc(c32[w] ^ q[w]);
        }
    } else {
        for (int w = 0; w < nw; w++) s += __popc(bin_word_bytes(c, w, cs) ^ q[w]);
    }
    return s;
}

// the query's words -> LDS, by a workgroup of nthr threads
__device__ __forceinline__ void bin_load_query(const uint8_t* xq, int cs, int nw, uint32_t* qw, int nthr = 64) {
    for (int w = (int)threadIdx.x; w < nw; w += nthr) qw[w] = bin_word_bytes(xq, w, cs);
}

__device__ __forceinline__ unsigned bin_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave walks the nch chunk histograms of one query (hq [nch][nb], nb = nbits + 1) in order: bound[c] = the k-th
// smallest valid distance of the rows before chunk c (kBinFlatNoBound while fewer than k), off[c] = candidates (rows with
// dis < bound) of the chunks before c; returns the query's candidates.  cum: nb counters in LDS, the running histogram
// (bins above the bound are never needed again: the bound never rises).
__device__ __forceinline__ uint32_t bin_bound_walk(const uint32_t* __restrict__ hq, int64_t nch, int nb, int k,
                                                   uint32_t* cum, int* __restrict__ bound, uint32_t* __restrict__ off) {
    const int lane = threadIdx.x;
    __syncthreads();
    for (int b = lane; b < nb; b += 64) cum[b] = 0u;
    __syncthreads();
    int B = kBinFlatNoBound;        // the k-th smallest valid distance of the rows so far
    long long cnt_le = 0;       // valid rows so far with dis <= B (all of them while there is no bound)
    uint32_t run = 0;           // candidates of the chunks so far
    for (int64_t c = 0; c < nch; c++) {
        const uint32_t* hc = hq + c * nb;
        const int lim = B == kBinFlatNoBound ? nb : B + 1;
        unsigned s_lt = 0, s_le = 0;
        for (int b = lane; b < lim; b += 64) {
            const uint32_t v = hc[b];
            cum[b] += v;
            s_le += v;
            s_lt += b < B ? v : 0u;
        }
        s_lt = bin_wave_sum(s_lt);
        s_le = bin_wave_sum(s_le);
        if (lane == 0) {
            bound[c] = B;
            off[c] = run;
        }
        run += s_lt;
        cnt_le += s_le;
        __syncthreads();
        if (B == kBinFlatNoBound && cnt_le >= k) B = nb - 1;
        if (B != kBinFlatNoBound) {
            // B too large while k rows lie strictly below it
            for (;;) {
                const uint32_t at = hs_u(cum[B]);
                if (B == 0 || cnt_le - (long long)at < k) break;
                cnt_le -= at;
                B--;
            }
        }
    }
    return run;
}

// One wave: heap_heapify, then `if (dis < simi[0]) { heap_pop; heap_push }` over the tot candidates cq (payload, dis) in
// segment order -- the admitted lanes of every 64 in stream order, as k_bin_scan takes them -- then heap_reorder.  The
// heap (hK: k + 2 entries in LDS) holds the result best first in hK[1 .. k], an empty slot's payload is 0xffffffff;
// returns the admissions.
__device__ __forceinline__ unsigned long long bin_replay_segment(const uint2* __restrict__ cq, int64_t tot, int k,
                                                                 uint2* hK) {
    const int lane = threadIdx.x;
    const bool reg_heap = k <= 15;
    const bool par_heap = !reg_heap && k <= kParHeapMaxK;
    __syncthreads();
    heap_fill(hK, k, lane, 64);   // heap_heapify<CMax<int32_t, idx_t>>
    __syncthreads();
    RegHeap<1> rh;
    rh.fill();
    float top = kHeapFltMax;
    unsigned long long nadm = 0;
    for (int64_t j0 = 0; j0 < tot; j0 += 64) {
        const int64_t j = j0 + lane;
        uint2 e = make_uint2(0u, 0u);
        if (j < tot) e = cq[j];
        const float dv = j < tot ? (float)e.y : INFINITY;
        // `if (dis < simi[0]) { heap_pop; heap_push }`, the admitted lanes in stream order
        unsigned long long m = __ballot(top > dv);
        while (m) {
            const int sl = (int)__ffsll((long long)m) - 1;
            const float val = hw_readlane_f(dv, sl);
            const unsigned pay = (unsigned)hw_readlane_i((int)e.x, sl);
            if (reg_heap) {
                rh.pop(k);
                rh.push(k, val, pay);
                top = rh.top();
            } else if (par_heap) {
                const float root = par_heap_pop(hK, k);
                top = par_heap_push(hK, k, val, pay) ? val : root;
            } else {
                heap_pop_seq(hK, k);
                heap_push_seq(hK, k, val, pay);
                top = hs_f(hK[1].x);
            }
            nadm++;
            const unsigned long long above = sl >= 63 ? 0ull : (~0ull << (sl + 1));
            m = __ballot(top > dv) & above;
        }
    }
    // heap_reorder
    if (reg_heap) {
        const int real = rh.reorder_pops(k);
        rh.dump(hK, k);
        __syncthreads();
        heap_reorder_tail(hK, k, real);
    } else {
        __syncthreads();
        par_heap_reorder(hK, k);
    }
    __syncthreads();
    return nadm;
}

}  // namespace gh
