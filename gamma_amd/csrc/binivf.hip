// binivf.hip -- the binary IVF model (index/impl/gamma_index_binary_ivf.{h,cc} over faiss 1.7.1's IndexBinaryIVF):
// codes of d bits, Hamming distances (XOR + v_bcnt_u32_b32), the realtime lists of the other IVF models.
//
// Hamming distances are small integers, so nearly every query has a tie at its k-th place, and the reference's answer
// inside a tie is whatever its heap array holds after the whole candidate stream (faiss 1.7.1's heaps never break ties
// by id).  Both heaps are therefore REPLAYED, one wave per query, with the primitives of heap_dev.h:
//   * coarse step (hammings_knn_hc, faiss:utils/hamming.cpp:230-265): the centroids in index order through a heap of
//     nprobe entries, `dis < top -> heap_replace_top` (HeapWalk: 64 compared per ballot, the sifts pipelined), then
//     heap_reorder;
//   * scan (GammaIVFBinaryScannerL2::scan_codes, gamma_index_binary_ivf.cc:407-448): probes in coarse order, entries in
//     list order; a lane per entry computes IsValid, the distance and the score window; a ballot over `dis < top` finds
//     the entries the heap admits, which are then taken in lane order with heap_pop + heap_push (in registers up to 15
//     entries, all-lane sifts up to 256, sequential beyond), then heap_reorder.
// The distances are integers <= 2048, exact as floats, so the float heaps order them as the int32 heaps do; the empty
// slots' INT32_MAX and the float heaps' FLT_MAX both lose against every real distance.
// Workgroups are one wave: every LDS hand-over between lanes is a __syncthreads of a single wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bin_dev.h"
#include "binivf.h"
#include "filter_dev.h"
#include "heap_dev.h"

namespace gh {

// one wave per query (grid-stride); the centroid codes in LDS when cc_lds
template <bool AL>
__global__ __launch_bounds__(64) void k_bin_coarse(const uint8_t* __restrict__ x, int nq, int64_t xs,
                                                   const uint8_t* __restrict__ cc, int nlist, int cs, int P, int cc_lds,
                                                   int* __restrict__ probe, int* __restrict__ pdis) {
    extern __shared__ __align__(16) char smem[];
    const int lane = threadIdx.x, nw = (cs + 3) >> 2;
    const size_t ccb = cc_lds ? bin_align16((size_t)nlist * cs) : 0;
    uint2* heap = reinterpret_cast<uint2*>(smem + ccb);
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem + ccb + bin_align16((size_t)(P + 2) * 8));
    const uint8_t* cb = cc;
    if (cc_lds) {
        const int64_t nb = (int64_t)nlist * cs;
        if (AL) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(cc);
            uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
            for (int64_t i = lane; i < (nb >> 2); i += 64) dst[i] = src[i];
        } else {
            for (int64_t i = lane; i < nb; i += 64) smem[i] = (char)cc[i];
        }
        cb = reinterpret_cast<const uint8_t*>(smem);
    }
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        __syncthreads();   // the previous query's heap and words have been read
        bin_load_query(x + (int64_t)q * xs, cs, nw, qw);
        heap_fill(heap, P, lane, 64);
        __syncthreads();
        HeapWalk w;
        w.begin(heap, P);
        for (int j0 = 0; j0 < nlist; j0 += 64) {
            const int j = j0 + lane;
            const int dis = j < nlist ? bin_hamming<AL>(qw, cb + (int64_t)j * cs, cs, nw) : 0;
            w.accept(j < nlist, (float)dis, j);   // `if (dis < bh_val[0]) maxheap_replace_top`
        }
        w.drain();
        __syncthreads();
        par_heap_reorder(heap, P);
        __syncthreads();
        for (int i = lane; i < P; i += 64) {
            const uint2 e = heap[1 + i];
            const bool empty = e.y == 0xffffffffu;
            probe[(int64_t)q * P + i] = empty ? -1 : (int)e.y;
            if (pdis) pdis[(int64_t)q * P + i] = empty ? 2147483647 : (int)__uint_as_float(e.x);
        }
    }
}

// one wave per query (grid-stride); the k-heap in LDS (or registers), payload = arena position of the entry
template <bool AL>
__global__ __launch_bounds__(64) void k_bin_scan(const uint8_t* __restrict__ x, int nq, int64_t xs, int cs,
                                                 const int* __restrict__ probe, int P, const int64_t* __restrict__ list_off,
                                                 const int* __restrict__ list_len, const uint8_t* __restrict__ codes,
                                                 const int64_t* __restrict__ ids, const FilterDesc* __restrict__ ftab,
                                                 int need_filter, float min_score, float max_score, int k,
                                                 float* __restrict__ D, int64_t* __restrict__ I,
                                                 unsigned long long* __restrict__ stats) {
    extern __shared__ __align__(16) char smem[];
    const int lane = threadIdx.x, nw = (cs + 3) >> 2;
    uint2* hK = reinterpret_cast<uint2*>(smem);
    uint32_t* qw = reinterpret_cast<uint32_t*>(smem + bin_align16((size_t)(k + 2) * 8));
    const bool reg_heap = k <= 15;
    const bool par_heap = !reg_heap && k <= kParHeapMaxK;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        __syncthreads();
        bin_load_query(x + (int64_t)q * xs, cs, nw, qw);
        heap_fill(hK, k, lane, 64);   // heap_heapify<CMax<int32_t, idx_t>>
        __syncthreads();
        RegHeap<1> rh;
        rh.fill();
        float top = kHeapFltMax;
        unsigned long long nadm = 0;
        for (int p = 0; p < P; p++) {
            const int l = probe[(int64_t)q * P + p];
            if (l < 0) continue;   // not enough centroids for multiprobe
            const int len = list_len[l];
            const int64_t base = list_off[l];
            for (int j0 = 0; j0 < len; j0 += 64) {
                const int j = j0 + lane;
                const int64_t pos = base + j;
                bool ok = j < len;
                const int64_t id = ok ? ids[pos] : -1;
                ok = ok && id >= 0;
                if (ok && need_filter) ok = is_valid_doc(ftab[0], id);   // IsValid
                float dv = INFINITY;
                if (ok) {
                    const float dis = (float)bin_hamming<AL>(qw, codes + pos * cs, cs, nw);
                    if (dis <= max_score && dis >= min_score) dv = dis;   // IsSimilarScoreValid
                }
                // `if (dis < simi[0]) { heap_pop; heap_push }`, the admitted lanes in stream order
                unsigned long long m = __ballot(top > dv);
                while (m) {
                    const int sl = (int)__ffsll((long long)m) - 1;
                    const float val = hw_readlane_f(dv, sl);
                    const unsigned pay = (unsigned)hw_readlane_i((int)pos, sl);
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
        for (int i = lane; i < k; i += 64) {
            const uint2 e = hK[1 + i];
            const bool empty = e.y == 0xffffffffu;
            D[(int64_t)q * k + i] = empty ? 2147483648.f : __uint_as_float(e.x);   // (float)INT32_MAX
            I[(int64_t)q * k + i] = empty ? -1 : ids[e.y];
        }
        if (stats && lane == 0) {
            atomicAdd(stats, 1ull);
            atomicAdd(stats + 1, nadm);
        }
    }
}

__global__ __launch_bounds__(256) void k_bin_decode(const uint8_t* __restrict__ codes, int64_t n, int d,
                                                    float* __restrict__ out) {
    const int64_t tot = n * d;
    const int cs = d >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / d;
        const int b = (int)(i - r * d);
        out[i] = ((codes[r * cs + (b >> 3)] >> (b & 7)) & 1) ? 1.f : -1.f;   // 2 * bit - 1
    }
}

namespace {
constexpr size_t kBinCoarseLdsCap = 64 * 1024;   // centroids + heap + query: two workgroups' worth per CU at most
size_t coarse_lds(int nlist, int cs, int P, bool cc_lds) {
    const size_t a = ((size_t)(P + 2) * 8 + 15) & ~(size_t)15;
    return (cc_lds ? (((size_t)nlist * cs + 15) & ~(size_t)15) : 0) + a + (size_t)kBinMaxCodeSize;
}
}  // namespace

void launch_bin_coarse(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* cc, int nlist, int cs, int P,
                       int* probe, int* pdis) {
    if (nq <= 0 || P <= 0) return;
    if (P > kBinMaxProbe || cs <= 0 || cs > kBinMaxCodeSize) return launch_refused("bin_coarse: nprobe / code size");
    const bool al = (cs & 3) == 0;
    const bool cc_lds = coarse_lds(nlist, cs, P, true) <= kBinCoarseLdsCap;
    const size_t lds = coarse_lds(nlist, cs, P, cc_lds);
    // with the centroids in LDS a workgroup takes several queries (their copy is amortised)
    const int grid = std::max(1, std::min(nq, cc_lds ? 256 * 8 : 65535));
    if (al)
        hipLaunchKernelGGL(k_bin_coarse<true>, dim3(grid), dim3(64), lds, s, x, nq, xs, cc, nlist, cs, P, cc_lds ? 1 : 0,
                           probe, pdis);
    else
        hipLaunchKernelGGL(k_bin_coarse<false>, dim3(grid), dim3(64), lds, s, x, nq, xs, cc, nlist, cs, P, cc_lds ? 1 : 0,
                           probe, pdis);
}

void launch_bin_scan(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P,
                     const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                     const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, float* D, int64_t* I,
                     unsigned long long* stats) {
    if (nq <= 0 || k <= 0) return;
    if (k > kBinMaxK || cs <= 0 || cs > kBinMaxCodeSize) return launch_refused("bin_scan: k / code size");
    const size_t lds = (((size_t)(k + 2) * 8 + 15) & ~(size_t)15) + (size_t)kBinMaxCodeSize;
    const int grid = std::max(1, std::min(nq, 65535));
    if ((cs & 3) == 0)
        hipLaunchKernelGGL(k_bin_scan<true>, dim3(grid), dim3(64), lds, s, x, nq, xs, cs, probe, P, list_off, list_len, codes,
                           ids, ftab, need_filter, min_score, max_score, k, D, I, stats);
    else
        hipLaunchKernelGGL(k_bin_scan<false>, dim3(grid), dim3(64), lds, s, x, nq, xs, cs, probe, P, list_off, list_len, codes,
                           ids, ftab, need_filter, min_score, max_score, k, D, I, stats);
}

void launch_bin_decode(hipStream_t s, const uint8_t* codes, int64_t n, int d, float* out) {
    if (n <= 0) return;
    const int64_t tot = n * d;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((tot + 255) / 256, 8192));
    hipLaunchKernelGGL(k_bin_decode, dim3(grid), dim3(256), 0, s, codes, n, d, out);
}

}  // namespace gh
