// binflat.h -- launchers of the exact Hamming (binary flat) search kernels (binflat.hip): faiss:IndexBinaryFlat.cpp /
// utils/hamming.cpp:230-265 over every stored code, answered as GammaIVFBinaryScannerL2::scan_codes
// (gamma_index_binary_ivf.cc:333-448) answers ONE list that holds every code in vid order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "binivf.h"
#include "kernels.h"

namespace gh {

// rows per chunk: the unit of the histograms, of the bounds B_c and of the candidate segments
constexpr int kBinFlatChunk = 4096;
// "fewer than k valid rows so far": every valid row of the chunk is a candidate
constexpr int kBinFlatNoBound = 2147483647;

// queries per tile of k_binflat_hist / k_binflat_collect for a call of nq queries over codes of cs bytes (1, 4 or 8: the
// (nbits + 1) counters per query of the tile have to fit the workgroup's LDS)
int binflat_query_tile(int nq, int cs);

// hist [nq][nch][nbits + 1]: how many valid rows of chunk c inside the score window lie at every distance of query q
void launch_binflat_hist(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* codes, int64_t n, int cs,
                         const FilterDesc* ftab, int need_filter, float min_score, float max_score, uint32_t* hist);
// per query the running sum of its chunk histograms: bound [nq][nch] = the k-th smallest valid distance of the rows before
// chunk c (kBinFlatNoBound while fewer than k), off [nq][nch] = candidates (rows with dis < bound) of the chunks before c,
// total [nq] = candidates of the query
void launch_binflat_bounds(hipStream_t s, const uint32_t* hist, int nq, int64_t n, int cs, int k, int* bound, uint32_t* off,
                           uint32_t* total);
// cand [base[q] + off[q][c] ..): the chunk's rows with dis < bound[q][c] as (vid, dis), in vid order
void launch_binflat_collect(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* codes, int64_t n, int cs,
                            const FilterDesc* ftab, int need_filter, float min_score, float max_score, const int* bound,
                            const uint32_t* off, const uint32_t* total, const int64_t* base, uint2* cand);
// scan_codes' `dis < simi[0] -> heap_pop + heap_push` over every query's candidates, heap_reorder; D / I [nq][k];
// total == nullptr: no candidates at all (an empty store); stats += {queries, candidates, heap admissions}
void launch_binflat_replay(hipStream_t s, const uint2* cand, const int64_t* base, const uint32_t* total, int nq, int k,
                           float* D, int64_t* I, unsigned long long* stats);

}  // namespace gh
