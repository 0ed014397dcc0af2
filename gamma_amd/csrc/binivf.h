// binivf.h -- launchers of the binary IVF kernels (binivf.hip); index/impl/gamma_index_binary_ivf.{h,cc}.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gh {

// largest k of the scan's LDS heap ((k + 2) x 8 bytes) and largest nprobe of the coarse step's heap
constexpr int kBinMaxK = 4096;
constexpr int kBinMaxProbe = 4096;
// largest code: 2048 bits (the query's words sit in LDS)
constexpr int kBinMaxCodeSize = 256;

// IndexBinaryFlat::search (faiss:IndexBinaryFlat.cpp:33-59, utils/hamming.cpp:230-265) of nq queries (row stride xs bytes)
// against nlist centroid codes: probe [nq][P] = centroid ids best first (-1 padded), pdis (may be null) = their Hamming
// distances (INT32_MAX padded)
void launch_bin_coarse(hipStream_t s, const uint8_t* x, int nq, int64_t xs, const uint8_t* cc, int nlist, int cs, int P,
                       int* probe, int* pdis);
// search_knn_hamming_heap + GammaIVFBinaryScannerL2::scan_codes (gamma_index_binary_ivf.cc:333-448) of every query over
// its P probes; D / I [nq][k]; stats (may be null): += {queries, heap admissions}
void launch_bin_scan(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P,
                     const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                     const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, float* D, int64_t* I,
                     unsigned long long* stats);
// ---- the scan of one query spread over the device (binivf_spread.hip) ----
// rows per chunk (a chunk never spans two lists): the unit of the histograms, of the bounds B_c and of the workgroups
constexpr int kBinSpreadChunk = 1024;
// queries of one spread call (the grid's y extent)
constexpr int kBinSpreadMaxNq = 65535;
// the largest call the automatic scan mode spreads (measured at workload B1)
constexpr int kBinSpreadAutoMaxNq = 1024;
// what no query of a call can exceed, from the longest list of the version the call reads: *maxch chunks, *rows rows
void bin_spread_bounds(int P, int nlist, int max_list_len, int* maxch, int64_t* rows);
// bytes of the chain's per-(query, chunk) tables
size_t bin_spread_meta_bytes(int nq, int maxch);
// launch_bin_scan's answer (D, I, stats) by the chain chunk table -> histograms -> bounds -> collect -> replay, enqueued
// on s, nothing read back.  hist: nq x maxch x (8 cs + 1) counters, meta: bin_spread_meta_bytes, cand: nq x stride
// (position, distance) pairs, stride = *rows of bin_spread_bounds.  sp_stats (may be null): += {queries, chunks,
// candidates}.  stage: 0 the whole chain, 1 table + histograms + bounds, 2 collect, 3 replay (for the stage timers)
void launch_bin_spread(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P,
                       const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                       const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, int maxch,
                       int64_t stride, uint32_t* hist, void* meta, uint2* cand, float* D, int64_t* I,
                       unsigned long long* stats, unsigned long long* sp_stats, int stage);
// binary_to_real (faiss:utils/utils.cpp:634-638): n codes of d bits -> n x d floats of +-1
void launch_bin_decode(hipStream_t s, const uint8_t* codes, int64_t n, int d, float* out);

}  // namespace gh
