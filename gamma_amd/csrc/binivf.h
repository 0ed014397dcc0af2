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
// ---- the chain's two heavy passes list-major, for large batches (binivf_lm.hip) ----
// queries of one work unit: a unit is (a kBinSpreadChunk-row chunk of a LIST) x (a tile of the queries that probe the list)
constexpr int kBinLmQueryTile = 32;
// the smallest call gamma_hip_binivf_set_lm_scan(on, 0) sends list-major.  Measured at workload B1: no
// size at which the path is faster at both k = 10 and k = 100; 16384 is the one size beyond the spread chain's range at
// which it was faster at k = 10.  The switch is an opt-in.
constexpr int kBinLmAutoMinNq = 16384;
// what the unit count of a call cannot exceed: every probed list has at most one ragged tile
int64_t bin_lm_unit_bound(int nq, int P, int nlist, int max_list_len);
// bytes of the chain's tables (bin_spread_meta_bytes) with the per-(query, probe) chunk base behind them
size_t bin_lm_meta_bytes(int nq, int P, int maxch);
// bytes of the call's inverse index: the (query, probe) pairs of every list, the lists' counts, starts and unit prefix
size_t bin_lm_inv_bytes(int nq, int P, int nlist);
// launch_bin_spread's answer with k_bin_sp_hist / k_bin_sp_collect replaced by k_bin_lm_hist / k_bin_lm_collect over
// the call's inverse index; the table, bounds and replay kernels are the chain's.  meta: bin_lm_meta_bytes, inv:
// bin_lm_inv_bytes, the rest as launch_bin_spread.  No limit on nq.  lm_stats (may be null): += {queries, chunks,
// candidates, units}.  stage: 0 all, 1 inverse index + table + histograms + bounds, 2 collect, 3 replay
void launch_bin_lm(hipStream_t s, const uint8_t* x, int nq, int64_t xs, int cs, const int* probe, int P, int nlist,
                   int max_list_len, const int64_t* list_off, const int* list_len, const uint8_t* codes, const int64_t* ids,
                   const FilterDesc* ftab, int need_filter, float min_score, float max_score, int k, int maxch,
                   int64_t stride, uint32_t* hist, void* meta, void* inv, uint2* cand, float* D, int64_t* I,
                   unsigned long long* stats, unsigned long long* lm_stats, int stage);
// the chain's kernels launch_bin_lm launches as launch_bin_spread does (binivf_spread.hip)
__global__ void k_bin_sp_table(const int* __restrict__ probe, int nq, int P, const int* __restrict__ list_len, int maxch,
                               int2* __restrict__ cmap, int* __restrict__ nchq);
__global__ void k_bin_sp_bounds(const uint32_t* __restrict__ hist, int nq, const int* __restrict__ nchq, int maxch, int nb,
                                int k, int* __restrict__ bound, uint32_t* __restrict__ off, uint32_t* __restrict__ total);
__global__ void k_bin_sp_replay(const uint2* __restrict__ cand, int64_t stride, const uint32_t* __restrict__ total,
                                const int* __restrict__ nchq, int nq, int k, const int64_t* __restrict__ ids,
                                float* __restrict__ D, int64_t* __restrict__ I, unsigned long long* __restrict__ stats,
                                unsigned long long* __restrict__ sp_stats);
// the counting sort of a call's (query, probe) pairs by list (ivfflat.hip), as launch_bin_lm runs it: cnt zeroed ->
// k_inv_count -> k_inv_scan_b (units of kBinLmQueryTile queries x kBinSpreadChunk rows) -> k_inv_fill
__global__ void k_inv_count(const int* __restrict__ probe, int npairs, int nlist, const int* __restrict__ list_len,
                            int* __restrict__ cnt);
__global__ void k_inv_scan_b(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist, int* __restrict__ start,
                             int* __restrict__ cur, int* __restrict__ ustart);
__global__ void k_inv_fill(const int* __restrict__ probe, int npairs, int nlist, const int* __restrict__ list_len,
                           const int* __restrict__ start, int* __restrict__ cur, int* __restrict__ inv);
// binary_to_real (faiss:utils/utils.cpp:634-638): n codes of d bits -> n x d floats of +-1
void launch_bin_decode(hipStream_t s, const uint8_t* codes, int64_t n, int d, float* out);

}  // namespace gh
