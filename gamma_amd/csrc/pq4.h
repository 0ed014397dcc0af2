// pq4.h -- launchers of the 4-bit product-quantizer kernels (pq4.hip): ksub = 16, two sub-quantizer indices per code
// byte as faiss's PQEncoderGeneric packs them (faiss:impl/ProductQuantizer-inl.h:10-44).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gh {

constexpr int kPq4Ksub = 16;
constexpr int kPq4MaxCodeSize = 64;   // M <= 128: the scan's table (M x 16 fp32) is at most 8 KB of LDS
inline int pq4_code_size(int M) { return (4 * M + 7) / 8; }

// out[q][m][j] = <x_q,m , c_mj>, j < 16 (ProductQuantizer::compute_inner_prod_table, fvec_inner_products_ny order)
void launch_pq4_ip_table(hipStream_t s, const float* x, int nq, int d, int M, const float* pqc, float* out);
// T2[l][m][j] = ||c_mj||^2 + 2 <centroid_l,m , c_mj>, j < 16 (faiss:IndexIVFPQ.cpp:460-476)
void launch_pq4_precompute_table(hipStream_t s, const float* cc, int nlist, int d, int M, const float* pqc, float* out);
// residual to centroid assign[i] (none: assign < 0), per sub-quantizer the first strict minimum of fvec_L2sqr_ny over its 16
// centroids (faiss:impl/ProductQuantizer.cpp:321-348), nibbles packed into codes[i][code_size]
void launch_pq4_encode(hipStream_t s, const float* x, int64_t n, int d, int M, const int* assign, const float* cc,
                       const float* pqc, uint8_t* codes);
// the list scan of a 4-bit index: one workgroup per (query, group of G probes), every distance into the pair's slot range of
// the ADC slab, filtered entries as the sentinel (+inf L2 / -inf inner product) -- what the plain path of
// launch_ivfpq_scan_pair leaves for the selection, the tie flags and the tie replay.  st2 [nq][M][16] (launch_pq4_ip_table),
// T2 [nlist][M][16]; dis0 [nq][P]: the coarse distance (L2) or <x, centroid> (inner product).
void launch_ivfpq4_scan_pair(hipStream_t s, bool l2, int nq, int M, int P, const int* probe_list, const float* dis0,
                             const float* st2, const float* T2, const int64_t* list_off, const int* list_len,
                             const uint8_t* list_mask, int nlist, const uint8_t* codes, const int64_t* ids,
                             const int* pair_off, int64_t q_stride, float* out, const FilterDesc* ftab, const int* qfil,
                             int need_ids, const int* qperm, int G, int pg_cnt);

}  // namespace gh
