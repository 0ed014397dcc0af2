// pq4.hip -- the kernels of a 4-bit IVFPQ index (gamma_hip_ivfpq4_init): ksub = 16, sub-quantizer m in bits [4m, 4m + 4) of
// the code (faiss:impl/ProductQuantizer-inl.h:10-44, PQEncoderGeneric / PQDecoderGeneric with nbits = 4; the reference's
// scanner is templated over that decoder, index/impl/gamma_index_ivfpq.h:540-601).  Query tables, the precomputed table,
// the encoder and the list scan; everything behind the scan (selection, tie flags, re-rank, tie replay) is the 8-bit code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device_math.h"
#include "filter_dev.h"
#include "kernels.h"
#include "pq4.h"

namespace gh {

// ------------------------------------------------------------------------------------
// per-query inner-product table  out[q][m][j] = <x_q,m , c_mj>, j < 16
// (ProductQuantizer::compute_inner_prod_table, faiss:impl/ProductQuantizer.cpp:518-531: fvec_inner_products_ny per
// sub-quantizer -- the arithmetic of k_pq_ip_table).  A workgroup = 16 sub-quantizers x 16 centroids, PQ4_QB queries.
// ------------------------------------------------------------------------------------
constexpr int PQ4_QB = 8;
__global__ __launch_bounds__(256) void k_pq4_ip_table(const float* __restrict__ x, int nq, int d, int M, int dsub,
                                                      const float* __restrict__ pqc, float* __restrict__ out) {
    const int m = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    if (m >= M) return;
    const float* c = pqc + ((int64_t)m * 16 + j) * dsub;
    const int q0 = blockIdx.y * PQ4_QB;
    for (int u = 0; u < PQ4_QB; u++) {
        const int q = q0 + u;
        if (q >= nq) break;   // uniform
        const float* xs = x + (int64_t)q * d + m * dsub;
        out[((int64_t)q * M + m) * 16 + j] = fvec_ny_row<false>(xs, c, dsub);
    }
}
void launch_pq4_ip_table(hipStream_t s, const float* x, int nq, int d, int M, const float* pqc, float* out) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_pq4_ip_table, dim3((M + 15) / 16, (nq + PQ4_QB - 1) / PQ4_QB), dim3(256), 0, s, x, nq, d, M, d / M,
                       pqc, out);
}

// precomputed table T2[l][m][j] = ||c_mj||^2 + 2 <centroid_l,m , c_mj>
// (faiss:IndexIVFPQ.cpp:453-479: r_norms via fvec_norm_L2sqr, fvec_madd with bf = 2 -- k_precompute_table with 16 columns)
__global__ __launch_bounds__(256) void k_pq4_precompute_table(const float* __restrict__ cc, int d, int M, int dsub,
                                                              const float* __restrict__ pqc, float* __restrict__ out) {
    const int m = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15, l = blockIdx.y;
    if (m >= M) return;
    const float* xs = cc + (int64_t)l * d + m * dsub;
    const float* c = pqc + ((int64_t)m * 16 + j) * dsub;
    const float ip = fvec_ny_row<false>(xs, c, dsub);
    const float rn = fvec_norm_L2sqr(c, dsub);
    out[((int64_t)l * M + m) * 16 + j] = __builtin_fmaf(2.0f, ip, rn);
}
void launch_pq4_precompute_table(hipStream_t s, const float* cc, int nlist, int d, int M, const float* pqc, float* out) {
    if (nlist <= 0) return;
    hipLaunchKernelGGL(k_pq4_precompute_table, dim3((M + 15) / 16, nlist), dim3(256), 0, s, cc, d, M, d / M, pqc, out);
}

// ------------------------------------------------------------------------------------
// Add / Update / encode: residual + PQ encode of one vector per workgroup.
//   idx[m] = argmin_j fvec_L2sqr_ny(residual_m, c_mj), j < 16 (strict <, first minimum, mindis starts at 1e20,
//   faiss:impl/ProductQuantizer.cpp:321-348); byte t = idx[2t] | idx[2t + 1] << 4, an odd M leaves the last high nibble 0
//   (PQEncoderGeneric, faiss:impl/ProductQuantizer-inl.h:10-44).
// 16 lanes per sub-quantizer, 16 sub-quantizers per pass.  LDS: the residual (d floats, dynamic).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pq4_encode(const float* __restrict__ x, int d, int M, int dsub, int cs,
                                                    const int* __restrict__ assign, const float* __restrict__ cc,
                                                    const float* __restrict__ pqc, uint8_t* __restrict__ codes) {
    extern __shared__ float s_res4[];   // [d]
    __shared__ uint8_t s_idx[2 * kPq4MaxCodeSize];
    const int64_t i = blockIdx.x;
    const int l = assign[i];
    for (int t = threadIdx.x; t < d; t += 256) {
        const float xv = x[i * d + t];
        s_res4[t] = l < 0 ? 0.f : xv - cc[(int64_t)l * d + t];
    }
    if (threadIdx.x < 2 * kPq4MaxCodeSize) s_idx[threadIdx.x] = 0;
    __syncthreads();
    const int j = threadIdx.x & 15;
    for (int m0 = 0; m0 < M; m0 += 16) {   // uniform trip count: the shuffles below take whole waves
        const int m = m0 + (threadIdx.x >> 4);
        unsigned long long item = ~0ull;
        if (m < M) {
            float dis = fvec_ny_row<true>(s_res4 + m * dsub, pqc + ((int64_t)m * 16 + j) * dsub, dsub);
            if (!(dis < 1e20f)) dis = INFINITY;   // the reference never picks dis >= 1e20 (mindis init)
            item = ((unsigned long long)f2key(dis) << 32) | (unsigned)j;   // first-index tie rule: min over (key, j)
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(item, off, 16);
            if (o < item) item = o;
        }
        if (m < M && j == 0) {
            int best = (int)(uint32_t)item;
            if (key2f((uint32_t)(item >> 32)) == INFINITY) best = 0;   // idxm's initial value
            s_idx[m] = (uint8_t)best;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < cs)
        codes[i * cs + threadIdx.x] = (uint8_t)(s_idx[2 * threadIdx.x] | (s_idx[2 * threadIdx.x + 1] << 4));
}
void launch_pq4_encode(hipStream_t s, const float* x, int64_t n, int d, int M, const int* assign, const float* cc,
                       const float* pqc, uint8_t* codes) {
    if (n <= 0) return;
    if (M > 2 * kPq4MaxCodeSize || (size_t)d * sizeof(float) > (48u << 10)) {
        launch_refused("launch_pq4_encode: more than 128 sub-quantizers or a residual beyond 48 KB of LDS");
        return;
    }
    hipLaunchKernelGGL(k_pq4_encode, dim3((unsigned)n), dim3(256), (size_t)d * sizeof(float), s, x, d, M, d / M,
                       pq4_code_size(M), assign, cc, pqc, codes);
}

// ------------------------------------------------------------------------------------
// The list scan.  One workgroup per (query, group of G consecutive probes), placed like the plain path of
// k_ivfpq_scan_pair (block b runs on XCD b % 8: a query's groups share an XCD and its L2; with qperm the XCD takes a
// contiguous eighth of the spatial query order).
//   LUT (M x 16 fp32, at most 8 KB of LDS):  L2: lut = T2[list] + (-2) * st2[q]  (fvec_madd)   IP: lut = st2[q]
//   per code j: skip if ids[j] bit 63 / !IsValid;  dis = dis0; for m ascending: dis += lut[m][nibble_m]
//   (sequential fp32 adds -- two nibbles are NOT paired into a 256-entry table: (dis + a) + b is not dis + (a + b)).
// MT > 0: M at compile time and a code of 4, 8, 16 or 32 bytes, read as dword / dwordx2 / dwordx4 loads, one code per lane
// and step.  The NEXT step's code words are requested before this step's gathers, so that the memory latency runs beside
// the LDS work instead of in front of it; the first step's words are requested before the list's table is built.
// MT == 0: any M (an odd M, a code size that is no multiple of 4): byte loads.
// ------------------------------------------------------------------------------------
template <int NW>
__device__ __forceinline__ void pq4_load_code(const uint8_t* __restrict__ p, uint32_t (&w)[NW]) {
    if constexpr (NW == 1) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if constexpr (NW == 2) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x;
        w[1] = v.y;
    } else {
#pragma unroll
        for (int u = 0; u < NW / 4; u++) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[u];
            w[4 * u] = v.x;
            w[4 * u + 1] = v.y;
            w[4 * u + 2] = v.z;
            w[4 * u + 3] = v.w;
        }
    }
}

template <bool L2, int MT>
__global__ __launch_bounds__(256) void k_ivfpq4_scan_pair(
        int nq, int M, int P, int G, const int* __restrict__ probe_list, const float* __restrict__ pair_dis0,
        const float* __restrict__ st2, const float* __restrict__ T2, const int64_t* __restrict__ list_off,
        const int* __restrict__ list_len, const uint8_t* __restrict__ list_mask, int nlist,
        const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids, const int* __restrict__ pair_off,
        int64_t q_stride, float* __restrict__ out, const FilterDesc* __restrict__ ftab, const int* __restrict__ qfil,
        int need_ids, float sentinel, const int* __restrict__ qperm, int pg_cnt) {
    extern __shared__ float s_lut4[];   // [M][16]: all of the kernel's LDS, so a gather address is (nibble << 2) + an immediate
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int pg = slot % pg_cnt, qslot = slot / pg_cnt;
    int q;
    if (qperm) {
        const int qi = xcd * ((nq + 7) >> 3) + qslot;
        if (qi >= nq) return;
        q = qperm[qi];
    } else {
        q = qslot * 8 + xcd;
        if (q >= nq) return;
    }
    const FilterDesc& filt = ftab[(need_ids && qfil) ? qfil[q] : 0];
    const int tid = threadIdx.x;
    const int Mr = MT > 0 ? MT : M;
    const int msz = Mr * 16, cs = (Mr + 1) >> 1;
    constexpr int NE = MT > 0 ? (MT * 16 + 255) / 256 : 1;   // table entries per thread
    constexpr int NW = MT > 0 ? MT / 8 : 1;                  // code words per code
    const float* st2q = st2 + (int64_t)q * msz;
    float s2r[NE];
    if constexpr (MT > 0) {
#pragma unroll
        for (int i = 0; i < NE; i++) s2r[i] = (tid + 256 * i < msz) ? st2q[tid + 256 * i] : 0.f;
    }
    if (!L2) {   // inner product: the table is the query's, whatever the list
        if constexpr (MT > 0) {
#pragma unroll
            for (int i = 0; i < NE; i++)
                if (tid + 256 * i < msz) s_lut4[tid + 256 * i] = s2r[i];
        } else {
            for (int e = tid; e < msz; e += 256) s_lut4[e] = st2q[e];
        }
        __syncthreads();
    }
    const int p_begin = pg * G, p_end = min(P, p_begin + G);
    for (int p = p_begin; p < p_end; p++) {
        const int pair = q * P + p;
        const int l = probe_list[pair];
        if (l < 0 || l >= nlist) continue;   // uniform
        if (list_mask && !list_mask[l]) continue;
        const int len = list_len[l];
        if (len <= 0) continue;
        const int64_t off = list_off[l];
        const uint8_t* lc = codes + off * cs;
        uint32_t cur[NW];
        if constexpr (MT > 0) pq4_load_code<NW>(lc + (int64_t)min(tid, len - 1) * cs, cur);
        if (L2) {
            __syncthreads();   // the previous list's gathers are finished
            const float* t2 = T2 + (int64_t)l * msz;
            if constexpr (MT > 0) {
#pragma unroll
                for (int i = 0; i < NE; i++)
                    if (tid + 256 * i < msz) s_lut4[tid + 256 * i] = __builtin_fmaf(-2.0f, s2r[i], t2[tid + 256 * i]);
            } else {
                for (int e = tid; e < msz; e += 256) s_lut4[e] = __builtin_fmaf(-2.0f, st2q[e], t2[e]);
            }
            __syncthreads();
        }
        const float dis0 = pair_dis0[pair];
        const int64_t* lid = ids + off;
        float* o = out + (int64_t)q * q_stride + pair_off[(int64_t)q * (P + 1) + p];
        // Two copies of the loop, with and without the validity predicates: their loads (ids, and flat loads through the filter
        // table's pointers) make the compiler wait for EVERY outstanding load at the join behind them -- the next step's
        // codes included, so the prefetch would never overlap the gathers.  The common call rejects nothing and takes the
        // copy without them.
        auto scan_list = [&](auto ids_tag) {
            constexpr bool IDS = decltype(ids_tag)::value;
            for (int j0 = 0; j0 < len; j0 += 256) {
                const int j = j0 + tid;
                const bool more = j0 + 256 < len;   // uniform
                uint32_t nxt[NW];
                if constexpr (MT > 0) {
                    if (more) pq4_load_code<NW>(lc + (int64_t)min(j + 256, len - 1) * cs, nxt);
                }
                if (j < len) {
                    // ids are read only when something can reject an entry (delete bit, filter, superseded slot)
                    bool ok = true;
                    if constexpr (IDS) {
                        const int64_t id = lid[j];
                        ok = id >= 0;   // bit 63 = kDelIdxMask (realtime_mem_data.h:26)
                        if (ok) ok = is_valid_doc(filt, id);
                    }
                    float dis = dis0;
                    if constexpr (MT > 0) {
                        float t[MT];
#pragma unroll
                        for (int m = 0; m < MT; m++) t[m] = s_lut4[m * 16 + ((cur[m >> 3] >> (4 * (m & 7))) & 15u)];
                        __builtin_amdgcn_sched_barrier(0);   // all gathers in flight before the add chain
#pragma unroll
                        for (int m = 0; m < MT; m++) dis += t[m];   // sequential, reference order
                    } else {
                        const uint8_t* cj = lc + (int64_t)j * cs;
                        for (int m = 0; m < Mr; m++) {
                            const uint32_t b = cj[m >> 1];
                            dis += s_lut4[m * 16 + ((m & 1) ? (b >> 4) : (b & 15u))];
                        }
                    }
                    o[j] = ok ? dis : sentinel;
                }
                if constexpr (MT > 0) {
                    if (more) {
#pragma unroll
                        for (int u = 0; u < NW; u++) cur[u] = nxt[u];
                    }
                }
            }
        };
        if (need_ids) scan_list(std::true_type{});
        else scan_list(std::false_type{});
    }
}

void launch_ivfpq4_scan_pair(hipStream_t s, bool l2, int nq, int M, int P, const int* probe_list, const float* dis0,
                             const float* st2, const float* T2, const int64_t* list_off, const int* list_len,
                             const uint8_t* list_mask, int nlist, const uint8_t* codes, const int64_t* ids,
                             const int* pair_off, int64_t q_stride, float* out, const FilterDesc* ftab, const int* qfil,
                             int need_ids, const int* qperm, int G, int pg_cnt) {
    if (nq <= 0 || pg_cnt <= 0) return;
    if (M <= 0 || M > 2 * kPq4MaxCodeSize || G <= 0 || (int64_t)pg_cnt * G < P || (l2 && !T2)) {
        launch_refused("launch_ivfpq4_scan_pair: M beyond 128, probe groups that do not cover nprobe, or L2 without a table");
        return;
    }
    const size_t lds = (size_t)M * 16 * sizeof(float);
    const dim3 grid((unsigned)(8 * (int64_t)((nq + 7) / 8) * pg_cnt));
#define GH_PQ4(LL, MT)                                                                                                   \
    hipLaunchKernelGGL((k_ivfpq4_scan_pair<LL, MT>), grid, dim3(256), lds, s, nq, M, P, G, probe_list, dis0, st2, T2,      \
                       list_off, list_len, list_mask, nlist, codes, ids, pair_off, q_stride, out, ftab, qfil, need_ids,  \
                       LL ? INFINITY : -INFINITY, qperm, pg_cnt)
#define GH_PQ4_M(LL)                    \
    do {                                \
        if (M == 32) GH_PQ4(LL, 32);    \
        else if (M == 16) GH_PQ4(LL, 16); \
        else if (M == 64) GH_PQ4(LL, 64); \
        else if (M == 8) GH_PQ4(LL, 8); \
        else GH_PQ4(LL, 0);             \
    } while (0)
    if (l2) GH_PQ4_M(true);
    else GH_PQ4_M(false);
#undef GH_PQ4_M
#undef GH_PQ4
}

}  // namespace gh
