// pqwide_res.hip -- the L2 list scan of a wide 8-bit IVFPQ handle (pqwide.hip) that holds NO precomputed table: table mode 0,
// gamma_hip_ivfpq_wide_set_table_mode0.  faiss leaves use_precomputed_table at 0 where the table would
// exceed precomputed_table_max_bytes (faiss:IndexIVFPQ.cpp:441-449) and the reference's scanner then scores each (query, list)
// pair with the distance table of the residual (index/impl/gamma_index_ivfpq.h:239-245):
//     r = x_q - centroid_l                                                  (compute_residual: plain fp32 subtraction)
//     lut[m][j] = fvec_L2sqr_ny row of (r + m * dsub, codebook centroid (m, j))     (pq.compute_distance_table)
//     dis = 0;  for m ascending: dis += lut[m][code[m]]                     (sequential fp32 adds, nothing reassociated)
// k_ivfpq_scan_pair<RES> (scan.hip) is this for M <= 64 with the whole table in LDS.  Here the table goes through LDS in slices of
// MS sub-quantizers as in k_ivfpq_scan_wide, and the partial sums are carried in registers (a list of one tile) or parked in
// the code's own slab slot (longer lists): the argument at the head of pqwide.hip, no bit changes.
//
// What differs is the table.  A pair's table costs 256 * d subtract-and-fma steps and one pass over the whole codebook
// (256 * d * 4 bytes from L2: 768 KB at d = 768).  The pass can be shared: a workgroup owns one query and G of its probes,
// runs the slices outermost, and in a slice a thread
//   1. loads centroid (m, tid) into registers ONCE per row m (several rows requested together),
//   2. scores it against the G residual slices in LDS (every lane reads the same address: a broadcast),
//   3. writes the G table rows to LDS,
// then the G lists are scanned against their own table slices.  LDS: G * MS KB of tables + G * MS * dsub * 4 bytes of
// residuals; a shape beyond the 64 KB default is allowed for (the limit is raised per kernel).  Measured (DESIGN.md section
// 40): on lists of ~1000 codes the gathers dominate, not the build, and the workgroups a CU holds count for more than the
// shared pass -- (MS, G) = (32, 1), 32 KB + the residual slice, is the shape kept (kernels.h).  One workgroup per
// (query, group of G probes), placed like k_ivfpq_scan_wide (block b runs on XCD b % 8, qperm).  The slab is that of
// launch_ivfpq_scan_wide: same offsets, same sentinel, ids read only with need_ids.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "device_math.h"
#include "filter_dev.h"
#include "kernels.h"

namespace gh {

namespace {
// pqwide.hip's wide_each: the body once per i = 0 .. N - 1 with i a compile-time constant -- the per-list and per-code registers
// are never indexed by a loop variable
template <int N, int I = 0, class F>
__device__ __forceinline__ void res_each(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        res_each<N, I + 1>(f);
    }
}

// N consecutive floats into registers with the widest loads the row's alignment allows: a codebook row (m, j) and a residual
// row m start at a multiple of dsub floats
template <int N>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&r)[N]) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; i++) {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
        }
    } else if constexpr (N % 2 == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            const float2 v = reinterpret_cast<const float2*>(p)[i];
            r[2 * i] = v.x; r[2 * i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) r[i] = p[i];
    }
}
}  // namespace

// DSUB > 0: d / M at compile time -- centroid and residual rows in registers, fvec_ny_row unrolled over them.
// DSUB == 0: any other dsub <= 64 -- fvec_ny_row reads the centroid row through its pointer, once per list of the group.
// VEC: M is a multiple of MS (whole slices): a code's MS bytes of a slice are MS / 16 dwordx4 words.  !VEC: any M, byte loads.
template <int MS, int G, int DSUB, bool VEC, int U>
__global__ __launch_bounds__(256) void k_ivfpq_scan_wide_res(
        int nq, int d, int M, int P, const int* __restrict__ probe_list, const float* __restrict__ x,
        const float* __restrict__ cc, const float* __restrict__ pqc, const int64_t* __restrict__ list_off,
        const int* __restrict__ list_len, const uint8_t* __restrict__ list_mask, int nlist,
        const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids, const int* __restrict__ pair_off,
        int64_t q_stride, float* out, const FilterDesc* __restrict__ ftab, const int* __restrict__ qfil, int need_ids,
        float sentinel, const int* __restrict__ qperm, int pg_cnt) {
    extern __shared__ float4 s_resw[];   // [G][MS][256] table slices | [G][MS * dsub] residual slices
    static_assert(MS % 16 == 0 && DSUB >= 0 && DSUB <= 64, "a slice is whole dwordx4 code words");
    constexpr int NW = MS / 16;          // dwordx4 words of one code in one slice
    constexpr int TILE = 256 * U;
    float* const s_lut = reinterpret_cast<float*>(s_resw);
    float* const s_res = s_lut + G * MS * 256;
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
    const int dsub = DSUB ? DSUB : d / M;
    const int RS = MS * dsub;            // floats of one residual slice
    const int NS = (M + MS - 1) / MS;
    const float* xq = x + (int64_t)q * d;
    // the group's lists; len 0: nothing to scan (an empty, masked or absent probe) -- uniform
    int lst[G], len[G];
    bool any = false;
    res_each<G>([&](auto g_) __attribute__((always_inline)) {
        constexpr int g = decltype(g_)::value;
        const int p = pg * G + g;
        int l = p < P ? probe_list[q * P + p] : -1, n = 0;
        if (l >= 0 && l < nlist && !(list_mask && !list_mask[l])) n = list_len[l];
        if (n <= 0) l = 0, n = 0;
        lst[g] = l;
        len[g] = n;
        any |= n > 0;
    });
    if (!any) return;
    float acc[G][U] = {};
    for (int s = 0; s < NS; s++) {
        const int m0 = s * MS, mc = min(MS, M - m0);
        const bool first = s == 0, last = s == NS - 1;
        // (no barrier here: the residuals were last read before the previous slice's table barrier)
        res_each<G>([&](auto g_) __attribute__((always_inline)) {
            constexpr int g = decltype(g_)::value;
            if (len[g] == 0) return;
            const float* cl = cc + (int64_t)lst[g] * d + m0 * dsub;
            for (int t = tid; t < mc * dsub; t += 256) s_res[g * RS + t] = xq[m0 * dsub + t] - cl[t];
        });
        __syncthreads();   // the residual slices are complete; the previous slice's gathers are finished
        if constexpr (DSUB > 0) {
            // RB rows at a time: their centroids are requested together, so a row's latency is paid once per RB rows
            constexpr int RB = DSUB <= 8 ? 8 : 4;
            for (int mb = 0; mb < mc; mb += RB) {
                float c[RB][DSUB];
                res_each<RB>([&](auto i_) __attribute__((always_inline)) {
                    constexpr int i = decltype(i_)::value;
                    load_row<DSUB>(pqc + ((int64_t)(m0 + min(mb + i, mc - 1)) * 256 + tid) * DSUB, c[i]);
                });
                res_each<RB>([&](auto i_) __attribute__((always_inline)) {
                    constexpr int i = decltype(i_)::value;
                    const int m = mb + i;
                    if (m >= mc) return;   // (uniform) the short last slice of an odd M
                    res_each<G>([&](auto g_) __attribute__((always_inline)) {
                        constexpr int g = decltype(g_)::value;
                        if (len[g] == 0) return;
                        float r[DSUB];
                        load_row<DSUB>(s_res + g * RS + m * DSUB, r);
                        s_lut[(g * MS + m) * 256 + tid] = fvec_ny_row<true>(r, c[i], DSUB);
                    });
                });
            }
        } else {
            for (int m = 0; m < mc; m++) {
                const float* cp = pqc + ((int64_t)(m0 + m) * 256 + tid) * dsub;
                res_each<G>([&](auto g_) __attribute__((always_inline)) {
                    constexpr int g = decltype(g_)::value;
                    if (len[g] == 0) return;
                    s_lut[(g * MS + m) * 256 + tid] = fvec_ny_row<true>(s_res + g * RS + m * dsub, cp, dsub);
                });
            }
        }
        __syncthreads();
        res_each<G>([&](auto g_) __attribute__((always_inline)) {
            constexpr int g = decltype(g_)::value;
            const int n = len[g];
            if (n == 0) return;
            const int p = pg * G + g;
            const int64_t off = list_off[lst[g]];
            const uint8_t* lc = codes + off * M + m0;
            const int64_t* lid = ids + off;
            float* o = out + (int64_t)q * q_stride + pair_off[(int64_t)q * (P + 1) + p];
            const float* lut = s_lut + g * MS * 256;
            const bool carry = n <= TILE;   // one step per slice: the running sums stay in registers
            // Two copies of the loop, with and without the validity predicates (k_ivfpq_scan_wide)
            auto scan_list = [&](auto ids_tag) __attribute__((always_inline)) {
                constexpr bool IDS = decltype(ids_tag)::value;
                for (int j0 = 0; j0 < n; j0 += TILE) {
                    res_each<U>([&](auto u_) __attribute__((always_inline)) {
                        constexpr int u = decltype(u_)::value;
                        const int j = j0 + u * 256 + tid;
                        if (j >= n) return;
                        // (the operands as values first: a choice between captured variables becomes a choice between their
                        //  addresses, and the sums would live in scratch memory)
                        const float kept = acc[g][u];
                        float a = 0.f;   // `float dis0 = 0` (gamma_index_ivfpq.h:236)
                        if (!first) {
                            if (carry) a = kept;
                            else a = o[j];
                        }
                        const uint8_t* cj = lc + (int64_t)j * M;
                        if constexpr (VEC) {
                            uint4 w[NW];
#pragma unroll
                            for (int i = 0; i < NW; i++) w[i] = reinterpret_cast<const uint4*>(cj)[i];
#pragma unroll
                            for (int i = 0; i < NW; i++) {
                                const uint32_t w4[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
                                float t[16];
#pragma unroll
                                for (int b = 0; b < 16; b++) t[b] = lut[(i * 16 + b) * 256 + ((w4[b >> 2] >> (8 * (b & 3))) & 255u)];
#pragma unroll
                                for (int b = 0; b < 16; b++) a += t[b];   // sequential, reference order
                            }
                        } else {
                            for (int m = 0; m < mc; m++) a += lut[m * 256 + cj[m]];
                        }
                        bool ok = true;
                        if constexpr (IDS) {
                            // ids are read only when something can reject an entry, and only where the result is stored
                            if (last) {
                                const int64_t id = lid[j];
                                ok = id >= 0 && is_valid_doc(filt, id);   // bit 63 = kDelIdxMask (realtime_mem_data.h:26)
                            }
                        }
                        const float sv = sentinel;
                        if (last) o[j] = ok ? a : sv;
                        else if (carry) acc[g][u] = a;
                        else o[j] = a;
                    });
                }
            };
            if (need_ids) scan_list(std::true_type{});
            else scan_list(std::false_type{});
        });
    }
}

template <int DSUB, bool VEC>
static void launch_wide_res_t(hipStream_t s, int nq, int d, int M, int P, const int* probe_list, const float* x, const float* cc,
                              const float* pqc, const int64_t* list_off, const int* list_len, const uint8_t* list_mask, int nlist,
                              const uint8_t* codes, const int64_t* ids, const int* pair_off, int64_t q_stride, float* out,
                              const FilterDesc* ftab, const int* qfil, int need_ids, const int* qperm) {
    const auto kern = k_ivfpq_scan_wide_res<kWideResMS, kWideResG, DSUB, VEC, kWideU>;
    static std::atomic<uint64_t> attr{0};   // per device
    if (first_call_on_device(attr))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)wide_res_lds_bytes(64));
    const int pg_cnt = (P + kWideResG - 1) / kWideResG;
    const dim3 grid((unsigned)(8 * (int64_t)((nq + 7) / 8) * pg_cnt));
    hipLaunchKernelGGL(kern, grid, dim3(256), wide_res_lds_bytes(d / M), s, nq, d, M, P, probe_list, x, cc, pqc, list_off, list_len,
                       list_mask, nlist, codes, ids, pair_off, q_stride, out, ftab, qfil, need_ids, INFINITY, qperm, pg_cnt);
}

void launch_ivfpq_scan_wide_res(hipStream_t s, int nq, int d, int M, int P, const int* probe_list, const float* x,
                                const float* cc, const float* pqc, const int64_t* list_off, const int* list_len,
                                const uint8_t* list_mask, int nlist, const uint8_t* codes, const int64_t* ids,
                                const int* pair_off, int64_t q_stride, float* out, const FilterDesc* ftab, const int* qfil,
                                int need_ids, const int* qperm) {
    if (nq <= 0 || P <= 0) return;
    if (M <= kWideMinM || M > kWideMaxM || d <= 0 || d % M != 0 || d / M > 64 || !x || !cc || !pqc) {
        launch_refused("launch_ivfpq_scan_wide_res: M outside 65 .. 256, d / M outside 1 .. 64, or no queries, centroids or codebook");
        return;
    }
    const bool vec = M % kWideResMS == 0;
#define GH_WRES(DS)                                                                                                              \
    do {                                                                                                                         \
        if (vec) launch_wide_res_t<DS, true>(s, nq, d, M, P, probe_list, x, cc, pqc, list_off, list_len, list_mask, nlist, codes, \
                                             ids, pair_off, q_stride, out, ftab, qfil, need_ids, qperm);                         \
        else launch_wide_res_t<DS, false>(s, nq, d, M, P, probe_list, x, cc, pqc, list_off, list_len, list_mask, nlist, codes,    \
                                          ids, pair_off, q_stride, out, ftab, qfil, need_ids, qperm);                            \
    } while (0)
    switch (d / M) {   // the sub-vector lengths of 768- and 1024-dimensional embeddings and fvec_ny_row's special forms
        case 1: GH_WRES(1); break;
        case 2: GH_WRES(2); break;
        case 3: GH_WRES(3); break;
        case 4: GH_WRES(4); break;
        case 6: GH_WRES(6); break;
        case 8: GH_WRES(8); break;
        case 12: GH_WRES(12); break;
        case 16: GH_WRES(16); break;
        default: GH_WRES(0); break;
    }
#undef GH_WRES
}

}  // namespace gh
