// pqwide.hip -- the list scan of a wide 8-bit IVFPQ handle (gamma_hip_ivfpq_wide_init): 64 < M <= 256 sub-quantizers, so the
// pair's lookup table (M x 256 fp32 = M KB) does not fit the 64 KB of LDS a workgroup gets without a raised limit.  The
// reference's scanner takes any M (pq.M = ivfpq_param.nsubvector, gamma_index_ivfpq.cc:167-170; the scan of
// gamma_index_ivfpq.h:540-601).  Query tables, T2, the encoder and everything behind the scan are the 8-bit kernels.
//
// The table lives in LDS one SLICE at a time: kWideMS consecutive sub-quantizers (kWideMS x 256 floats).  A lane owns
// kWideU codes of the current tile (256 x kWideU codes) and carries their running sums from slice to slice, so the chain
//     dis = dis0;  for m ascending: dis += lut[m][code[m]]        (sequential fp32 adds, nothing reassociated)
// continues exactly where it stopped: parking a partial fp32 sum and picking it up again changes no bit.
//   * a segment (L2: one list; inner product: the group's G lists, whose slices depend on the query only) of ONE tile keeps
//     the sums in registers across the slices;
//   * a longer segment runs the slices outermost and the tiles inside, and parks each code's partial sum in the code's own
//     slot of the ADC slab (where the result goes anyway) with plain vector stores and loads: 8 bytes per code and extra
//     slice against kWideMS code bytes -- a slice is never rebuilt per tile.
// One workgroup per (query, group of G probes), placed like k_ivfpq4_scan_pair (block b runs on XCD b % 8, qperm).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "device_math.h"
#include "filter_dev.h"
#include "kernels.h"

namespace gh {

// the body once per u = 0 .. N - 1 with u a compile-time constant: the per-code registers (sums, code words, predicates) are
// never indexed by a loop variable, whatever the unroller decides about a body with calls and branches in it
template <int N, int I = 0, class F>
__device__ __forceinline__ void wide_each(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        wide_each<N, I + 1>(f);
    }
}

// VEC: M is a multiple of MS (whole slices) -- a code's MS bytes of a slice are MS / 16 dwordx4 words, the next step's words
// (and parked sums) are requested before this step's gathers, the next slice's T2 entries before this slice's tiles.
// !VEC: any M (an odd M, a last slice shorter than MS): byte loads, no prefetch.
template <bool L2, int MS, bool VEC, int U>
__global__ __launch_bounds__(256) void k_ivfpq_scan_wide(
        int nq, int M, int P, int G, const int* __restrict__ probe_list, const float* __restrict__ pair_dis0,
        const float* __restrict__ st2, const float* __restrict__ T2, const int64_t* __restrict__ list_off,
        const int* __restrict__ list_len, const uint8_t* __restrict__ list_mask, int nlist,
        const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids, const int* __restrict__ pair_off,
        int64_t q_stride, float* out, const FilterDesc* __restrict__ ftab, const int* __restrict__ qfil,
        int need_ids, float sentinel, const int* __restrict__ qperm, int pg_cnt) {
    extern __shared__ float s_lutw[];   // [MS][256]: all of the kernel's LDS, a gather address is (byte << 2) + an immediate
    static_assert(MS % 16 == 0 && MS * 1024 <= 65536, "a slice is whole dwordx4 code words and at most 64 KB");
    constexpr int NW = MS / 16;         // dwordx4 words of one code in one slice
    constexpr int TILE = 256 * U;
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
    const int NS = (M + MS - 1) / MS;
    const int64_t msz = (int64_t)M * 256;
    const float* st2q = st2 + (int64_t)q * msz;
    const int p_begin = pg * G, p_end = min(P, p_begin + G);
    // probe p's list, or false: nothing to scan (uniform)
    auto pick = [&](int p, int& l, int& len) __attribute__((always_inline)) {
        l = probe_list[q * P + p];
        if (l < 0 || l >= nlist) return false;
        if (list_mask && !list_mask[l]) return false;
        len = list_len[l];
        return len > 0;
    };
    for (int ps = p_begin; ps < p_end; ps += (L2 ? 1 : G)) {
        const int pe = L2 ? ps + 1 : p_end;
        int ntiles = 0, l0 = 0, len0 = 0;   // (l0: the segment's list under L2)
        for (int p = ps; p < pe; p++) {
            int l, len;
            if (!pick(p, l, len)) continue;
            ntiles += (len + TILE - 1) / TILE;
            l0 = l;
            len0 = len;
        }
        if (ntiles == 0) continue;
        const bool carry = ntiles == 1;   // one step per slice: the running sums stay in registers
        float acc[U];
        uint4 cur[U][NW];
        float t2n[MS];                    // (VEC && L2) the thread's T2 entries of the next slice to build
        const float* t2l = L2 ? T2 + (int64_t)l0 * msz : nullptr;
        if constexpr (VEC && L2) {
#pragma unroll
            for (int i = 0; i < MS; i++) t2n[i] = t2l[tid + 256 * i];
        }
        for (int s = 0; s < NS; s++) {
            const int m0 = s * MS, mc = min(MS, M - m0);
            const bool first = s == 0, last = s == NS - 1;
            // a step's operands: the code words of the lane's U codes in this slice and, from the second slice of a parked
            // segment on, their partial sums
            auto fetch = [&](const uint8_t* lc, const float* o, int len, int j0, uint4 (&w)[U][NW], float (&a)[U], float dis0) __attribute__((always_inline)) {
                wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                    constexpr int u = decltype(u_)::value;
                    const int j = j0 + u * 256 + tid;
                    const uint4* cp = reinterpret_cast<const uint4*>(lc + (int64_t)min(j, len - 1) * M + m0);
#pragma unroll
                    for (int i = 0; i < NW; i++) w[u][i] = cp[i];
                    if (first) a[u] = dis0;
                    else if (!carry) a[u] = o[min(j, len - 1)];
                });
            };
            if constexpr (VEC && L2) {   // the first step's words are on their way while the slice is built
                const float* o0 = out + (int64_t)q * q_stride + pair_off[(int64_t)q * (P + 1) + ps];
                fetch(codes + list_off[l0] * M, o0, len0, 0, cur, acc, pair_dis0[q * P + ps]);
            }
            __syncthreads();   // the previous slice's gathers are finished
            if constexpr (VEC && L2) {
                const float* sq = st2q + m0 * 256;
#pragma unroll
                for (int i = 0; i < MS; i++) s_lutw[tid + 256 * i] = __builtin_fmaf(-2.0f, sq[tid + 256 * i], t2n[i]);
                if (!last) {
#pragma unroll
                    for (int i = 0; i < MS; i++) t2n[i] = t2l[(m0 + MS) * 256 + tid + 256 * i];
                }
            } else if (L2) {
                for (int e = tid; e < mc * 256; e += 256) s_lutw[e] = __builtin_fmaf(-2.0f, st2q[m0 * 256 + e], t2l[m0 * 256 + e]);
            } else {
                for (int e = tid; e < mc * 256; e += 256) s_lutw[e] = st2q[m0 * 256 + e];
            }
            __syncthreads();
            for (int p = ps; p < pe; p++) {
                int l, len;
                if (!pick(p, l, len)) continue;
                const int64_t off = list_off[l];
                const uint8_t* lc = codes + off * M;
                const int64_t* lid = ids + off;
                const float dis0 = pair_dis0[q * P + p];
                float* o = out + (int64_t)q * q_stride + pair_off[(int64_t)q * (P + 1) + p];
                if constexpr (VEC && !L2) fetch(lc, o, len, 0, cur, acc, dis0);
                // Two copies of the loop, with and without the validity predicates (the lesson of k_ivfpq4_scan_pair: their
                // loads make the compiler wait for every outstanding load, the prefetched words included).
                auto scan_list = [&](auto ids_tag) __attribute__((always_inline)) {
                    constexpr bool IDS = decltype(ids_tag)::value;
                    for (int j0 = 0; j0 < len; j0 += TILE) {
                        bool ok[U];
                        wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                            constexpr int u = decltype(u_)::value;
                            ok[u] = true;
                        });
                        if constexpr (IDS) {
                            // ids are read only when something can reject an entry, and only where the result is stored
                            if (last) {
                                wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                                    constexpr int u = decltype(u_)::value;
                                    const int j = j0 + u * 256 + tid;
                                    if (j < len) {
                                        const int64_t id = lid[j];
                                        ok[u] = id >= 0 && is_valid_doc(filt, id);   // bit 63 = kDelIdxMask (realtime_mem_data.h:26)
                                    }
                                });
                            }
                        }
                        const bool more = VEC && j0 + TILE < len;   // uniform
                        uint4 nxt[U][NW];
                        float accn[U];
                        if constexpr (VEC) {
                            if (more) fetch(lc, o, len, j0 + TILE, nxt, accn, dis0);
#pragma unroll
                            for (int i = 0; i < NW; i++) {
                                float t[U][16];
                                wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                                    constexpr int u = decltype(u_)::value;
                                    const uint32_t w4[4] = {cur[u][i].x, cur[u][i].y, cur[u][i].z, cur[u][i].w};
#pragma unroll
                                    for (int b = 0; b < 16; b++)
                                        t[u][b] = s_lutw[(i * 16 + b) * 256 + ((w4[b >> 2] >> (8 * (b & 3))) & 255u)];
                                });
                                __builtin_amdgcn_sched_barrier(0);   // the word's gathers in flight before the add chains
                                wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                                    constexpr int u = decltype(u_)::value;
#pragma unroll
                                    for (int b = 0; b < 16; b++) acc[u] += t[u][b];   // sequential, reference order
                                });
                            }
                        } else {
                            wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                                constexpr int u = decltype(u_)::value;
                                const int j = j0 + u * 256 + tid;
                                if (j >= len) return;
                                if (first) acc[u] = dis0;
                                else if (!carry) acc[u] = o[j];
                                const uint8_t* cj = lc + (int64_t)j * M + m0;
                                for (int m = 0; m < mc; m++) acc[u] += s_lutw[m * 256 + cj[m]];
                            });
                        }
                        wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                            constexpr int u = decltype(u_)::value;
                            const int j = j0 + u * 256 + tid;
                            // (the operands as values first: a choice between two captured variables becomes a choice between
                            //  their addresses, and the sums would live in scratch memory)
                            const float a = acc[u], sv = sentinel;
                            const bool keep = ok[u];
                            if (j < len) {
                                if (last) o[j] = keep ? a : sv;
                                else if (!carry) o[j] = a;
                            }
                        });
                        if constexpr (VEC) {
                            if (more) {
                                wide_each<U>([&](auto u_) __attribute__((always_inline)) {
                                    constexpr int u = decltype(u_)::value;
                                    acc[u] = accn[u];
#pragma unroll
                                    for (int i = 0; i < NW; i++) cur[u][i] = nxt[u][i];
                                });
                            }
                        }
                    }
                };
                if (need_ids) scan_list(std::true_type{});
                else scan_list(std::false_type{});
            }
        }
    }
}

void launch_ivfpq_scan_wide(hipStream_t s, bool l2, int nq, int M, int P, const int* probe_list, const float* dis0,
                            const float* st2, const float* T2, const int64_t* list_off, const int* list_len,
                            const uint8_t* list_mask, int nlist, const uint8_t* codes, const int64_t* ids,
                            const int* pair_off, int64_t q_stride, float* out, const FilterDesc* ftab, const int* qfil,
                            int need_ids, const int* qperm, int G, int pg_cnt) {
    if (nq <= 0 || pg_cnt <= 0) return;
    if (M <= kWideMinM || M > kWideMaxM || G <= 0 || (int64_t)pg_cnt * G < P || (l2 && !T2)) {
        launch_refused("launch_ivfpq_scan_wide: M outside 65 .. 256, probe groups that do not cover nprobe, or L2 without a table");
        return;
    }
    const dim3 grid((unsigned)(8 * (int64_t)((nq + 7) / 8) * pg_cnt));
    const bool vec = M % kWideMS == 0;
#define GH_WIDE(LL, VV)                                                                                                          \
    hipLaunchKernelGGL((k_ivfpq_scan_wide<LL, kWideMS, VV, kWideU>), grid, dim3(256), wide_lds_bytes(), s, nq, M, P, G, probe_list, \
                       dis0, st2, T2, list_off, list_len, list_mask, nlist, codes, ids, pair_off, q_stride, out, ftab, qfil,     \
                       need_ids, LL ? INFINITY : -INFINITY, qperm, pg_cnt)
    if (l2 && vec) GH_WIDE(true, true);
    else if (l2) GH_WIDE(true, false);
    else if (vec) GH_WIDE(false, true);
    else GH_WIDE(false, false);
#undef GH_WIDE
}

}  // namespace gh
