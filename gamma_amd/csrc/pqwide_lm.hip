// pqwide_lm.hip -- the list scan of a wide 8-bit IVFPQ handle (pqwide.hip) list-major, behind gamma_hip_ivfpq_wide_set_lm_scan
// (DESIGN.md section 39).  k_ivfpq_scan_wide is one workgroup per (query, probe group): it fetches a list's codes and its T2
// row once per probing query and, on a list longer than its tile, parks the partial sums in the ADC slab between table slices.
// Here a work unit is
//   one list  x  one slab of kWideLmSlab consecutive codes (a code per lane, 4 waves)  x  one tile of up to QT of the
//   (query, probe) pairs that probe the list (the call's inverse index: k_inv_count / k_inv_scan_w / k_inv_fill),
// walked by a persistent grid, SLICES OUTERMOST, PAIRS INSIDE: per slice of kWideMS sub-quantizers the lane's two dwordx4 code
// words and -- L2 -- the thread's entries of the list's T2 slice are loaded once for all pairs of the tile; per pair the
// table slice (fmaf(-2, st2, t2) or st2) goes through one half of two LDS buffers of [kWideMS][256] floats while the waves
// gather the previous pair from the other half: one barrier per (slice, pair) step, the steps of a unit one pipeline across
// the slice boundaries.  The running sums of ALL pairs of the tile, acc[QT], live in registers for the whole unit:
//     acc[i] = dis0(pair i);  for m ascending: acc[i] += lut_i[m][code[m]]      (sequential fp32 adds, nothing reassociated)
// is k_ivfpq_scan_wide's chain, continued across slices, so the slab is the same byte for byte and nothing is parked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "filter_dev.h"
#include "kernels.h"
#include "pq4.h"   // k_inv_count, k_inv_fill

namespace gh {

__global__ void k_inv_scan_w(const int* __restrict__ cnt, const int* __restrict__ list_len, int nlist, int* __restrict__ start,
                             int* __restrict__ cur, int* __restrict__ ustart);

namespace {
constexpr int WIDE_LM_GRID = 256 * 2;   // persistent, two workgroups of 64 KB per CU: each walks the unit list with stride gridDim.x
static_assert(kWideLmQueryTile <= 64 && kWideLmSlab == 256, "a tile's pairs sit in the lanes of one wave; a code per thread");

// pqwide.hip's wide_each: the body once per i = 0 .. N - 1 with i a compile-time constant, so acc[] is never indexed by a
// loop variable
template <int N, int I = 0, class F>
__device__ __forceinline__ void wide_lm_each(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        wide_lm_each<N, I + 1>(f);
    }
}
__device__ __forceinline__ int lm_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lm_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
}  // namespace

template <bool L2, int QT>
__global__ __launch_bounds__(256, 2) void k_ivfpq_scan_wide_lm(
        int M, int P, const float* __restrict__ pair_dis0, const float* __restrict__ st2, const float* __restrict__ T2,
        const int64_t* __restrict__ list_off, const int* __restrict__ list_len, int nlist,
        const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids, const int* __restrict__ pair_off,
        int64_t q_stride, float* __restrict__ out, const FilterDesc* __restrict__ ftab, const int* __restrict__ qfil,
        int need_ids, float sentinel, const int* __restrict__ inv, const int* __restrict__ inv_start,
        const int* __restrict__ inv_cnt, const int* __restrict__ ustart) {
    extern __shared__ float4 s_lmw[];   // [2][MS][256] floats and nothing else
    constexpr int MS = kWideMS;
    constexpr int NW = MS / 16;         // dwordx4 words of one code in one slice
    constexpr int SV = MS * 64;         // float4 entries of one table slice
    constexpr int NV = SV / 256;        // ... of one thread: entries tid + 256 * k
    const int tid = threadIdx.x, lane = tid & 63;
    const int NS = M / MS;
    const int64_t msz = (int64_t)M * 256;
    const int nunits = ustart[nlist];
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {   // (everything that decides control flow below is uniform)
        // unit u: lists in order, a list's slabs in order, a slab's tiles in order (neighbouring workgroups read the same codes)
        int l = 0, hi = nlist - 1;
        while (l < hi) {   // last list with ustart[l] <= u
            const int mid = (l + hi + 1) >> 1;
            if (ustart[mid] <= u) l = mid; else hi = mid - 1;
        }
        const int n = inv_cnt[l], len = list_len[l];
        if (n <= 0 || len <= 0) continue;   // (no such unit exists: k_inv_scan_w gives these lists none)
        const int tiles = (n + QT - 1) / QT, rel = u - ustart[l];
        const int slab = rel / tiles, t0 = (rel - slab * tiles) * QT;
        const int r0 = slab * kWideLmSlab;
        if (r0 >= len) continue;
        const int nt = min(QT, n - t0), first = inv_start[l] + t0;
        const int64_t off = list_off[l];
        const int j = r0 + tid, jc = min(j, len - 1);   // this lane's code; the lanes beyond the list read its last one
        const uint8_t* cj = codes + (off + jc) * M;
        const float4* t2l = reinterpret_cast<const float4*>(T2 + (L2 ? (int64_t)l * msz : 0));
        // pair t of the tile in lane t of every wave: its query, dis0, filter and the slab position of the lane-0 code
        const int pr = inv[first + min(lane, nt - 1)];
        const int qv = pr / P;
        const float d0v = pair_dis0[pr];
        const int64_t oov = (int64_t)qv * q_stride + pair_off[(int64_t)qv * (P + 1) + (pr - qv * P)] + r0;
        const int oolo = (int)(uint32_t)oov, oohi = (int)(oov >> 32);
        const int fv = (need_ids && qfil) ? qfil[qv] : 0;

        float acc[QT];
        wide_lm_each<QT>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            acc[i] = lm_lane_f(d0v, i);
        });
        uint4 cw[NW];
        float4 t2r[NV], sn[NV];
        auto load_cw = [&](int s) __attribute__((always_inline)) {
            const uint4* cp = reinterpret_cast<const uint4*>(cj + s * MS);
#pragma unroll
            for (int w = 0; w < NW; w++) cw[w] = cp[w];
        };
        auto load_t2 = [&](int s) __attribute__((always_inline)) {
            if constexpr (L2) {
#pragma unroll
                for (int k = 0; k < NV; k++) t2r[k] = t2l[s * SV + tid + 256 * k];
            }
        };
        auto load_s2 = [&](int i, int s) __attribute__((always_inline)) {
            const float4* sq = reinterpret_cast<const float4*>(st2 + (int64_t)lm_lane_i(qv, i) * msz) + s * SV;
#pragma unroll
            for (int k = 0; k < NV; k++) sn[k] = sq[tid + 256 * k];
        };
        auto write_lut = [&](float4* buf) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < NV; k++) {
                float4 v = sn[k];
                if constexpr (L2) {
                    v.x = __builtin_fmaf(-2.0f, v.x, t2r[k].x);
                    v.y = __builtin_fmaf(-2.0f, v.y, t2r[k].y);
                    v.z = __builtin_fmaf(-2.0f, v.z, t2r[k].z);
                    v.w = __builtin_fmaf(-2.0f, v.w, t2r[k].w);
                }
                buf[tid + 256 * k] = v;
            }
        };
        // The unit's steps (slice s, pair i), slices outermost, are ONE pipeline: in step t the waves gather from `cur`, write
        // step t + 1's table from sn / t2r into `nxt` and request step t + 2's st2 entries into sn -- and, where step t + 2
        // opens a slice, that slice's T2 entries into t2r, whose last reader was the write just done.  after(s, i, ...): the
        // step behind (s, i) and whether it exists.
        auto after = [&](int s, int i, int& s1, int& i1) __attribute__((always_inline)) {
            const bool wrap = i + 1 == nt;
            s1 = s + (wrap ? 1 : 0);
            i1 = wrap ? 0 : i + 1;
            return s1 < NS;
        };
        auto request = [&](int s1, int i1) __attribute__((always_inline)) {   // what the step behind (s1, i1) needs
            int s2, i2;
            if (after(s1, i1, s2, i2)) {
                if (s2 != s1) load_t2(s2);
                load_s2(i2, s2);
            }
        };
        float4* cur = s_lmw;
        float4* nxt = s_lmw + SV;
        load_cw(0);
        load_t2(0);
        load_s2(0, 0);
        write_lut(cur);   // (the previous unit's gathers are behind its last barrier)
        request(0, 0);
        __syncthreads();
        // The pair loop is NOT unrolled (eight copies of the step spilled the gathered values to scratch memory); acc is still
        // never indexed by a run-time value: the step works on acc[0] and the array rotates by one register per pair, QT times
        // per slice, so pair i is back in acc[i] when the next slice starts.
        auto rotate = [&]() __attribute__((always_inline)) {
            const float a0 = acc[0];
            wide_lm_each<QT - 1>([&](auto k_) __attribute__((always_inline)) {
                constexpr int k = decltype(k_)::value;
                acc[k] = acc[k + 1];
            });
            acc[QT - 1] = a0;
        };
        for (int s = 0; s < NS; s++) {
#pragma unroll 1
            for (int i = 0; i < QT; i++) {
                if (i < nt) {
                    const float* lut = reinterpret_cast<const float*>(cur);
                    float t[MS];
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const uint32_t w4[4] = {cw[w].x, cw[w].y, cw[w].z, cw[w].w};
#pragma unroll
                        for (int b = 0; b < 16; b++)
                            t[w * 16 + b] = lut[(w * 16 + b) * 256 + ((w4[b >> 2] >> (8 * (b & 3))) & 255u)];
                    }
                    __builtin_amdgcn_sched_barrier(0);   // all gathers in flight before the table write and the add chain
                    int s1, i1;
                    if (after(s, i, s1, i1)) {
                        write_lut(nxt);
                        if (s1 != s) load_cw(s1);   // (this slice's words were last read by the gathers above)
                        request(s1, i1);
                    }
                    float a = acc[0];
#pragma unroll
                    for (int m = 0; m < MS; m++) a += t[m];   // sequential, reference order
                    acc[0] = a;
                    __syncthreads();   // step (s, i)'s gathers are over, the next step's table is in place
                    float4* const x = cur;
                    cur = nxt;
                    nxt = x;
                }
                rotate();
            }
        }
        // ---- after the last slice: the sums, or the sentinel the pair kernel writes for a rejected entry ----
        // (the predicates stand here, outside the pair loop: their loads cost the loop no wait; the id is read once per unit,
        //  and only when something can reject an entry)
        int64_t id = 0;
        bool live = true;
        if (need_ids) {
            id = ids[off + jc];
            live = id >= 0;   // bit 63 = kDelIdxMask (realtime_mem_data.h:26)
        }
#pragma unroll 1
        for (int i = 0; i < nt; i++) {
            const int64_t oo = (int64_t)(((uint64_t)(uint32_t)lm_lane_i(oohi, i) << 32) | (uint32_t)lm_lane_i(oolo, i));
            bool ok = live;
            if (need_ids) ok = live && is_valid_doc(ftab[lm_lane_i(fv, i)], id);
            const float a = acc[0], sv = sentinel;
            if (j < len) out[oo + tid] = ok ? a : sv;
            rotate();
        }
    }
}

void launch_ivfpq_scan_wide_lm(hipStream_t s, bool l2, int nq, int M, int P, const int* probe_list, const float* dis0,
                               const float* st2, const float* T2, const int64_t* list_off, const int* list_len,
                               const uint8_t* list_mask, int nlist, int max_list_len, const uint8_t* codes,
                               const int64_t* ids, const int* pair_off, int64_t q_stride, float* out, const FilterDesc* ftab,
                               const int* qfil, int need_ids, void* scratch) {
    if (nq <= 0) return;
    if (wide_lm_ms(M) == 0 || (l2 && !T2)) {
        launch_refused("launch_ivfpq_scan_wide_lm: M is not 96, 128, ... 256, or L2 without a table");
        return;
    }
    // what the unit count cannot exceed: every probed list has at most one ragged tile per slab
    constexpr int QT = kWideLmQueryTile;
    const int64_t pairs = (int64_t)nq * std::max(0, P);
    const int64_t slabs = ((int64_t)std::max(0, max_list_len) + kWideLmSlab - 1) / kWideLmSlab;
    const int64_t ub = (pairs / QT + std::min<int64_t>(pairs, std::max(0, nlist))) * slabs;
    if (!scratch || list_mask || P <= 0 || nlist <= 0 || pairs > 2147483647 || ub > 2147483647) {
        launch_refused("launch_ivfpq_scan_wide_lm: no scratch for the inverse index, a list mask, or nq x nprobe / units beyond 2^31 - 1");
        return;
    }
    // inv [nq * P] | cnt | start | cur [nlist] | ustart [nlist + 1]  (ivfflat_lm_scratch_bytes)
    int* inv = static_cast<int*>(scratch);
    int* cnt = inv + (size_t)nq * P;
    int* start = cnt + nlist;
    int* cur = start + nlist;
    int* ustart = cur + nlist;
    const int npairs = (int)pairs;
    (void)hipMemsetAsync(cnt, 0, (size_t)nlist * sizeof(int), s);
    hipLaunchKernelGGL(k_inv_count, dim3((npairs + 255) / 256), dim3(256), 0, s, probe_list, npairs, nlist, list_len, cnt);
    hipLaunchKernelGGL(k_inv_scan_w, dim3(1), dim3(1024), 0, s, cnt, list_len, nlist, start, cur, ustart);
    hipLaunchKernelGGL(k_inv_fill, dim3((npairs + 255) / 256), dim3(256), 0, s, probe_list, npairs, nlist, list_len, start, cur, inv);
    const int lds = (int)wide_lm_lds_bytes();
    static std::atomic<uint64_t> attr{0};   // the attribute is per DEVICE
    if (first_call_on_device(attr)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ivfpq_scan_wide_lm<true, QT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ivfpq_scan_wide_lm<false, QT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
    (void)hipGetLastError();   // (a stale error of an earlier call is not this launch's)
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ub, WIDE_LM_GRID)));
#define GH_WIDELM(LL)                                                                                                          \
    hipLaunchKernelGGL((k_ivfpq_scan_wide_lm<LL, QT>), grid, dim3(256), (size_t)lds, s, M, P, dis0, st2, T2, list_off, list_len, \
                       nlist, codes, ids, pair_off, q_stride, out, ftab, qfil, need_ids, LL ? INFINITY : -INFINITY, inv, start, \
                       cnt, ustart)
    if (l2) GH_WIDELM(true);
    else GH_WIDELM(false);
#undef GH_WIDELM
    // a scan that did not start leaves the slab as the previous call left it and the selection would read that: never silent
    if (hipGetLastError() != hipSuccess) launch_refused("launch_ivfpq_scan_wide_lm: the kernel failed to launch (64 KB of dynamic LDS)");
}

}  // namespace gh
