// scan_plan.cpp -- the scan stage's decisions (scan_plan.h).  Every threshold of the stage and the measurement behind it
// live here; gamma_hip_search.cpp carries the plan out.
#include "scan_plan.h"

#include <stdlib.h>

#include <cmath>

namespace gh {

ScanSwitches ScanSwitches::from_env() {
    ScanSwitches s;
    s.no_c8 = getenv("GAMMA_HIP_NO_C8") != nullptr;
    s.no_fused_ip = getenv("GAMMA_HIP_NO_FUSED_IP") != nullptr;
    s.no_scan_cf = getenv("GAMMA_HIP_NO_SCAN_CF") != nullptr;
    if (const char* e = getenv("GAMMA_HIP_SCAN_CF_CODES")) s.cf_codes = atof(e);
    s.no_q8 = getenv("GAMMA_HIP_NO_Q8") != nullptr;
    if (const char* e = getenv("GAMMA_HIP_Q8_MINLEN")) s.q8_minlen = atof(e);
    s.no_q8_demand = getenv("GAMMA_HIP_NO_Q8_DEMAND") != nullptr;
    s.no_bound_feedback = getenv("GAMMA_HIP_NO_BOUND_FEEDBACK") != nullptr;
    return s;
}

const ScanSwitches& ScanSwitches::get() {
    static const ScanSwitches s = from_env();
    return s;
}

int scan_group_size(int nq, int P, int G0) {
    // probes per workgroup: amortise the query table, but keep >= ~4096 workgroups in flight
    const char* ge = getenv("GAMMA_HIP_SCAN_G");
    const int g_env = ge ? atoi(ge) : 0;
    int G = g_env > 0 ? g_env : G0;
    // (a start that is not a power of two -- 5 with the byte-image pass -- steps to the power of two below it: 5 -> 4 -> 2, not
    //  5 -> 2, which skipped the G >= 4 the bounded scan needs for batches of 512 .. 585 queries at 32 probes)
    while (G > 1 && (int64_t)nq * ((P + G - 1) / G) < 4096) G = (G & (G - 1)) ? (1 << (31 - __builtin_clz((unsigned)G))) : G >> 1;
    return std::max(1, std::min(G, P));
}

ListStats scan_list_stats(int64_t ntotal, int nlist, const int* list_len, const uint8_t* list_mask, bool shard) {
    ListStats st;
    st.mean_len = (double)ntotal / std::max(1, nlist);
    st.owned = st.live = nlist;
    if (!shard) return st;
    int64_t tot = 0, n = 0;
    for (int l = 0; l < nlist; l++)
        if (list_len[l] > 0 && (!list_mask || list_mask[l])) {
            n++;
            tot += list_len[l];
        }
    st.live = n;
    // (a shard without a mask keeps the whole index's figures here although it holds 1 / W of the lists -- its
    //  expected-candidate count comes out W times too small.  Kept as it was: dropping this condition is the fix)
    if (list_mask) {
        st.owned = n;
        st.mean_len = n ? (double)tot / (double)n : 0.0;
    }
    return st;
}

// (recall_num up to 512 since round 6 -- with the wave-per-query selection of eight sorted runs, select.hip: C3 at
//  recall_num 300 3.00 -> 2.07 ms per 16384 queries (scan 0.475 -> 0.675 of the roofline, select 910 -> 277 us), the C4 shape
//  at 8 M 5.19 -> 3.96 ms per 8192; the candidate stages (1536 / 768 slots) overflow into the unfiltered path as ever)
static constexpr int cf_maxr = 512;

ScanPlan scan_plan_groups(const ScanShape& sh, const ScanSwitches& sw) {
    ScanPlan pl;
    const int P = sh.P, M = sh.M, R = sh.R;
    const double mean_len = sh.lists.mean_len;
    // Probes per workgroup.  8 probes per workgroup pay off with short lists (half the query-table re-reads, a tighter bound
    // from a first group of 8 lists); long lists or many probes balance better with 4 (tools/shape_sweep.py)
    int G0 = (mean_len <= 700.0 && P <= 64) ? 8 : 4;
    // (with the byte-table filter pass a consumer probe costs a third of a producer's: five probes bound nearly as well as
    //  eight -- C3: scan 729 us at 8, 691 at 6, 676 at 5, 671 at 4 but with queries whose slices overflow; GAMMA_HIP_SCAN_G to sweep)
    pl.c8_shape = !sh.pq4 && !sw.no_c8 && sh.l2 && M == 16 && R <= cf_maxr && sh.have_sums;
    if (G0 == 8 && pl.c8_shape && P > 8) G0 = 5;
    pl.t2_bytes = (int64_t)sh.nlist * M * (sh.pq4 ? 16 : 256) * (int64_t)sizeof(float);
    if (sh.two_phase) {
        // the producers take the query's nearest G1 owned probes only: everything else waits for the GLOBAL bound
        G0 = std::max(1, std::min(sh.G1, P));
        pl.t2_bytes = sh.lists.owned * M * 256 * (int64_t)sizeof(float);
    } else if (sh.compacted && sh.scan_bound && R <= 256) {
        // Sharded search with a compacted assignment: a query keeps ~P/W probes on this shard, all in its first group(s) --
        // the other P/G - 1 workgroups of the query would start only to find nothing to do (at W = 8 that was half of the
        // scan time).  When the expected candidate count per query is small, ONE workgroup takes all of a query's probes
        // (G = P): it bounds the R-th best itself (producer path of the pre-filter, no consumers), and computes the query's
        // PQ table on the fly instead of reading it back from HBM (IPF, scan.hip).
        pl.t2_bytes = sh.lists.live * M * 256 * (int64_t)sizeof(float);
        const double exp_probes = (double)P * (double)sh.lists.live / std::max(1, sh.nlist);
        const double exp_cand = exp_probes * mean_len;
        // (not beyond that: one workgroup walking 50 k - 200 k codes of a query is the long pole of the launch -- full-size
        //  C4 emulated, profiles/r04_scaling_emul.txt: W = 2 25.4 ms per step with 4 or 8 probes per workgroup, 27.9 with
        //  16, 31.4 with 32 or 64; W = 4 27.0 / 27.1 / 30.1 / 30.3 / 30.2)
        if (exp_cand <= 16384.0) {
            G0 = 1;
            while (G0 < P) G0 <<= 1;
        }
    }
    pl.G = scan_group_size(sh.nq, P, G0);
    pl.PGN = (P + pl.G - 1) / pl.G;
    // Threshold pre-filter: scan the nearest probe group first, bound each query's R-th best distance from it, and let the
    // scan of the remaining groups keep a short survivor list per query; the exact top-R then comes from a few hundred
    // survivors instead of ~10^4 candidates (select.hip).  Queries without a usable bound fall back to the unfiltered selection.
    // (sharded without a supplied assignment: probe groups are sparse, nothing to bound from)
    // small batches: one probe per workgroup, a single list rarely holds R candidates, and the unfiltered selection is
    // latency-bound anyway
    // (one group per query -- few probes, or a shard -- is fine: the producer bounds and compacts its own candidates)
    // (recall_num up to 1024 since round 5: slices of 2048 items and k_select_final_wg beyond 256 -- the configurations that
    //  need a long short-list, full-size C5 at ~1000, keep the pre-filter)
    constexpr int scan_gmin = 4, bound_maxr = 1024;
    pl.bound_eligible = !sh.pq4 && (!sh.shard || sh.compacted) && sh.scan_bound && R <= bound_maxr && P <= 128 &&
                        pl.G >= (sh.two_phase ? 1 : scan_gmin);
    return pl;
}

void scan_plan_passes(ScanPlan& pl, const ScanShape& sh, const ScanSwitches& sw, bool bounded) {
    const int nq = sh.nq, P = sh.P, M = sh.M, R = sh.R, G = pl.G, PGN = pl.PGN;
    const double mean_len = sh.lists.mean_len;
    pl.bounded = bounded;
    // ids are only read during the scan when something can reject an entry: a delete bit, a range filter, or a superseded
    // (bit 63) slot left behind by Update
    pl.need_ids = (!sh.prefiltered && (sh.any_clause || sh.rejects)) ? 1 : 0;
    // L2 table mode 0 (no precomputed table, H::table_mode): per-list tables from the residual (scan.hip RES) -- the plain and
    // the bounded loop; no query table, none of the passes built on T2 sums (the sums are absent: cf / c8 / q8 are off by their own gates)
    pl.res = !sh.pq4 && sh.l2 && sh.table_mode == 0;
    pl.fuse_ip = !sh.pq4 && bounded && !pl.res && PGN == 1 && (M == 16 || M == 32) && !sw.no_fused_ip;
    // (byte-table filter pass: a first group of a few probes bounds loosely for some queries -- slices of 2048 keep them out of the
    //  unfiltered path; never beyond 2048: the selection and the tie replay hold one slice in LDS)
    pl.cap = scan_slice_cap(R);
    // per-query slab of the distance buffer; multiple of 4 floats so rows are 16-byte aligned
    const int64_t q_stride0 = (std::max<int64_t>(1, (int64_t)P * std::max(1, sh.max_list_len)) + 3) & ~(int64_t)3;
    // (the longest candidate row of THIS batch, measured on its assignment: list shards, and whole-index calls whose general
    //  stride -- nprobe x the longest list -- would cut the batch into chunks)
    pl.q_stride = sh.q_stride_cap > 0 ? std::min(q_stride0, sh.q_stride_cap) : q_stride0;
    // enough queries that L2 capacity matters: run them in spatial order (kernels.hip)
    // (not when the T2 rows of the lists scanned here fit the L2s anyway: a shard of a small index)
    pl.order = sh.sort_queries && nq >= 256 && pl.t2_bytes > ((int64_t)8 << 20);
    pl.cf_ok = pl.q8_ok = false;
    pl.PGM = pl.nsl = PGN;
    pl.cf_span = pl.c8 = 0;
    if (!bounded) return;
    // Filter pass of the consumers (scan.hip, CF): needs the sums beside the arena the scan reads -- not the shadow arena of
    // a call running over lists compacted under its filter.  With it ONE consumer workgroup per query takes every probe
    // behind the producer's: two groups, two slices per query.
    // Short lists only (mean <= 2000 codes).  With thousands of codes per list the per-pair table costs next to
    // nothing and the pass loses: full-size C4 (6100 codes per list, 8192 queries) 27.7 ms without it; 38.6 ms with ONE
    // consumer workgroup per query (it stages more candidates than its SCAN_CF_CAP = 768 slots hold and the query goes to
    // the unfiltered path); 32.5 ms with the probes behind the producer's cut into consumer groups of ~48 k codes, each
    // with its own stage and slice (round 4, profiles/r04_scale_runs.txt) -- the margin candidates' exact recompute
    // and the second look at the codes cost more than the table build they save.  The split (cf_span) stays for the
    // lists in between: a consumer group takes at most ~64 k codes (cf_codes).
    constexpr double cf_maxlen = 2000.0;
    const bool cf_shape = scan_cf_applies(sh.l2, M, P, G, sh.have_sums, false);
    pl.cf_ok = !sw.no_scan_cf && R <= cf_maxr && (!sh.prefiltered || sh.cmp_has_sums) && PGN > 1 && mean_len <= cf_maxlen && cf_shape;
    // List-major byte-table pass for the consumer probes (q8scan.hip, round 5): same conditions as the filter pass it
    // replaces, one validity predicate for the whole call (GAMMA_HIP_NO_Q8: the query-major pass, for A/B)
    // (long lists: a tile's table staging and its chain of dependent loads are amortised over thousands of codes; at C3's
    //  244 codes per list a tile is one step of 64 codes per wave and the pass is latency-bound -- measured slower than the
    //  query-major pass there, profiles/r05_q8_*.txt -- so short lists keep the query-major filter pass)
    // (the switch, measured after the byte image went into the query-major pass: nlist 4096 / M 16 / nprobe 32 -- 732 codes per
    //  list 2.81 ms query-major, 2.84 list-major; 976: 3.31 / 3.20; 1465: 4.49 / 3.57 -- nlist 16384 / M 32 / nprobe 64 -- 732: 4.35 /
    //  4.38; 976: 5.36 / 4.87)
    // (a list shard with a supplied, compacted assignment runs it too: pairs of lists of other shards are simply not placed)
    // (shadow lists of the standing deletes are as long as the lists: the pass stays on over them -- C4 shape at 20 M with
    //  5 % deleted: 6.2 ms per 8192 queries without it, 4.5 unfiltered; lists cut down under a request's own clause
    //  are as short as the clause makes them: the query-major pass)
    pl.q8_ok = !sw.no_q8 && !sw.no_scan_cf && R <= 1024 && (!sh.shard || sh.compacted) &&
               (!sh.prefiltered || (sh.cmp_has_sums && !sh.cmp_by_clause)) && !sh.per_query_filters && PGN > 1 && cf_shape &&
               q8_supported(M, P, G, q_stride0) && mean_len >= sw.q8_minlen && sh.nlist <= 16384;
    if (pl.q8_ok) {
        pl.cf_ok = false;
        pl.PGM = 1;   // the main launch: producers only; slice 0: the producer's, slices 1 ..: the consumer probe groups' (k_q8_exact)
    } else if (pl.cf_ok) {
        const int rest = P - G;
        int nc = (int)std::ceil(rest * mean_len / sw.cf_codes);
        nc = std::max(1, std::min(nc, std::max(1, PGN - 1)));
        pl.cf_span = nc > 1 ? (rest + nc - 1) / nc : 0;
        pl.PGM = 1 + (nc > 1 ? (rest + pl.cf_span - 1) / pl.cf_span : 1);
        pl.nsl = pl.PGM;   // one survivor slice per probe group (slice 0: the producer's own)
        // the consumers' filter pass on a byte image of the query's table (scan.hip, "byte table"): a list per lane, 64 at most
        pl.c8 = (pl.c8_shape && (pl.cf_span > 0 ? pl.cf_span : rest) <= 64) ? 1 : 0;
    }
    pl.ready_off = (((size_t)nq + 1) * sizeof(int) + 7) & ~(size_t)7;
    pl.gcnt_off = pl.ready_off + (size_t)nq * sizeof(unsigned long long);
    pl.fl_off = pl.gcnt_off + (size_t)nq * (size_t)pl.nsl * sizeof(int);
    pl.scnt_bytes = pl.fl_off + ((size_t)nq + 1) * sizeof(int);
}

bool BoundFeedbackState::new_kind(uint64_t s) {
    // (what was learnt holds for one kind of call: other cuts or a filter bound differently -- start over, with counters of
    //  its own: the two slots alternate, so counts of the previous kind still on their way land elsewhere)
    if (s == sig) return false;
    sig = s;
    epoch++;
    off_calls = 0;
    calls = 0;
    seen[0] = seen[1] = 0;
    return true;
}

bool BoundFeedbackState::step(bool enabled, const Sample* s) {
    if (!enabled || off) return true;
    if (off_calls > 0) return --off_calls == 0;   // (0: this call re-probes)
    if (!s) return true;
    // (a sample that runs backwards, e.g. a late copy landing on words zeroed for a new kind of call, is ignored,
    //  and the fell-through count can never exceed the queries)
    const unsigned long long u = s->fell_through, n = s->queries;
    if (n < seen[1] || u < seen[0]) return true;
    const unsigned long long dn = n - seen[1], du = std::min(u - seen[0], dn);
    if (dn < 2048) return true;
    seen[0] = u;
    seen[1] = n;
    if (2 * du > dn) {   // more than half of the recent queries went to the unfiltered selection anyway
        off_calls = 256;
        backoffs++;
        return false;
    }
    return true;
}

}  // namespace gh
