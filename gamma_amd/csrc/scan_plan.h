// scan_plan.h -- the host decisions of the IVFPQ scan stage (gamma_hip_search.cpp ivfpq_stage_a) as plain values and pure
// functions: the environment switches (ScanSwitches), what a call looks like (ScanShape), which kernels run over which
// groups and slices (ScanPlan), and the feedback that turns the bounded scan off on data where it does not pay
// (BoundFeedbackState).  Nothing of HIP in here: a host compiler alone builds scan_plan.cpp, and tests/scan_plan_check.cc
// checks the plans of known shapes without a GPU.  The .hip files take their shared constants from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace gh {

constexpr int SCAN_SLICE = 1024;   // candidate slice of one workgroup (global) up to recall_num 256; a producer needs recall_num +
                                   // one histogram bin: 2048 beyond (ScanBound::slice_cap, scan_slice_cap)
constexpr int Q8_POS_BITS = 25;    // q8scan.hip: candidate = position in the query's segment | probe << 25

inline int scan_slice_cap(int K) { return K <= 256 ? SCAN_SLICE : 2 * SCAN_SLICE; }   // 1024 up to recall_num 256, 2048 up to 1024
// true when launch_ivfpq_scan_pair would run the filter pass (CF) for a bounded scan with these arguments; the caller
// then launches TWO groups per query -- the producer's G probes and one consumer group with all the others
inline bool scan_cf_applies(bool l2, int M, int P, int G, bool have_sums, bool store_all) {
    return l2 && have_sums && !store_all && (M == 16 || M == 32) && P > G;
}
// (the caller checks nlist <= 16384: the per-list counters live in LDS)
inline bool q8_supported(int M, int P, int G, int64_t q_stride) {
    return (M == 16 || M == 32) && P <= 128 && G >= 1 && (P + G - 1) / G <= 64 && q_stride < ((int64_t)1 << Q8_POS_BITS);
}
// G0: probes per workgroup to start from; shrinks through the powers of two below it.  GAMMA_HIP_SCAN_G overrides G0 and is
// read per call: tools sweep it inside one process
int scan_group_size(int nq, int P, int G0);

// The switches of the stage, read from the environment once per process (get()); names, defaults and meaning as documented
// in README.md / DESIGN.md.  This is the one place that reads them.
struct ScanSwitches {
    bool no_c8 = false;               // GAMMA_HIP_NO_C8: no byte image in the query-major filter pass
    bool no_fused_ip = false;         // GAMMA_HIP_NO_FUSED_IP: query tables from HBM even with one group per query
    bool no_scan_cf = false;          // GAMMA_HIP_NO_SCAN_CF: neither filter pass (query-major or list-major)
    double cf_codes = 65536.0;        // GAMMA_HIP_SCAN_CF_CODES: codes a consumer group of the query-major pass takes at most
    bool no_q8 = false;               // GAMMA_HIP_NO_Q8: the query-major pass where the list-major one would run (A/B)
    double q8_minlen = 800.0;         // GAMMA_HIP_Q8_MINLEN: codes per list from which the list-major pass runs
    bool no_q8_demand = false;        // GAMMA_HIP_NO_Q8_DEMAND: a shard's k_q8_exact never computes table entries on demand
    bool no_bound_feedback = false;   // GAMMA_HIP_NO_BOUND_FEEDBACK: the bounded scan whenever it is eligible
    static ScanSwitches from_env();
    static const ScanSwitches& get();
};

// Codes per list of the lists THIS handle scans, and how many lists those are: a list shard holds (or, under a mask, scans)
// 1 / W of the lists.  Not a shard: the whole index, no loop.
struct ListStats {
    double mean_len = 0.0;
    int64_t owned = 0;   // lists of this handle: non-empty and unmasked under a shard's mask, otherwise nlist
    int64_t live = 0;    // a shard's non-empty (and unmasked) lists, mask or not; otherwise nlist
};
ListStats scan_list_stats(int64_t ntotal, int nlist, const int* list_len, const uint8_t* list_mask /* nullptr: none */, bool shard);

struct ScanShape {
    int nq = 0, P = 0, R = 0, M = 0, nlist = 0;
    int max_list_len = 0;
    int64_t q_stride_cap = 0;       // > 0: the longest candidate row of the batch, measured (list shards)
    bool l2 = true, pq4 = false;
    int table_mode = 1;
    bool have_sums = false;         // the per-code sums and t2max exist beside the arena
    bool prefiltered = false, cmp_has_sums = false, cmp_by_clause = false;   // the call runs over lists compacted under its filter
    bool any_clause = false, per_query_filters = false;
    bool rejects = false;           // a delete bit or a superseded slot can reject an entry
    bool shard = false, compacted = false, two_phase = false;
    int G1 = 2;                     // two-phase: probes of the producers' group
    bool scan_bound = true;         // the handle's switch (GAMMA_HIP_NO_SCAN_BOUND)
    bool sort_queries = false;      // the handle sorts queries and has a list rank
    ListStats lists;
};

struct ScanPlan {
    // scan_plan_groups
    int G = 1, PGN = 1;             // probes per workgroup, probe groups per query
    bool c8_shape = false;          // the byte image of the query-major filter pass fits the shape
    int64_t t2_bytes = 0;           // T2 rows of the lists scanned here
    bool bound_eligible = false;    // the bounded scan applies (the feedback has the last word)
    // scan_plan_passes
    bool bounded = false, res = false, fuse_ip = false, cf_ok = false, q8_ok = false, order = false;
    int c8 = 0, cf_span = 0;
    int PGM = 1, nsl = 1, cap = SCAN_SLICE;   // probe groups of the main launch, survivor slices per query, items per slice
    int need_ids = 0;
    int64_t q_stride = 0;
    // bounded: rq | ready[nq] | gcnt[nq][nsl] | fl inside w_scnt (rq, at offset 0: count + list of the queries that need the repair
    // launch, 8-byte aligned; fl: count + list of the queries k_select_final left to the unfiltered selection, flag = 1)
    size_t ready_off = 0, gcnt_off = 0, fl_off = 0, scnt_bytes = 0;
};
// The plan is made in two calls, with the feedback between them: groups and eligibility, then everything that depends on
// whether THIS call runs bounded.
ScanPlan scan_plan_groups(const ScanShape& sh, const ScanSwitches& sw);
void scan_plan_passes(ScanPlan& pl, const ScanShape& sh, const ScanSwitches& sw, bool bounded);

// Feedback for the bounded scan (results are the same either way): the pre-filter pays when the first probe group
// bounds well.  On data where it does not (full-size C5: noise-dominated inner-product vectors, 2460 survivors per
// query instead of ~100, every query sent to the unfiltered selection AFTER the filtered scan) the path costs more
// than it saves.  k_select_final counts the queries it gives up on; the totals come back through a pinned word every
// few calls, and while more than half of the recent queries fell through the handle scans unbounded, re-probing now
// and then.  This is the arithmetic; the copies and the event are BoundFeedback's (gamma_hip_internal.h).
struct BoundFeedbackState {
    struct Sample { unsigned long long fell_through, queries; };   // cumulative counts of the current kind of call
    uint64_t sig = 0;                        // (nprobe, recall_num, metric, filter, shard) of the calls the counts are of
    int epoch = 0;                           // kinds of call seen; its low bit selects the counter slot
    bool off = false;                        // gamma_hip_set_scan_bound_feedback(h, 0): the pre-filter whenever it applies
    int calls = 0, off_calls = 0;            // bounded calls of this kind; unbounded calls left before the re-probe
    int64_t backoffs = 0;                    // times the handle turned the pre-filter off
    unsigned long long seen[2] = {0, 0};     // what the last decision had read
    int slot() const { return epoch & 1; }
    static uint64_t signature(int P, int R, bool l2, bool any_clause, bool shard) {
        return ((uint64_t)P << 40) ^ ((uint64_t)R << 20) ^ ((uint64_t)(l2 ? 1 : 0) << 1) ^ (any_clause ? 1u : 0u) ^
               ((uint64_t)(shard ? 1 : 0) << 2) ^ (1ull << 63);
    }
    void set_on(bool on) { off = !on; off_calls = 0; }
    bool consults() const { return !off && off_calls == 0; }   // step() looks at a sample
    bool copy_due() const { return calls < 4 || (calls & 15) == 0; }   // the first calls of a kind, then every 16th
    bool new_kind(uint64_t s);                  // true: another kind of call -- counters reset, the other slot
    bool step(bool enabled, const Sample* s);   // s: the landed sample or nullptr; returns whether this call is bounded
};

}  // namespace gh
