// gamma_hip_internal.h -- the handle of libgamma_hip.so (HBM-resident state, workspaces, locks) and the helpers its
// translation units share: gamma_hip.cpp (life cycle, switches, accounting), gamma_hip_store.cpp (realtime lists,
// raw store, columns, bitmap: the writers), gamma_hip_search.cpp / _ivfflat.cpp / _flat.cpp / _shard.cpp (the search
// pipelines and their entry points), gamma_hip_combine.cpp (the combining queue).
#pragma once
#include "../../include/gamma_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "call_slots.h"
#include "dev_mem.h"
#include "kernels.h"

namespace ghi {

constexpr double kPI = 3.14159265;  // realtime/realtime_mem_data.h:24
constexpr int64_t kDelMask = (int64_t)(1ULL << 63);

struct StageEvent {
    int stage;
    hipEvent_t a, b;
    bool count;
};

// The bounded scan's feedback on a handle: the counters k_select_final adds to, their pinned image and the copy between
// them.  The rules (what a sample decides) are gh::BoundFeedbackState's, scan_plan.h.
struct BoundFeedback : gh::BoundFeedbackState {
    unsigned long long* d_stat = nullptr;     // 2 slots x {queries given to the unfiltered selection, queries}, then: consumer groups that gave up waiting
    unsigned long long* pin_stat = nullptr;   // the two slots as of some recent call (pinned host memory)
    hipEvent_t copy_ev = nullptr;             // behind the last copy into pin_stat
    bool copy_pending = false;
    unsigned long long* d_slot() const { return d_stat + 2 * slot(); }   // the counts of the current kind of call
    unsigned long long* d_timeouts() const { return d_stat + 4; }
    // an eligible call: is it bounded?  enabled: ScanSwitches::no_bound_feedback is not set
    hipError_t begin(hipStream_t s, uint64_t sig_now, bool enabled, bool* bounded) {
        if (new_kind(sig_now)) {
            if (copy_pending) {   // a copy of the previous kind's counts still on its way: it lands before the words are reused
                (void)hipEventSynchronize(copy_ev);
                copy_pending = false;
            }
            pin_stat[2 * slot()] = pin_stat[2 * slot() + 1] = 0;
            const hipError_t e = hipMemsetAsync(d_slot(), 0, 2 * sizeof(unsigned long long), s);
            if (e != hipSuccess) return e;
        }
        Sample smp = {0, 0};
        bool landed = false;
        if (enabled && consults()) {
            // (the pair is consulted only once the copy that writes it has completed -- copy_ev -- so the two words
            //  belong to one state of the counters)
            landed = !copy_pending || hipEventQuery(copy_ev) == hipSuccess;
            if (landed) copy_pending = false;
            else (void)hipGetLastError();
            smp = {pin_stat[2 * slot()], pin_stat[2 * slot() + 1]};
        }
        *bounded = step(enabled, landed ? &smp : nullptr);
        return hipSuccess;
    }
    // behind k_select_final of a bounded call: the counts as of this call, for a later call's decision (16 bytes; ~5 us on
    // the call's critical path, so: the first calls of a kind, then every 16th)
    hipError_t end(hipStream_t s) {
        hipError_t e = hipSuccess;
        if (copy_due() && !copy_pending) {
            e = hipMemcpyAsync(pin_stat + 2 * slot(), d_slot(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && !copy_ev) e = hipEventCreateWithFlags(&copy_ev, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(copy_ev, s);
            if (e != hipSuccess) return e;
            copy_pending = true;
        }
        calls++;
        return e;
    }
};

}  // namespace ghi
using ghi::StageEvent;

struct WriteLock;

// GEMM-form distance calls (coarse quantizer, assign, k-means: faiss's exhaustive_L2sqr_blas, faiss:utils/distances.cpp:215-296)
// whose sgemm_ kernel is NOT restated (oracle/gamma_oracle.c, go_gemm_k_split): K beyond 768 or an odd split, K = 384 with
// a database remainder block of 9..512 rows, remainder blocks of a few rows (nx mod 4096 / ny mod 1024 in 1..7: MKL takes
// another kernel there -- measured: the rows of a 1..3-row query remainder differ in ~10 % of their entries by an ulp).
// Such calls are COUNTED (gamma_hip_blas_form_not_restated), never silent.
inline bool blas_form_not_restated(int64_t nx, int64_t ny, int d) {
    if (d > 768 || (d > 384 && (d & 7))) return true;
    const int64_t rx = nx % 4096, ry = ny % 1024;
    if ((rx >= 1 && rx <= 7) || (ry >= 1 && ry <= 7)) return true;
    return d == 384 && ry >= 9 && ry <= 512;
}

struct gamma_hip_index {
    int device = 0;
    // Concurrency (SURVEY 8b "Threading": Search from any number of client threads while ONE indexing thread adds
    // and API threads delete; the reference's lists are lock-free for readers, realtime_mem_data.cc:279-300):
    //   stream / search_mu : searches.  One at a time (they share the workspaces); search_mu is held for a whole
    //                        call, mu only while the call reads the handle's state and enqueues its kernels.
    //   wstream / writer_mu: writers (list appends, encode, raw / bitmap / column updates) on their own stream, so
    //                        they neither wait for the searches in flight nor hold them up; mu while they work.
    //   list meta versions : a search's kernels read the (offset, length) table of the VERSION that was current
    //                        when it was enqueued; a writer publishes a new version after its copies (the
    //                        reference publishes retrieve_idx_pos_ after the copy, realtime_mem_data.cc:299-300).
    //                        Old extents stay intact inside the arena, so a search in flight keeps reading a
    //                        consistent prefix of the insert log.
    //   reallocation       : growing the arena / raw store / bitmap frees memory a search in flight may read --
    //                        the writer then takes search_mu too and drains both streams first (WriteLock::exclusive).
    // Lock order: writer_mu -> search_mu -> mu.
    hipStream_t stream = nullptr, wstream = nullptr;
    // side stream of the searches: kernels of a call that may overlap its main chain (the heap replay of the coarse
    // rows with a tie, beside the query tables); forked from and joined into `stream` by events, never used alone
    hipStream_t side = nullptr;
    hipStream_t side2 = nullptr;   // the deferred tie replay (its own stream: the coarse heap fix must not queue behind it)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool coarse_join_pending = false;
    // deferred tie replay (gamma_hip_set_deferred_replay): the replay of a device-pointer call's flagged queries runs on
    // the side stream and the search stream waits for it only before the next kernel that touches what it reads (the
    // next call's or chunk's pair offsets) -- its latency hides behind the next coarse quantizer and query tables
    hipEvent_t ev_rfork = nullptr, ev_rdone = nullptr;
    bool defer_replay = false, defer_now = false, replay_pending = false;
    // the _wait entries: completion event and pinned overflow word of every call in flight, each owned by its call from the
    // take under the search lock until its waiter has read the word (call_slots.h)
    ghi::CallSlots call_slots;
    // large host-buffer IVFPQ calls from several client threads (ivfpq_search_host_overlap): a call's queries go up on
    // `up_stream` into its own staging slot BEFORE it takes the search lock, its results come down behind its tie replay
    // on the side stream into pinned memory, and the caller waits for its own event with the handle already free
    struct HostSlot {
        DevBuf x, D, I;
        void* pin = nullptr;
        size_t pin_bytes = 0;
        hipEvent_t ev_up = nullptr, ev_done = nullptr;
        bool busy = false;
    };
    HostSlot hslot[2];
    std::mutex hs_mu;
    std::condition_variable hs_cv;
    hipStream_t up_stream = nullptr;
    // flat search with overlapping callers (gamma_hip_flat_search_device_wait): what a flat call's tie replay reads -- the first
    // row chunk's slab, the survivor log, the flag list, the candidate tables -- exists TWICE; a call that finds a flat replay
    // pending switches to the other bank instead of waiting, and waits (in stream order) only for the replay that last read
    // the bank it is about to overwrite
    DevBuf fbank[5];
    int flat_bank = 0;
    hipEvent_t ev_bank[2] = {nullptr, nullptr};
    bool bank_used[2] = {false, false};
    bool replay_is_flat = false;
    // (the flat call's "did a survivor list overflow" word is read by the host; a _wait call reads it AFTER its completion
    //  event, with the handle free, from the pinned word of its own slot (call_slots), and redoes the call without a bound in
    //  the rare yes)
    int* flat_over_dst = nullptr;    // set by the _wait entry for the call under way
    int flat_over_passes = 0;        // filter passes of the call under way whose overflow word the _wait entry reads later
    bool flat_no_bound = false;
    std::atomic<int> big_calls_in_flight{0};
    std::atomic<int64_t> big_calls_overlap_seen_ns{INT64_MIN / 2};
    // the shadow lists of compact_lists_for_call stay valid while nothing was written and the call has no clauses of its own
    // (standing deletes): write_gen counts writer calls (WriteLock), cmp_gen = the count the shadow lists were built at
    uint64_t write_gen = 1, cmp_gen = 0;
    bool cmp_has_sums = false, cmp_sums_built = false;
    bool cmp_by_clause = false;   // the shadow lists were cut under a request's own clauses (as short as those make them)
    bool merge_flags = false;   // the last gamma_hip_ivfpq_merge_rerank left tie flags of its slice in w_tlist
    int shard_cut_nq = 0;       // the last shard search left the cut-tie flags of its nq queries in w_tcut
    bool shard_cut_chunked = false;   // ... of a call of several chunks: gathered in w_shard_cut
    const uint8_t* merge_shard_flags = nullptr;   // [nshards][nq] for the next merge (gamma_hip_ivfpq_merge_set_shard_flags)
    int merge_nql = 0;
    std::mutex mu, search_mu, writer_mu;
    WriteLock* wl = nullptr;   // the writer holding mu (for exclusive() deep inside the arena code)
    static constexpr int NVER = 4;
    int64_t* d_ver_off[NVER] = {nullptr, nullptr, nullptr, nullptr};
    int* d_ver_len[NVER] = {nullptr, nullptr, nullptr, nullptr};
    void* pin_ver[NVER] = {nullptr, nullptr, nullptr, nullptr};   // pinned staging of a version's tables
    hipEvent_t ver_ev[NVER] = {nullptr, nullptr, nullptr, nullptr};   // wstream: the version's tables are in place
    hipEvent_t rd_ev[NVER] = {nullptr, nullptr, nullptr, nullptr};    // stream: the last search reading it is past its list kernels
    bool rd_set[NVER] = {false, false, false, false};
    int cur_ver = 0;
    std::string err;

    // raw vector store
    // The rows live in ONE array, raw, and raw_et says what they are (gh::RowType, the numbering of
    // gamma_hip_raw_elem_type; fixed at the first init): fp32 (gamma_hip_raw_init), IEEE binary16 (_init_f16: rows of 2 * raw_d
    // bytes, the writers round the caller's fp32 on the writer stream, store_kernels.hip), uint8 / int8 (_init_i8: the writers
    // take fp32 that converts exactly, checked on the host, gamma_hip_raw_i8_check) or one scalar-quantised code per element
    // (_init_sq8).  One growth machinery for all of them, rows of raw_d * raw_esz() bytes.
    // Who reads them: a reader of every element type takes raw_rows_ref() and switches on its et.  A reader that was only ever
    // taught fp32 rows takes raw_f32() and nothing else -- null on a narrow store, so its "needs the raw store" check fails
    // there instead of misreading bytes.  Nothing outside the store's own bookkeeping touches the array.
    int raw_d = 0;
    int raw_et = gh::ROW_F32;
    ghi::DevArray raw;
    int64_t nraw = 0;
    int64_t raw_cap() const { return raw_d > 0 ? (int64_t)(raw.cap / ((size_t)raw_d * raw_esz())) : 0; }   // rows
    // sq8 store: sq8_vmin / sq8_vmax: the ranges (empty until set or trained); d_sq8_tab: 2 * raw_d float2 -- the readers'
    // decode table {step[j], vmin[j]} and behind it the writers' encode table {inv[j], vmin[j]}.
    std::vector<float> sq8_vmin, sq8_vmax, sq8_step;
    float* d_sq8_tab = nullptr;
    size_t raw_esz() const { return gh::row_elem_bytes(raw_et); }
    bool has_raw_rows() const { return raw.p != nullptr; }
    int raw_elem_type() const { return raw_et; }
    bool raw_narrow() const { return raw_et != gh::ROW_F32; }   // any store but fp32
    const float* raw_f32() const { return raw_et == gh::ROW_F32 ? static_cast<const float*>(raw.p) : nullptr; }
    float* raw_f32() { return raw_et == gh::ROW_F32 ? static_cast<float*>(raw.p) : nullptr; }
    // raw vectors SHARDED with their lists (gamma_hip_raw_put, round 6): the store holds the rows of the vectors in this shard's
    // lists only, in arrival order; raw_slot[vid] = row (-1: held by another shard).  Such a handle re-ranks nothing by itself --
    // has_rank searches, flat search and raw_gets refuse -- it serves _shard_exact / _shard_export_exact.
    bool raw_sparse = false;
    std::vector<int32_t> h_raw_slot;
    ghi::DevArrayOf<int32_t> d_raw_slot;
    int64_t raw_slot_cap() const { return (int64_t)(d_raw_slot.cap / sizeof(int32_t)); }   // entries
    // a sparse store's rows can be rewritten in place, dropped (gamma_hip_raw_drop) and their rows reused: nraw = rows handed
    // out so far, raw_live of them hold a vector, raw_free lists the others (reused, last freed first, before the store grows)
    int64_t raw_live = 0;
    std::vector<int32_t> raw_free;
    // The store grows IN PLACE where the runtime offers virtual memory management: one address range reserved up
    // front, physical chunks mapped behind the rows as they come -- no copy, no second allocation, no wait for the
    // searches in flight (the reference keeps 500 000-vector segments for the same reason, vector/memory_raw_vector.cc:
    // 90-142; a segment table would cost every gather an indirection, a mapped range costs nothing).  Fallback: a
    // geometric reallocation (DevArray::grow; raw.mapped / raw.regrows say which it is and how often it moved).

    // Re-rank filter (rerank_filter.hip, gamma_hip_set_rerank_filter): a one-byte image of a dense fp32 store's rows, created by
    // the first has_rank call that qualifies -- on the search stream, under mu, so beside no writer -- and kept in step by the dense
    // writers from then on: they re-quantise the rows they wrote on the writer stream (behind `built`), in front of their wait.
    // raw_clear releases it; it is never dumped or loaded.
    // Feedback on the pattern of the coarse filter's: the kernel counts the survivors (gh::kRerankFilterStatLines words), the
    // host the candidates it handed over; the survivor words come back through pinned memory behind an event, paired with the
    // candidate count as of the launch in front of the copy, and while more than half of the recent candidates of one kind of
    // call (metric, d, R, k) survived, the handle runs the plain kernel for 256 calls and probes again.  Same results either way.
    struct RerankImage {
        ghi::DevArray rows, aux;   // u8[cap][raw_d], {err, nrm}[cap]
        float* par = nullptr;      // gh::rerank_image_par_bytes(raw_d): lo, Delta, |lo|
        bool on = false;           // image rows [0, nraw) are those of the store's rows
        hipEvent_t built = nullptr;
        int mode = 1;              // 0 off, 1 calls of kAutoMinNq queries and more, 2 every call
        static constexpr int kAutoMinNq = 1024;
        int form = 0;              // gamma_hip_set_rerank_filter_form: 0 automatic, 1 the workgroup kernel always, 2 the wave form wherever admitted
        int last_form = 0;         // the kernel of the last filtered call: 1 workgroup, 2 wave (0: none yet)
        int64_t wave_calls = 0;
        unsigned long long* d_stat = nullptr;
        unsigned long long* pin_stat = nullptr;
        unsigned long long seen[2] = {0, 0};           // {survivors, candidates} at the last decision
        unsigned long long cand = 0, cand_at_copy = 0;   // candidates handed to the filter so far; as of the copy under way / landed
        hipEvent_t copy_ev = nullptr;
        bool copy_pending = false;
        uint64_t sig = 0;
        int off_calls = 0;   // plain calls left before the next probe
        int64_t backoffs = 0, calls = 0;
        int64_t cap_rows(int d) const { return d > 0 ? (int64_t)std::min(rows.cap / (size_t)d, aux.cap / (2 * sizeof(float))) : 0; }
    } rf;

    // numeric scalar columns (on-device range filters)
    struct Column {
        int dtype = 0;
        ghi::DevArrayOf<uint8_t> d;
        int64_t n = 0;
    };
    std::map<int, Column> fields;
    // STRING columns as dictionary-encoded item lists (on-device term filters): doc i = tok[start .. start + len),
    // row word off[i] = start << 16 | len (gamma_hip_term_update rewrites a row)
    struct TermColumn {
        ghi::DevArrayOf<int64_t> d_off;
        ghi::DevArrayOf<int32_t> d_tok;
        int64_t ndocs = 0, ntok = 0;
        std::vector<int64_t> h_rows;   // host copy of the row words
    };
    std::map<int, TermColumn> terms;

    // delete bitmap
    ghi::DevArrayOf<uint8_t> d_bitmap;   // d_bitmap.cap bytes, the host copy beside it
    int64_t bitmap_bits = 0;
    std::vector<uint8_t> h_bitmap;
    bool bitmap_any = false;   // any delete bit set
    int64_t n_moved = 0;       // inverted-list slots marked superseded (bit 63) since creation

    // IVFPQ model
    bool ivf_init = false, trained = false;
    int d = 0, nlist = 0, M = 0, ksub = 256, dsub = 0, code_size = 0, metric = GAMMA_HIP_METRIC_L2;
    int bucket_init = 1000, bucket_max = 1280000;
    float *d_cc = nullptr, *d_cc_norms = nullptr, *d_pqc = nullptr, *d_T2 = nullptr;
    int* d_list_rank = nullptr;   // spatial order of the coarse centroids (scan locality only)
    bool sort_queries = getenv("GAMMA_HIP_NO_QUERY_SORT") == nullptr;
    bool scan_bound = getenv("GAMMA_HIP_NO_SCAN_BOUND") == nullptr;
    ghi::BoundFeedback bound_fb;   // feedback for the bounded scan (scan_plan.h: results are the same either way)

    // inverted-list arena
    uint8_t* d_codes = nullptr;
    int64_t* d_ids = nullptr;
    // L2 scan filter pass (k_ivfpq_scan_pair<.., CF>): per arena entry sum_m T2[list][m][code[m]], kept beside the codes
    // by every writer; per list sum_m max_c |T2[l][m][c]| (the margin of the filter).  Null for IVFFLAT / inner-product
    // indexes (the inner-product scan has no per-list table to avoid).
    float* d_sums = nullptr;
    float* d_t2max = nullptr;
    float t2max_all = 0.f;   // max over d_t2max (set with it)
    // L2 table mode (faiss::IndexIVFPQ::use_precomputed_table after train / Load): 1 = the precomputed table T2 is resident,
    // 0 = it would exceed precomputed_table_max_bytes (faiss:IndexIVFPQ.cpp:441-449) -- none is built, L2 searches score with
    // per-(query, list) residual tables (gamma_index_ivfpq.h:239-245).  Decided by Init from nlist * M and the limit.
    int table_mode = 1;
    // what the scan launcher takes as (st2, T2): mode 0 -> (the PQ codebook, nullptr), see scan.hip RES
    const float* scan_st2(bool l2) const { return (l2 && table_mode == 0) ? d_pqc : w_st2.as<float>(); }
    bool keep_sums = false;   // set by Init: IVFPQ handles (GAMMA_HIP_NO_CODE_SUMS=1 turns the filter pass off)
    // OPQ (gamma_hip_opq_set; gamma_hip_opq.cpp): the d x d rotation, device + host copy.  Null = none: every path is the one
    // it was without it.  Set while the lists are empty and never replaced afterwards, so kernels in flight never lose it.
    // Vectors that are QUANTISED (coarse quantizer, PQ encoder, query tables, scan) are rotated first -- the writers' into
    // we_xrot on the writer stream, a search call's into w_xrot on the search stream, once for the whole call before its
    // first chunk (no growth while the call's kernels are queued; a later call's growth goes through hipFree, which
    // waits for the device like every other workspace's) -- the exact re-rank and the tie replay read the caller's vectors.
    float* d_opq = nullptr;
    std::vector<float> h_opq;
    bool group_member = false;   // created by gamma_hip_group_create: refuses a matrix
    // list shard over a supplied assignment (gamma_hip_ivfpq_search_shard_preassigned): the longest candidate row of the
    // call, measured on the device -- the slab stride of its chunks (0: nprobe x the longest list)
    int64_t q_stride_cap = 0;
    int64_t arena_cap = 0, arena_used = 0, arena_waste = 0;   // entries; waste = abandoned extents inside used
    // the three arena arrays (codes, ids, code sums) are mapped ranges like the raw store where the runtime allows:
    // growth maps chunks behind them -- no copy, no second arena, no exclusive lock (the reference grows per bucket for
    // the same reason, realtime/realtime_mem_data.cc:152-188,426-474).  Fallback: reallocation under the exclusive lock.
    // arena.cur owns what d_codes / d_ids / d_sums point at (arena_adopt sets them), arena.alt is the repack's target set
    // (the two swap roles; see arena_repack), arena.retired the ranges that may not be mapped again.
    ghi::ArenaSets arena;
    bool arena_vmm() const { return arena.cur.mapped(); }
    int64_t arena_regrows = 0;   // growths that moved the arena (0 with virtual memory management)
    int64_t repack_min_entries = 1 << 16;                     // no repack for less waste than this
    int64_t n_repacks = 0;
    int64_t repack_verified = 0, repack_verify_failures = 0;   // read-backs of a repack target / those that differed from the source
    std::vector<int64_t> h_list_off;
    std::vector<int> h_list_len, h_list_cap, h_deleted;
    std::vector<uint8_t> h_extend_time;
    int64_t* d_list_off = nullptr;
    int* d_list_len = nullptr;
    uint8_t* d_list_mask = nullptr;
    std::vector<uint8_t> h_list_mask;
    std::vector<int64_t> vid_pos;
    int max_list_len = 0;
    int64_t ntotal = 0;

    // workspace
    DevBuf w_mat, w_coarse_dis, w_probe, w_xn, w_st2, w_pair_off, w_qtotal, w_dist, w_cand_dis,
            w_cand_pos, w_cand_ids, w_exact, w_selv, w_selp, w_x, w_outd, w_outl, w_stage, w_shard_cut, w_filter,
            w_m_dis, w_m_ids, w_part_v, w_part_i, w_assign, w_codes_tmp, w_qperm, w_qbins, w_scnt, w_sflag, w_surv, w_pair_base, w_q8, w_q8meta, w_q8cand, w_q8int,
            w_pair_ip, w_flat_cand, w_flat_meta, w_full_cdis, w_full_probe, w_ftab, w_qfil, w_tieflag, w_tcut, w_tlist, w_textra, w_fq, w_fraw, w_frcnt, w_lm_units, w_lm_cnt, w_fbits, w_cmp_codes, w_cmp_ids, w_cmp_len, w_cmp_sums, w_fD, w_fI, w_fx, w_fslab, w_flog, w_mr_vals, w_mr_ids, w_mr_meta, w_xrot, w_bf_hist, w_bf_meta, w_bf_cand, w_bs_hist, w_bs_meta, w_bs_cand,
            we_mat, we_cdis, we_x, we_assign, we_codes, we_stage, we_chk, we_xrot;   // writer side (encode, bitmap_set): never shared with a search
    unsigned long long* d_scan_codes = nullptr;
    size_t dist_budget_bytes = (size_t)8 << 30;   // per-chunk ADC distance buffer (288 GB of HBM per GPU)

    // device copy of the filter table of the running call (entry 0 = the call's own descriptor) and the
    // host image of what entry 0 holds, so an unchanged descriptor is not uploaded again
    gh::FilterDesc ftab_shadow;
    bool ftab_valid = false;

    bool exact_ties = true;    // gamma_hip_set_exact_ties
    std::atomic<int64_t> ties_unhonoured{0};   // gamma_hip_ties_not_honoured
    int scan_dbg_now = 0;   // GAMMA_HIP_SCAN_PART (timing experiments)
    std::atomic<int64_t> blas_unrestated{0};   // gamma_hip_blas_form_not_restated
    int coarse_fused = 1;      // gamma_hip_set_coarse_fused: 0 matrix path, 1 bf16 filter where supported, 2 fp32 fused path
    // bf16 filter of the fused coarse path (coarse.hip): the centroids' hi / lo image in the MFMA fragment layout, rebuilt
    // wherever d_cc_norms is; cc_img_ok: every centroid norm lies in the filter's magnitude domain.
    // Feedback on the pattern of the bounded scan's: k_coarse_final counts the queries the bf16 chain gave up on (margin
    // band wider than the strip lists: data with norms >> distances; queries outside the domain); the cumulative pair
    // comes back through pinned words, and while more than 1/8 of the recent queries of one kind of call (nlist, nprobe,
    // d) were given up on, the handle runs the fp32 filter, re-probing every 256 calls.  Results are the same either way.
    void* d_cc_img = nullptr;
    size_t cc_img_bytes = 0;
    bool cc_img_ok = false;
    float cc_norm_max = 0.f;
    unsigned long long* d_cbf_stat = nullptr;     // {given up on, queries}
    unsigned long long* pin_cbf_stat = nullptr;
    unsigned long long cbf_seen[2] = {0, 0};
    hipEvent_t cbf_copy_ev = nullptr;
    bool cbf_copy_pending = false;
    uint64_t cbf_sig = 0;
    int cbf_off_calls = 0;                         // fp32 calls left before the re-probe
    int64_t cbf_backoffs = 0, cbf_calls = 0;       // times the handle turned the bf16 filter off; calls that ran it
    // gamma_hip_flat_filter_stats: filter passes launched, (query, row) pairs they scored, passes redone without the bound
    std::atomic<int64_t> ff_passes{0}, ff_pairs{0}, ff_redone{0};
    // gamma_hip_ivfflat_scan_stats: calls the small path served; query chunks of the chunked path scanned by the pair kernel,
    // by the fixed-length list-major kernel, by the row-sliced one
    std::atomic<int64_t> fl_small{0}, fl_pair{0}, fl_lm{0}, fl_lms{0};
    bool small_path = true;    // gamma_hip_set_small_path
    bool flat_narrow_rows = false;   // gamma_hip_set_flat_narrow_rows: flat search serves a float16 / uint8 / int8 raw store
    bool ivfflat_narrow_rows = false;   // gamma_hip_set_ivfflat_narrow_rows: the same for the IVFFLAT search
    // gamma_hip_set_sparse_narrow_rows: gamma_hip_raw_put / _raw_drop and the shard's exact entries serve a float16 / uint8 /
    // int8 / sq8 raw store (rows sharded with their lists in 2 or 1 bytes per element)
    bool sparse_narrow_rows = false;
    bool flat_sq8_rows = false;      // gamma_hip_set_flat_sq8_rows: flat search serves an sq8 raw store
    bool ivfflat_sq8_rows = false;   // gamma_hip_set_ivfflat_sq8_rows: the same for the IVFFLAT search
    int small_presel = 0;      // 0: pre-selection by estimate, > 0: always, that many slices (tests)
    // multi-vector documents (VIDMgr::VID2DocID, vector/raw_vector_common.h:90-95): docid of every vid, host + device;
    // empty = single-vector documents, docid == vid.  Every delete-bitmap / filter test goes through it.
    std::vector<int32_t> h_v2d;
    ghi::DevArrayOf<int32_t> d_v2d;
    int64_t doc_of(int64_t v) const { return (v >= 0 && (size_t)v < h_v2d.size()) ? (int64_t)h_v2d[v] : v; }
    bool doc_deleted(int64_t v) const {
        const int64_t dd = doc_of(v);
        return dd >= 0 && dd < bitmap_bits && !h_bitmap.empty() && ((h_bitmap[dd >> 3] >> (dd & 7)) & 1);
    }
    bool ivfflat = false;      // gamma_hip_ivfflat_init: lists of vector ids (1 dummy code byte), rows from the raw store
    // gamma_hip_binivf_init (ivfflat is set too: no PQ tables, no code sums): lists of binary codes (code_size = nbits / 8),
    // d = nbits; the centroid codes, the search's {queries, heap admissions} counters (gamma_hip_binivf_stats)
    bool binivf = false;
    uint8_t* d_bin_cc = nullptr;
    unsigned long long* d_bin_stats = nullptr;   // [5]: + the spread scan's {queries, chunks, candidates}
    // gamma_hip_binivf_set_scan_mode: 0 one wave per query, 1 spread (binivf_spread.hip) whenever the workspace allows,
    // -1 spread for calls of up to kBinSpreadAutoMaxNq queries; the queries that fell back for lack of workspace
    int bin_scan_mode = -1;
    int64_t bin_sp_fallback = 0;
    // gamma_hip_binflat_init (gamma_hip_binflat.cpp): every code in vid order for the exact Hamming search, rows of bf_cs
    // bytes; bf_count is published after the rows it counts are in place; {queries, candidates, heap admissions} counters
    // and the number of query sub-batches (gamma_hip_binflat_stats); host images of a call's candidate totals / segment bases
    bool bf_init = false;
    int bf_cs = 0;
    ghi::DevArrayOf<uint8_t> d_bf_codes;
    int64_t bf_count = 0, bf_subbatches = 0;
    int64_t bf_cap() const { return bf_cs > 0 ? (int64_t)(d_bf_codes.cap / (size_t)bf_cs) : 0; }   // rows
    unsigned long long* d_bf_stats = nullptr;
    std::vector<uint32_t> bf_tot_h;
    std::vector<int64_t> bf_base_h;
    int coarse_cap = gh::kCoarseCap;
    unsigned long long* d_tie_stats = nullptr;   // {coarse rows redone, top-R cuts through a tie, queries replayed}
    // what stage A leaves for the tie replay of stage B (ties.hip)
    struct TieCtx {
        bool on = false, bounded = false;
        int G = 0, nsl = 0, cap = 0;
        int64_t q_stride = 0;
    } tie;

    // last-search stage info
    int last_nq = 0, last_P = 0, last_R = 0;
    const int* last_qperm = nullptr;   // query order of the last stage A (null: arrival order)

    // request combining of small concurrent host-buffer searches (gamma_hip_ivfpq_search)
    struct Waiter {
        const gamma_hip_search_params* p;
        int nq, k, mode;   // mode: coarse path resolved from THIS request's size
        int kind = 0;      // 0: IVFPQ search, 1: flat search
        const float* x;
        float* D;
        int64_t* I;
        int rc = 0;
        // delivery (gamma_hip_combine.cpp, combine_worker): every waiter sleeps on its OWN mutex + condition variable; the
        // worker's helper copies a batch's rows into the callers' buffers, links the waiters into a forest, wakes the
        // first FAN, and every woken waiter wakes FAN more on its way out -- a batch of 128 is awake after three hops
        // instead of 128 wake-ups issued by one thread through one mutex
        static constexpr int FAN = 4;
        bool done = false;
        std::mutex wm;
        std::condition_variable cv;
        Waiter* child[FAN] = {nullptr, nullptr, nullptr, nullptr};
    };
    std::mutex comb_mu;
    std::condition_variable comb_wcv;   // the worker waits here
    std::deque<Waiter*> comb_q;
    bool prefiltered = false;           // this call runs over lists compacted under its filter: nothing is left to reject
    bool comb_busy = false;             // a batch (or a direct call) is in flight
    bool comb_stop = false;
    std::thread comb_thread;
    bool combine = getenv("GAMMA_HIP_NO_COMBINE") == nullptr;
    // pinned staging of the combined batches: one set per batch from formation until its last caller has copied its
    // rows out (only the worker allocates them); four, so that forming a batch never waits for a delivery
    static constexpr int NSET = 4;
    void* comb_pin[NSET] = {nullptr, nullptr, nullptr, nullptr};
    void* comb_pin_dev[NSET] = {nullptr, nullptr, nullptr, nullptr};   // their addresses on the device (results are stored in place)
    size_t comb_pin_bytes[NSET] = {0, 0, 0, 0};
    // pinned staging of small direct calls (host_search; the search lock serialises its users)
    void* dir_pin = nullptr;
    void* dir_pin_dev = nullptr;   // its address on the device (hipHostGetDevicePointer), nullptr: not mapped
    size_t dir_pin_bytes = 0;

    // profiling
    int profile = 0;   // 0 off, 1 every stage + the scanned-code counter, 2 the scan stage alone (gamma_hip_profile_enable)
    std::vector<StageEvent> events;
    std::vector<hipEvent_t> event_pool;
    double stage_ms[GAMMA_HIP_NUM_STAGES] = {0};
    int64_t stage_n[GAMMA_HIP_NUM_STAGES] = {0};
    int64_t scan_pairs = 0;
};

// a writer call: writer_mu (one writer at a time) + mu; exclusive() before memory that a search in flight may be
// reading is freed or moved: search_mu as well (no search can start), both streams drained
struct WriteLock final : ghi::DevExclusive {
    gamma_hip_index* h;
    std::unique_lock<std::mutex> w, s, m;
    explicit WriteLock(gamma_hip_index* h_) : h(h_), w(h_->writer_mu), s(h_->search_mu, std::defer_lock), m(h_->mu) {
        h->wl = this;
        h->write_gen++;   // (under mu: searches read it under mu)
    }
    ~WriteLock() { h->wl = nullptr; }
    hipError_t exclusive() override {
        if (!s.owns_lock()) {
            m.unlock();
            s.lock();
            m.lock();
        }
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->wstream);
        if (e == hipSuccess && h->side) e = hipStreamSynchronize(h->side);
        if (e == hipSuccess && h->side2) e = hipStreamSynchronize(h->side2);   // a deferred tie replay reads lists and rows
        return e;
    }
    // searches may start again (the writer keeps writer_mu + mu): after a step that only needed the device idle
    void shared() {
        if (s.owns_lock()) s.unlock();
    }
};

namespace ghi {

using H = gamma_hip_index;

// what DevArray::grow takes as "exclusive": the lock of the writer call under way (a call that holds none has no search
// beside it to wait for)
inline DevExclusive& writer_exclusive(H* h) {
    static struct : DevExclusive {
        hipError_t exclusive() override { return hipSuccess; }
    } nobody;
    return h->wl ? static_cast<DevExclusive&>(*h->wl) : nobody;
}

// The raw store towards a caller that holds several handles (gamma_hip_store.cpp; the group reaches them through its table,
// gamma_hip_group_rawshard.cpp).  raw_rows_check: the store's own acceptance predicate over n caller rows, nothing written --
// GAMMA_HIP_OK, or the refusal of the store's writers with their message (an fp32 store takes everything).  raw_same_rows: both
// stores hold rows of one element type and length, an sq8 store decoded through the same ranges (or neither has any yet).
int raw_rows_check(H* h, int64_t n, const float* vecs);
bool raw_same_rows(H* a, H* b);

// the raw store's rows as the kernels of every element type take them (kernels.h): base pointer, element type and, for an sq8
// store, the decode table
inline gh::RowsRef raw_rows_ref(const H* h) {
    return gh::RowsRef{h->raw.p, h->raw_et, h->raw_et == gh::ROW_SQ8 ? h->d_sq8_tab : nullptr};
}

// a search-type call: search_mu for the whole call, mu while it reads the handle and enqueues
struct SearchLock {
    std::unique_lock<std::mutex> s, m;
    explicit SearchLock(H* h) : s(h->search_mu), m(h->mu) {}
    void enqueued() {   // everything is on the stream: writers may go on while the call waits for the GPU
        if (m.owns_lock()) m.unlock();
    }
};

#define GH_CHECK(h, expr)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return e_ == hipErrorOutOfMemory ? GAMMA_HIP_ENOMEM : GAMMA_HIP_EDEVICE;       \
        }                                                                                  \
        if (const char* r_ = gh::launch_refused_take()) {   /* kernels.h: a launcher was handed a shape its callers rule out */ \
            (h)->err = std::string("internal: ") + r_;                                     \
            return GAMMA_HIP_EDEVICE;                                                      \
        }                                                                                  \
    } while (0)

#define GH_TRY(expr)                   \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != GAMMA_HIP_OK) return rc_; \
    } while (0)

inline int fail(H* h, int code, const char* msg) {
    h->err = msg;
    return code;
}

// a failed DevArray / DevColumns growth as the store's error: `who` names the store, `what` the step
inline int grow_fail(H* h, const char* who, hipError_t e, const char* what) {
    if (e == hipErrorOutOfMemory && !strcmp(what, "hipMalloc")) return fail(h, GAMMA_HIP_ENOMEM, (std::string(who) + ": out of memory").c_str());
    if (e == hipErrorOutOfMemory) return fail(h, GAMMA_HIP_ENOMEM, (std::string(who) + ": out of device memory (" + what + ")").c_str());
    h->err = std::string(who) + ": " + what + " failed: " + hipGetErrorString(e);
    return GAMMA_HIP_EDEVICE;
}
// one array through DevArray::grow on the writer stream, under the writer's lock
inline int grow_array(H* h, const char* who, DevArray& a, size_t need, size_t want, size_t keep, int fill = -1) {
    const char* what = "";
    const hipError_t e = a.grow(need, want, keep, fill, h->wstream, writer_exclusive(h), &what);
    return e == hipSuccess ? GAMMA_HIP_OK : grow_fail(h, who, e, what);
}

struct StageScope {
    H* h;
    int stage;
    bool count;   // false: add the time to the stage but do not count a new invocation
    hipEvent_t a = nullptr, b = nullptr;
    StageScope(H* h_, int st, bool count_ = true) : h(h_), stage(st), count(count_) {
        if (h->profile == 1 || (h->profile == 2 && st == GAMMA_HIP_STAGE_SCAN && count_)) {
            // events are recycled: creating / destroying two per stage and step costs the host
            // more than the stages' launches
            auto take = [&]() -> hipEvent_t {
                if (!h->event_pool.empty()) {
                    hipEvent_t e = h->event_pool.back();
                    h->event_pool.pop_back();
                    return e;
                }
                hipEvent_t e = nullptr;
                return hipEventCreate(&e) == hipSuccess ? e : nullptr;
            };
            a = take();
            b = take();
            if (!a || !b) {
                a = b = nullptr;
                return;
            }
            (void)hipEventRecord(a, h->stream);
        }
    }
    ~StageScope() {
        if (a && b) {
            (void)hipEventRecord(b, h->stream);
            h->events.push_back({stage, a, b, count});
        }
    }
};

inline int drain_events(H* h) {
    if (h->events.empty()) return GAMMA_HIP_OK;
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    for (auto& e : h->events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            h->stage_ms[e.stage] += ms;
            h->stage_n[e.stage] += e.count ? 1 : 0;
        }
        h->event_pool.push_back(e.a);
        h->event_pool.push_back(e.b);
    }
    h->events.clear();
    return GAMMA_HIP_OK;
}

inline double extend_coefficient(uint8_t t) { return 1.1 + kPI / 2 - atan((double)t); }

// A new version of the lists' (offset, length) tables: what the host mirror holds, copied through the
// version's pinned staging on the writer stream -- behind the data copies of the writer that calls this, so a
// search that uses the version finds the entries in place (publish after write, realtime_mem_data.cc:299-300).
// The slot that is overwritten was current NVER - 1 versions ago; the last search that read it is awaited first.
inline int publish_meta(H* h) {
    const int v = (h->cur_ver + 1) % H::NVER;
    if (h->rd_set[v]) GH_CHECK(h, hipStreamWaitEvent(h->wstream, h->rd_ev[v], 0));
    // the staging itself: free once the copies of the version's previous use are done (the writer stream is
    // drained at the end of every writer call, so they are)
    int64_t* po = reinterpret_cast<int64_t*>(h->pin_ver[v]);
    int* pl = reinterpret_cast<int*>(po + h->nlist);
    memcpy(po, h->h_list_off.data(), (size_t)h->nlist * sizeof(int64_t));
    memcpy(pl, h->h_list_len.data(), (size_t)h->nlist * sizeof(int));
    GH_CHECK(h, hipMemcpyAsync(h->d_ver_off[v], po, (size_t)h->nlist * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipMemcpyAsync(h->d_ver_len[v], pl, (size_t)h->nlist * sizeof(int), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipEventRecord(h->ver_ev[v], h->wstream));
    h->cur_ver = v;
    h->d_list_off = h->d_ver_off[v];
    h->d_list_len = h->d_ver_len[v];
    int mx = 0;
    for (int l = 0; l < h->nlist; l++) mx = std::max(mx, h->h_list_len[l]);
    h->max_list_len = mx;
    return GAMMA_HIP_OK;
}

// gamma_hip_store.cpp: the re-rank image's arrays hold `need` rows (the caller holds mu)
int rerank_image_reserve(H* h, int64_t need);

inline size_t field_elem_size(int dtype) {
    return dtype == GAMMA_HIP_FIELD_INT || dtype == GAMMA_HIP_FIELD_FLOAT ? 4 : 8;
}

}  // namespace ghi
