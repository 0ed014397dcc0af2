// kernels.h -- launch wrappers of the gfx950 kernels in kernels.hip (internal to
// libgamma_hip.so; the public surface is include/gamma_hip.h).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_plan.h"

namespace gh {

// A launcher that is handed a shape its callers are supposed to rule out does not abort the process (a database server's): it
// records what it refused, launches nothing, and the C-ABI entry point under way fails with GAMMA_HIP_EDEVICE and that text at
// its next GH_CHECK (gamma_hip_internal.h).  Thread-local: a call enqueues from one thread.
void launch_refused(const char* what);
const char* launch_refused_take();   // what was refused since the last take (nullptr: nothing), cleared


// once-per-device initialisation of a kernel attribute (hipFuncSetAttribute is per device; a process may hold handles
// on several): true the first time the calling thread's current device comes by
inline bool first_call_on_device(std::atomic<uint64_t>& done) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    return (done.fetch_or(bit) & bit) == 0;
}

constexpr int kMaxRange = 8;

// RangeQueryResult on device (table/range_query_result.h:53-67)
struct RangeDesc {
    const uint8_t* bitmap;
    int32_t min_doc, max_doc, min_aligned, b_not_in;
};

// numeric column predicate (IsInRange<T>, index/impl/gpu/gamma_index_ivfpq_gpu.cc:685-727)
constexpr int kMaxField = 8;
struct FieldDesc {
    const void* col;
    int64_t n;
    int32_t dtype, incl;   // incl: bit 0 include_lower, bit 1 include_upper
    int64_t lo_i, hi_i;
    double lo_f, hi_f;
};

// term filter on a STRING field (FilteredByTermFilter, index/impl/gpu/gamma_index_ivfpq_gpu.cc:727-762): the
// field's items (split at \001) are dictionary-encoded on the host; doc i holds tok[off[i] .. off[i + 1])
constexpr int kMaxTerm = 8, kMaxTermItems = 16;
struct TermDesc {
    const int64_t* off;
    const int32_t* tok;
    int64_t n;              // docs in the column
    int32_t op, n_items;    // FilterOperator (table/field_range_index.h:23): 0 And, 1 Or, 2 Not
    int32_t items[kMaxTermItems];   // -1: an item no doc has
};

// everything GammaSearchCondition::IsValid reads (common/gamma_common_data.h:99-108)
struct FilterDesc {
    const uint8_t* del_bitmap;
    int64_t del_bits;
    const int* vid2doc;      // VIDMgr::VID2DocID of multi-vector documents; nullptr: docid == vid
    int64_t n_vid2doc;
    int32_t has_range, n_range;
    RangeDesc range[kMaxRange];
    int32_t n_field, n_term;
    FieldDesc field[kMaxField];
    TermDesc term[kMaxTerm];
};

void launch_pairwise(hipStream_t s, bool l2, const float* x, int nq, int d, const float* y,
                     int64_t ny, float* out, int64_t ld_out);
// field / term clauses of f -> one bit per document id in [0, nbits) (out: ceil(nbits / 64) * 8 bytes); f must carry no
// range bitmaps, no delete bitmap and no vid -> doc map (it is evaluated on document ids)
void launch_filter_bitmap(hipStream_t s, const FilterDesc& f, int64_t nbits, uint8_t* out);
// every list cut down to the entries that pass ftab[0] (delete bitmap, superseded slots, every clause), in order,
// at the same offsets of (out_codes, out_ids); out_len: the new lengths
void launch_compact_lists(hipStream_t s, const int64_t* list_off, const int* list_len, int nlist, const uint8_t* codes,
                          const int64_t* ids, int code_size, const FilterDesc* ftab /* device */, uint8_t* out_codes,
                          int64_t* out_ids, int* out_len, const float* sums = nullptr, float* out_sums = nullptr);
void launch_pairwise_filtered(hipStream_t s, bool l2, const float* x, int nq, int d,
                              const float* y, int64_t ny, float* out, int64_t ld_out,
                              const FilterDesc& filt, float min_score, float max_score,
                              int64_t row_base);
// The element types of the raw store's rows (the integers of gamma_hip_raw_elem_type)
enum RowType : int { ROW_F32 = 0, ROW_F16 = 1, ROW_U8 = 2, ROW_I8 = 3, ROW_SQ8 = 4 };
inline size_t row_elem_bytes(int et) { return et == ROW_F32 ? 4 : et == ROW_F16 ? 2 : 1; }
// Rows of the raw store as every reader of more than fp32 rows takes them -- the flat and IVFFLAT scans, the exact re-rank, the
// tie replay: base pointer and element type.  A launcher that takes one does one switch (et) into its template on the row
// type (float, uint16_t, uint8_t, int8_t, sq8_t); the flat overloads launch, for ROW_F32, exactly what their float overloads launch.
// tab (ROW_SQ8 only): the store's decode table, d x {step[j], vmin[j]} -- per dimension, the same for every row.
struct RowsRef {
    const void* p = nullptr;
    int et = ROW_F32;
    const float* tab = nullptr;
    size_t esz() const { return row_elem_bytes(et); }
    RowsRef at(int64_t row, int d) const { return RowsRef{static_cast<const char*>(p) + (size_t)row * d * esz(), et, tab}; }
    template <class T> const T* as() const { return static_cast<const T*>(p); }
};
void launch_pairwise_filtered(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& y, int64_t ny, float* out,
                              int64_t ld_out, const FilterDesc& filt, float min_score, float max_score, int64_t row_base);
// Flat search with a running bound: candidate lists of the queries of one call
struct FlatEmit {
    const uint32_t* tau;        // [nq] key bound per query (0xff7fffff = anything valid)
    unsigned long long* cand;   // [nq][cap] (key << 32 | row id)
    int* cnt;                   // [nq * cstride] items appended (may exceed cap: overflow); query q's counter at q * cstride
    int cap;
    int cstride = 1;            // counters one 128-byte line apart (32): appends of different queries do not serialise on a line
};
bool pairwise_can_emit(int nq, int d, int64_t ny);
int flat_list_cap();
void launch_pairwise_emit(hipStream_t s, bool l2, const float* x, int nq, int d, const float* y, int64_t ny,
                          const FilterDesc& filt, float min_score, float max_score, int64_t row_base,
                          const FlatEmit& em);
void launch_pairwise_emit(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& y, int64_t ny,
                          const FilterDesc& filt, float min_score, float max_score, int64_t row_base, const FlatEmit& em);
// candidate lists from the first chunk's top-k (vals / positions inside the chunk starting at row r0)
void launch_flat_init(hipStream_t s, bool l2, const float* vals, const int* pos, int nq, int k, int64_t r0,
                      const FlatEmit& em, uint32_t* tau, int* kept = nullptr);   // kept: FlatLog::kept
// per query: keep the k best of its list (sorted), set the new bound; lists that overflowed set *overflow
// log (exact ties): what pass `pass` (1..) appended to a query's list, kept for the replay -- items [nq][nsl][cap] in the
// layout of the scan's survivor slices, counts [nq][nsl]; kept[nq]: list entries that are older than the pass
struct FlatLog {
    unsigned long long* items = nullptr;
    int* cnt = nullptr;
    int* kept = nullptr;
    int nsl = 0, pass = 0;
    unsigned long long* dbg = nullptr;   // GAMMA_HIP_COMPACT_DBG: phase clocks of query 0
};
void launch_flat_compact(hipStream_t s, int nq, int k, const FlatEmit& em, uint32_t* tau, int* overflow,
                         const FlatLog* log = nullptr);
// sorted lists -> distances / labels (neutral / -1 padded)
void launch_flat_final(hipStream_t s, bool l2, int nq, int k, const FlatEmit& em, float neutral, float* distances,
                       int64_t* labels);
void launch_row_norms(hipStream_t s, const float* y, int64_t n, int d, float* out);
// Flat search on the matrix pipe (flat_mfma.hip): a bf16 hi / lo filter with a proven margin + the survivors' exact
// distances -- appends to the FlatEmit lists exactly the items launch_pairwise_emit would append.
bool flat_filter_supported(int nq, int d, int64_t ny);
// rows of d elements have a filter kernel (whatever the switches and gates say): the padded length and the margin constant
int flat_filter_shape(int d, int* d_pad, float* margin);
bool flat_filter_new_shape(int d);   // served by k_flat_filter_any (neither a register-resident length nor d % 32 == 0 <= 1536)
int64_t flat_filter_pair_cap(int nq);
int flat_filter_counter_bytes();   // the pair list's counters (one per segment, a cache line apart): zeroed before a pass
size_t flat_filter_query_image_bytes(int nq, int d);
void launch_flat_prep_queries(hipStream_t s, const float* x, int nq, int d, void* image);
size_t flat_filter_bounds_bytes(int nq);
// survivors of the pass as (query, store row) pairs in any order: pairs [cap] of 8 bytes, *npairs appended (zeroed by the caller)
void launch_flat_filter(hipStream_t s, bool l2, int d, const void* qimage, const float* xn, const uint32_t* tau, float* bounds,
                        int nq, const float* y, int64_t ny, int64_t row_base, void* pairs, int* npairs, int64_t cap);
void launch_flat_exact(hipStream_t s, bool l2, const void* pairs, const int* npairs, int64_t cap, const float* x, int nq, int d,
                       const float* store, const FilterDesc& filt, float min_score, float max_score, const FlatEmit& em,
                       int* overflow);
// (rows of any element type; `store` is the store's row 0)
void launch_flat_filter(hipStream_t s, bool l2, int d, const void* qimage, const float* xn, const uint32_t* tau, float* bounds,
                        int nq, const RowsRef& y, int64_t ny, int64_t row_base, void* pairs, int* npairs, int64_t cap);
void launch_flat_exact(hipStream_t s, bool l2, const void* pairs, const int* npairs, int64_t cap, const float* x, int nq, int d,
                       const RowsRef& store, const FilterDesc& filt, float min_score, float max_score, const FlatEmit& em,
                       int* overflow);
// How the compiled reference's sgemm_ (MKL, the BLAS faiss links in the reference's build) sums the K dimension of
// exhaustive_L2sqr_blas's x . y^T (faiss:utils/distances.cpp:215-296), measured against the compiled library
// (oracle/gamma_oracle.c go_gemm_k_split, tests/test_oracle_vs_ref.py): K <= 384 -- one k-ascending fma chain per
// element, which is what v_mfma_f32_32x32x2_f32 computes; 384 < K <= 768 with K % 8 == 0 -- two chains, [0, K/2) and
// [K/2, K), each from zero, added once; beyond that MKL's blocking is not restated (one chain).  Returns the split
// point, 0 = none.  With it the GEMM-form coarse distances are the library's, bit for bit.
inline int gemm_k_split(int d) { return (d > 384 && d <= 768 && d % 8 == 0) ? d / 2 : 0; }
void launch_l2_gemmform(hipStream_t s, const float* x, int nq, int d, const float* y, int64_t ny,
                        const float* xn, const float* yn, float* out, int64_t ld_out,
                        bool use_mfma);
void launch_pq_ip_table(hipStream_t s, const float* x, int nq, int d, int M, const float* pqc,
                        float* out);
void launch_precompute_table(hipStream_t s, const float* cc, int nlist, int d, int M,
                             const float* pqc, float* out);
// per-call state cleared by the pair-offset kernel (one byte and one 8-byte word per query, two counters); null = skip
struct PairZero {
    uint8_t* bytes = nullptr;
    unsigned long long* words = nullptr;
    int* count_a = nullptr;
    int* count_b = nullptr;
    int* count_c = nullptr;
    // histogram pass of the grid-wide query order (launch_query_order with hist_done): list_rank, qkey[nq], bins
    const int* qo_rank = nullptr;
    int* qo_key = nullptr;
    int* qo_bins = nullptr;
};
void launch_pair_offsets(hipStream_t s, const int* probe_list, int nq, int P, const int* list_len,
                         const uint8_t* list_mask, int nlist, int* pair_off, int* q_total,
                         unsigned long long* scan_codes, const int64_t* list_off = nullptr,
                         int64_t* pair_base = nullptr, const PairZero* zero = nullptr);
void launch_compact_probes(hipStream_t s, const int* probe_in, const float* cdis_in, int nq, int P,
                           const int* list_len, const uint8_t* list_mask, int nlist, int* probe_out,
                           float* cdis_out, int P_out = 0);   // P_out: row length of the output (0: P)
// two-phase shard search: the producers' bounds as floats (+-inf: none) for the reduction across shards, and back
void launch_bound_export(hipStream_t s, bool l2, const unsigned long long* ready, int nq, float* out);
void launch_bound_import(hipStream_t s, bool l2, const float* in, int nq, unsigned long long* ready);
void launch_fill_f32(hipStream_t s, float* p, int n, float v);
void launch_bound_combine(hipStream_t s, float* acc, const float* in, int n, int take_max);
// inner-product scan: dis0[q][p] = <x_q, centroid of probe p> (fvec_inner_product order); the scan takes it
// through its coarse_dis argument
void launch_pair_ip(hipStream_t s, const float* x, const float* cc, const int* probe_list, int nq, int P, int d,
                    int nlist, float* out);
// threshold pre-filter of the scan (kernels.hip, k_ivfpq_scan_pair<.., FILT>)
struct ScanBound {
    unsigned long long* ready;  // [nq] 0 = not yet published; (1 << 32 | key bound) = bound valid;
                                // (2 << 32) = no bound (unfiltered selection); zeroed per launch
    unsigned long long* surv;   // [nq][groups][scan_slice_cap()] candidates within the bound, per workgroup,
                                // as (key << 32 | position in the query's segment)
    int* gcnt;                  // [nq][groups] items per slice; > scan_slice_cap() = overflowed
    int K;                      // recall_num
    int cnt_stride;             // gcnt[q * cnt_stride + group]  (groups of this launch; more with pair slices behind)
    int store_all;              // != 0: consumer groups store their distances even with a bound (exact-ties replay)
    int* rq_list;               // queries k_select_final could not finish from the slices (launch_ivfpq_scan_repair)
    int* rq_count;
    const float* sums;          // filter pass of the L2 consumers (k_ivfpq_scan_pair<.., CF>): per arena entry
                                // sum_m T2[list][m][code[m]]; per list sum_m max_c |T2[l][m][c]|.  nullptr: regular loop
    const float* t2max;
    int cf_span;                // filter pass: probes per consumer group behind the producer's G (0: one consumer takes them all)
    unsigned long long* timeouts;   // consumers that gave up waiting (diagnostics; may be nullptr)
    int slice_cap;              // items a slice holds: scan_slice_cap(K)
    int part;                   // two-phase shard search: 1 = only the producers of this launch work (the consumers leave at once),
                                // 2 = only the consumers (the bounds are in `ready` already: imported after the reduction across shards)
    int dbg_part;               // timing experiments only (GAMMA_HIP_SCAN_PART): 1 = consumers leave at once, 2 = producers do
    int c8;                     // != 0 (filter-pass launches only): the consumers' filter pass gathers from a BYTE image of the query's
                                // table made in the workgroup (2-way bank conflicts at most instead of ~3.5); candidates as ever
    const int64_t* pair_base;   // filter pass: [nq][P] arena offset of the pair's list (k_pair_offsets) -- with pair_off the pass needs no
                                // look-up through the list id in front of a list
    float t2max_all;            // filter pass: max over t2max (the margin's bound S without a look-up per list)
};
// ---- q8scan.hip: the consumer probes of a bounded L2 scan, list-major over byte tables (one list x 8 queries per tile) ----
struct Q8Args {
    int nq, P, G, M, nlist;
    double mean_len;                  // codes per list (short lists take the pipelined filter kernel)
    const int* probe_list;            // [nq][P]
    const float* coarse_dis;          // [nq][P] dis0
    const float* st2;                 // [nq][M][256] fp32 inner-product tables (k_pq_ip_table)
    const float* pqc = nullptr;
    int d = 0;
    const float* xd = nullptr;        // != nullptr (with pqc, d): k_q8_exact computes the table entries of a query's candidates on
                                      // demand when they are few -- the queries [nq][d]
    const float* T2;                  // [nlist][M][256]
    const float* t2max;               // [nlist]
    const float* sums;                // per arena entry: sum_m T2[list][m][code[m]]
    const uint8_t* codes;
    const int64_t* ids;
    const int64_t* list_off;
    const int* list_len;
    const uint8_t* list_mask;
    const int* pair_off;              // [nq][P + 1]
    const unsigned long long* ready;  // [nq] the producers' bounds
    const FilterDesc* ftab;           // entry 0: the call's validity predicate (need_ids)
    int need_ids;
    unsigned long long* surv;         // survivor slices [nq][cnt_stride][slice_cap]; slices 1 .. of the consumer probe groups are written here
    int* gcnt;
    int cnt_stride, slice_cap;
    int* rq_list;                     // queries without a bound are appended (their consumer groups are scored by the repair launch)
    int* rq_count;
    uint8_t* q8;                      // workspace [nq][M][256]
    float4* meta;                     // workspace [nq]
    uint32_t* cand;                   // workspace [nq][q8_cand_cap(nq)]
    int* iwork;                       // workspace q8_int_words(..) ints
};
int q8_cand_cap(int nq);
size_t q8_int_words(int nq, int P, int G, int nlist);
void launch_q8_consumers(hipStream_t s, const Q8Args& a);
// (scan_slice_cap, scan_cf_applies, scan_group_size, q8_supported: scan_plan.h)
// One launch of the list scan.  The first block is the same for every launch of a call (gamma_hip_search.cpp scan_args);
// a call site sets what it means in the second.
struct ScanArgs {
    bool l2 = true;
    const float* x = nullptr;
    int nq = 0, d = 0, M = 0, P = 0;
    const int* probe_list = nullptr;
    const float* coarse_dis = nullptr;   // dis0 of every (query, probe) pair
    const float* cc = nullptr;
    const float* st2 = nullptr;
    const float* T2 = nullptr;
    const int64_t* list_off = nullptr;
    const int* list_len = nullptr;
    const uint8_t* list_mask = nullptr;
    int nlist = 0;
    const uint8_t* codes = nullptr;
    const int64_t* ids = nullptr;
    const int* pair_off = nullptr;
    int64_t q_stride = 0;
    float* out = nullptr;
    const FilterDesc* ftab = nullptr;   // device
    const int* qfil = nullptr;          // device, may be null
    int need_ids = 0;
    int G = 1;
    const int* qperm = nullptr;
    int pg_lo = 0, pg_cnt = 0, sparse = 0;
    const ScanBound* bound = nullptr;
    const float* pqc_fused = nullptr;                       // != nullptr: query table computed in the kernel
    const int* rq_list = nullptr, *rq_count = nullptr;      // repair launch (scan.hip)
    int chunk_len = 0, max_units = 0;                       // > 0: rq_list is a work list of list chunks (scan.hip)
};
void launch_ivfpq_scan_pair(hipStream_t s, const ScanArgs& a);
int query_order_bins();
bool query_order_grid(int nq);   // the batch is sorted over the whole grid (needs bins)
// bins: 2 * query_order_bins() ints (histogram | cursors) for the grid-wide sort of large batches; the histogram half is
// zero on entry and left zero.  hist_done: qkey and the histogram were filled by the pair-offset kernel (PairZero::qo_*)
void launch_query_order(hipStream_t s, const int* probe_list, int nq, int P, const int* list_rank,
                        int nlist, int* qkey, int* qperm, int* bins = nullptr, bool hist_done = false);
void launch_sum_totals(hipStream_t s, const int* q_total, int nq, unsigned long long* acc);
// list shard over a supplied assignment: out_max[0] = the longest candidate row of the batch over the lists scanned here,
// out_max[1] = the most owned, non-empty probes of any query (TWO words)
void launch_max_local_total(hipStream_t s, const int* probe_list, int nq, int P, const int* list_len,
                            const uint8_t* list_mask, int nlist, int* out_max);
int select_kpad(int K);
// coarse quantizer selection (ties at the K-th distance resolved like the reference's heap); tie_flag: nq bytes
// coarse.hip: coarse quantizer of a large batch without the distance matrix (sample -> bound -> filtered GEMM
// epilogue -> merge; see the file header).  ws: pl.bytes of scratch.
constexpr int kCoarseCap = 128, kCoarseRepairGrid = 256;
struct CoarseFusedPlan {
    int sample, nseg, tiles_per_strip, cap, cap_stride;
    size_t off_mat, off_tau, off_cand, off_cnt, off_ovf, off_scratch, off_full, bytes;
};
// bf16 filter of the fused path (coarse.hip, "bf16 filter"): |L~ - exact| margin c (xn + yn), and the magnitude domain
// of its derivation; queries outside it go to the repair list, an index with a centroid outside it keeps the fp32 filter
constexpr float kCoarseBfMargin = 1.220703125e-4f;     // c = 2^-13
constexpr float kCoarseBfXnMin = 5.421010862427522e-20f;    // 2^-64  <= |x|^2
constexpr float kCoarseBfNormMax = 1.329227995784916e+36f;  // 2^120  >= |x|^2, |y|^2
struct CoarseBf16 {
    const void* img;             // launch_coarse_image
    const float* hc;             // (1 - c) |y|^2 per image column
    float yn_max;                // largest centroid norm
    unsigned long long* stat;    // {queries the bf16 chain gave up on, queries}, cumulative
};
size_t coarse_image_bytes(int d, int nlist);
bool coarse_image_supported(int d, int nlist);
void launch_coarse_image(hipStream_t s, const float* y, const float* yn, int nlist, int d, void* image);
bool coarse_fused_supported(int nq, int d, int nlist, int P, bool exact_ties = false);
CoarseFusedPlan coarse_fused_plan(int nq, int nlist, int P, int cap, bool exact_ties = false);
// rows[0] distance rows mat[i][0..nlist) of the queries rows[1 + i], each walked through faiss's result heap
// (select.hip k_coarse_heap_fix): the K nearest in the reference's order, ties included
void launch_coarse_heap_rows(hipStream_t s, const float* mat, int nlist, int nq, int K, const int* rows, float* out_vals,
                             int* out_pos, unsigned long long* tie_stats);
void launch_coarse_fused(hipStream_t s, const CoarseFusedPlan& pl, void* ws, const float* x, int nq, int d,
                         const float* y, int nlist, const float* yn, int P, float* out_dis, int* out_idx,
                         bool exact_ties = false, unsigned long long* tie_stats = nullptr,
                         hipStream_t side = nullptr, hipEvent_t fork = nullptr, hipEvent_t join = nullptr,
                         const CoarseBf16* bf = nullptr);   // bf: the filter launch on the bf16 pipe
// small batches: exact coarse distances [nq][nlist] + inner-product tables [nq][M][256] in one launch; false = shape
// not covered (nq > 16), nothing launched
bool launch_small_coarse_ip(hipStream_t s, const float* x, int nq, int d, const float* cc, int nlist, float* mat, int M,
                            const float* pqc, float* st2, int* zero_me = nullptr);
// small batches (select.hip): coarse top-nprobe + slab offsets in one kernel; ADC top-recall_num + ids + exact
// re-rank + top-k + output in one kernel.  P <= 64, R <= 1024.
// pair_ip != nullptr (inner-product metric): also dis0 = <x_q, centroid> of every probe in fvec_inner_product order
void launch_small_coarse_select(hipStream_t s, const float* mat, int nlist, int nq, int P, float* out_vals, int* out_pos,
                                const int* list_len, const uint8_t* list_mask, const int64_t* list_off, int* pair_off,
                                int* q_total, int64_t* pair_base, const float* x = nullptr, const float* cc = nullptr,
                                int d = 0, float* pair_ip = nullptr, uint32_t* units = nullptr, int* unit_count = nullptr,
                                int chunk_len = 0, int exact_ties = 0, unsigned long long* tie_stats = nullptr);
struct TieReplayArgs;   // below
void launch_small_tail(hipStream_t s, bool l2, const float* slab, int64_t q_stride, const int* q_total, int nq, int R, int P,
                       const int* probe_list, const int* pair_off, const int64_t* list_off, const int64_t* ids,
                       float* cand_dis, int* cand_pos, int64_t* cand_ids, int has_rank, const float* x, int d,
                       const float* raw, int64_t nraw, int k, float min_score, float max_score, float neutral,
                       float* distances, int64_t* labels, int smax = 0, float* pre_val = nullptr, int* pre_pos = nullptr,
                       int fixed_n = 0,    // q_total == nullptr (flat search): every row has fixed_n entries, position = vector id
                       const TieReplayArgs* tr = nullptr,   // exact ties: a query with a tie at a cut is replayed in the kernel
                       unsigned long long* tie_stats = nullptr);
// IVFFLAT: exact distances of every entry of the probed lists (rows from the raw store) into the query's slab
void launch_ivfflat_scan(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                         const int64_t* pair_base, const int64_t* ids, const float* raw, int64_t nraw, int64_t q_stride,
                         float* out, const FilterDesc* ftab, int need_filter, float min_score, float max_score);
// ... over rows of any element type (a narrow row widens to fp32 exactly on load, an sq8 code is decoded with raw.tab); element
// type 0 forwards to the launch above; the same for launch_ivfflat_lm below
void launch_ivfflat_scan(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                         const int64_t* pair_base, const int64_t* ids, const RowsRef& raw, int64_t nraw, int64_t q_stride,
                         float* out, const FilterDesc* ftab, int need_filter, float min_score, float max_score);
// IVFFLAT, list-major (ivfflat.hip): one workgroup per list, every query probing it run past the list's rows
bool ivfflat_lm_supported(int d);
// the list-major form of rows of d floats: *kind 0 = none (the pair kernel), 1 = fixed-length (k_ivfflat_lm: the whole row in
// registers, d in {16, 32, 64, 96, 128}), 2 = row-sliced (k_ivfflat_lms: every other d % 16 == 0 up to 4096); *slab = the
// elements of a row a pair of threads holds at a time, *qtile = the queries per LDS tile (both 0 with kind 0).  Returns kind.
int ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile);
size_t ivfflat_lm_scratch_bytes(int nq, int P, int nlist);
void launch_ivfflat_lm(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                       const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const float* raw,
                       int64_t nraw, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter, float min_score,
                       float max_score, void* scratch);
void launch_ivfflat_lm(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                       const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const RowsRef& raw,
                       int64_t nraw, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter, float min_score,
                       float max_score, void* scratch);
// The three scans over the fp32 rows of a SPARSE store (gamma_hip_raw_put: a list shard's own rows): slot [nslot] = vector id ->
// row of `raw` (nraw rows), -1 = not held here; an entry without a row here gets the sentinel and nothing is read through it.
// Kernels of their own (the sparse instantiation of each scan's body): the launches above are untouched.  slot == nullptr (a
// store that never took a row): nothing is launched -- the caller fills the slab with the sentinel.
void launch_ivfflat_scan_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                                const int64_t* pair_base, const int64_t* ids, const float* raw, int64_t nraw, const int32_t* slot,
                                int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab, int need_filter,
                                float min_score, float max_score);
void launch_ivfflat_lm_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                              const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const float* raw,
                              int64_t nraw, const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                              int need_filter, float min_score, float max_score, void* scratch);
// ... over the rows of a sparse store of any element type but sq8 (float16 / uint8 / int8 rows widen exactly on load: the same
// bodies, instantiated per type); element type 0 launches the kernels of the two launches above
void launch_ivfflat_scan_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* pair_off,
                                const int64_t* pair_base, const int64_t* ids, const RowsRef& raw, int64_t nraw,
                                const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                                int need_filter, float min_score, float max_score);
void launch_ivfflat_lm_sparse(hipStream_t s, bool l2, const float* x, int nq, int d, int P, const int* probe, const int* pair_off,
                              const int64_t* list_off, const int* list_len, int nlist, const int64_t* ids, const RowsRef& raw,
                              int64_t nraw, const int32_t* slot, int64_t nslot, int64_t q_stride, float* out, const FilterDesc* ftab,
                              int need_filter, float min_score, float max_score, void* scratch);
// out[l] = mask[l] ? list_len[l] : 0 -- the list-length table of a list shard: to the list-major launch an unowned list is empty
void launch_masked_list_len(hipStream_t s, const int* list_len, const uint8_t* mask, int nlist, int* out);
// returns true when the walk of the tied rows went to `side` (the caller then waits for `join` before reading the result)
bool launch_coarse_select(hipStream_t s, const float* mat, int nlist, int nq, int K, float* out_vals, int* out_pos,
                          uint8_t* tie_flag, unsigned long long* tie_stats = nullptr, hipStream_t side = nullptr,
                          hipEvent_t fork = nullptr, hipEvent_t join = nullptr);
// the rows a launch works on, as a list written on the device (k_select_final's fall-through list: a handful of a batch's
// queries): the grid is a small cap -- row_list_grid -- whose workgroups / waves stride over the list.  Empty: every row.
struct RowList {
    const int* rows = nullptr;
    const int* count = nullptr;
    RowList() = default;
    RowList(const int* r, const int* c) : rows(r), count(c) {}
    explicit operator bool() const { return rows != nullptr; }
};
inline int row_list_grid(int nrows) { return nrows < 256 ? nrows : 256; }   // (one workgroup per compute unit)
// what a listed launch of the selection does for a row once it is selected, in the same workgroup (the two launches that
// followed it over the same handful of rows): whether the cut went through a group of equal values (launch_flag_cut_ties;
// tflag null: skipped) and the candidates' ids (launch_map_candidates)
struct RowTail {
    uint8_t* tflag = nullptr;
    int P = 0;
    const int* probe_list = nullptr;
    const int* pair_off = nullptr;
    const int64_t* list_off = nullptr;
    const int64_t* ids = nullptr;
    int64_t* cand_ids = nullptr;
};
void launch_select_topk(hipStream_t s, bool smallest, const float* vals, int64_t seg_stride,
                        const int* seg_len, int fixed_len, int max_len, int nseg, int K,
                        float* out_vals, int* out_pos, RowList only = {}, const RowTail* tail = nullptr);
// threshold pre-filter of the scan: exact top-K from the survivor lists (select.hip); rows that end
// with flag != 0 are appended to fl_list and left to launch_select_topk(..., only = {fl_list, fl_count})
void launch_select_final(hipStream_t s, bool smallest, const unsigned long long* surv, const int* gcnt,
                         int nslices, int slice_cap, const unsigned long long* ready, const int* pair_off, int P,
                         int nq, int K, const int64_t* pair_base, const int64_t* ids, uint8_t* flag, float* out_vals,
                         int* out_pos, int64_t* out_ids, uint8_t* cut_tie = nullptr,
                         unsigned long long* tie_stats = nullptr, int* rq_list = nullptr, int* rq_count = nullptr, unsigned long long* bound_stat = nullptr,
                         int* fl_list = nullptr, int* fl_count = nullptr);
// (surv: [nq][nslices][slice_cap] items, slice g of query q at (q * nslices + g) * slice_cap -- the kernels request a slice's
//  first blocks before they know its count, so every slice must be allocated in full; P >= 1 and slice_cap >= 1.
//  cut_tie[q] = 1: the K-th and (K+1)-th keys are equal)
void launch_map_candidates(hipStream_t s, const int* pos, int nq, int R, int P,
                           const int* probe_list, const int* pair_off, const int64_t* list_off,
                           const int64_t* ids, int64_t* cand_ids);
// The exact re-rank over rows of any element type: the exact distance is that of the fp32 query and the widened (sq8: decoded
// through raw.tab in front of the fma chain) row in the same operation order.  How a row is loaded depends on its type and d
// (rerank_dev.h): float16 rows with d % 8 == 0 with one 16-byte load per lane, every other d with 2-byte loads; byte and sq8 rows
// with d % 16 == 0 with 16-byte loads, d % 4 == 0 with dword loads, every other d with byte loads.
// slot / nslot: the vid -> row table of a sparse store (below), rows of any element type.
void launch_rerank_dist(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& raw,
                        int64_t nraw, const int64_t* cand_ids, int R, float min_score,
                        float max_score, float* out, const int32_t* slot = nullptr, int64_t nslot = 0);
// raw vectors sharded with their lists (round 6).  slot [nslot]: vector id -> row of `raw` on THIS shard, -1 = held elsewhere.
// _export_exact: ex[f][j] = exact distance (no score window) of entry j of exported stream row f when its ADC value is
// within bound[f] and its vector is held here, NaN otherwise (raw: the sparse store's rows, of any element type).
// _lookup_exact: cand_exact[q][r] = the exact distance that travelled with candidate cand_ids[q][r] in one of the W shard
// tables (all_ids / all_exact [W][nq][R]), sentinel if none.
void launch_export_exact(hipStream_t s, bool l2, const float* xf, int nf, int d, const RowsRef& raw, const int32_t* slot, int64_t nslot,
                         const float* vals, const int64_t* ids, int64_t stride, const int32_t* off, int P, const float* bound, float* ex);
void launch_lookup_exact(hipStream_t s, bool l2, const float* all_dis, const int64_t* all_ids, const float* all_exact, int W, int nq, int R,
                         int q0, int nql, const float* cand_dis, const int64_t* cand_ids, float* cand_exact);
// Exact-tie bookkeeping (ties.hip, gamma_hip_set_exact_ties).  cut[q] != 0: the top-recall_num cut of query q
// went through a group of equal ADC distances (set by the selection kernels).  The final-stage kernels add
// their own condition -- two of the first k+1 final distances equal -- and append every query either one
// holds for to list[*count]; launch_tie_replay then redoes those queries the way the reference's heaps do.
// stats: device counters {coarse rows redone, cut ties, queries replayed}, accumulated over calls.
struct TieFlags {
    const uint8_t* cut = nullptr;
    int* list = nullptr;     // nullptr: exact ties off
    int* count = nullptr;
    unsigned long long* stats = nullptr;
};
// (rows of any element type, as launch_rerank_dist takes them)
void launch_rerank_topk(hipStream_t s, bool l2, const float* x, int nq, int d, const RowsRef& raw,
                        int64_t nraw, const int64_t* cand_ids, int R, int k, float min_score,
                        float max_score, float neutral, float* distances, int64_t* labels,
                        const int* qperm = nullptr,   // qperm: run the queries in this order (speed only)
                        const TieFlags* ties = nullptr);
// rerank_filter.hip: the same re-rank over a dense fp32 store with a one-byte image of its rows in front -- most candidates are
// proven out of the first k + 1 from the image, the survivors get launch_rerank_topk's arithmetic.  Same outputs, same flags.
// The margin of the bound (derivation: the file's header) and the longest row the kernel stages.
constexpr float kRerankFilterMargin = 3.0517578125e-05f;   // M = 2^-15
constexpr int kRerankFilterMaxD = 1536;
constexpr int kRerankFilterStatLines = 64;
inline size_t rerank_filter_stat_bytes() { return (size_t)kRerankFilterStatLines * 16 * sizeof(unsigned long long); }
bool rerank_filter_shape_ok(int d, int R, int k);   // d % 16 == 0, d <= kRerankFilterMaxD, R <= 1024, min(k + 1, R) <= 64
inline size_t rerank_image_par_bytes(int d) { return ((size_t)3 * d + 2) * sizeof(float); }
// par (rerank_image_par_bytes): the image's parameters from the n rows present -- lo[d], Delta, |lo| -- all on the device
void launch_rerank_image_params(hipStream_t s, const float* rows, int64_t n, int d, float* par);
// image rows (img: u8[d], aux: {err, nrm} each) of the store's rows first + i, or vids[i] (outside [0, nrows): skipped), i < n
void launch_rerank_image_rows(hipStream_t s, const float* rows, const int64_t* vids, int64_t first, int64_t n, int d, const float* par,
                              uint8_t* img, float* aux, int64_t nrows);
// The wave form (k_rerank_topk_filt_wave: one wave per query, no workgroup barrier) takes d == 128, R <= 256, min(k + 1, R) <= 64
bool rerank_filter_wave_ok(int d, int R, int k);
// Automatic dispatch takes the wave form from this many queries on.  A wave walks its query's chain alone, so a call that fills
// the device with waves only thinly is quicker with a workgroup's 256 threads per query (DESIGN.md section 31 has the measurement).
// The one place the number stands: gamma_hip_rerank_filter_form reports it.
constexpr int kRerankWaveAutoMinNq = 4096;
// stat: kRerankFilterStatLines x 16 words; the queries add their survivors to word 0 of a line each (the sum is the count)
// form (gamma_hip_set_rerank_filter_form): 0 = automatic, the wave form where rerank_filter_wave_ok holds and the call has enough
// queries to fill the device with waves (kRerankWaveAutoMinNq); 1 = the workgroup kernel always; 2 = the wave
// form wherever rerank_filter_wave_ok holds.
// Returns the form it launched (1 workgroup kernel, 2 wave form), 0 when it launched nothing.
int launch_rerank_topk_filtered(hipStream_t s, bool l2, const float* x, int nq, int d, const float* raw, int64_t nraw, const uint8_t* img,
                                 const float* aux, const float* par, const int64_t* cand_ids, int R, int k, float min_score,
                                 float max_score, float neutral, float* distances, int64_t* labels, const int* qperm,
                                 const TieFlags* ties, unsigned long long* stat, int form = 0);
// what k_tie_replay needs to redo one query (ties.hip)
struct TieReplayArgs {
    const int* list;              // flagged queries, *count of them
    const int* count;
    int nq;
    const float* slab;            // ADC distances [nq][q_stride] in scan order, +-inf = filtered entry
    int64_t q_stride;
    const int* pair_off;          // [nq][P + 1]
    const int64_t* pair_base;     // [nq][P] arena offset of each probed list
    const int64_t* ids;           // list arena
    int P, G;                     // probes per query; probes of the first group (bounded scan)
    const unsigned long long* ready;   // bounded scan (may be null): bound word, survivor slices, counts
    const unsigned long long* surv;
    const int* gcnt;
    int nsl, slice_cap;
    const float* x;               // queries [nq][d]
    int d;
    RowsRef rows;                 // raw vectors (has_rank), of any element type: launch_tie_replay takes the kernels of rows.et;
                                  // the small-batch tail (launch_small_tail) replays over fp32 rows only
    int64_t nraw;
    const float* ex_slab = nullptr;   // raw vectors sharded with their lists (round 6): the exact distance of stream entry ps
                                      // travelled with the shards' exports -- [rows][q_stride] like the slab, NaN where a shard
                                      // did not compute it; read instead of the raw row
    int* ex_missing = nullptr;        // counts R-heap members whose exact distance was NOT exported (must stay 0)
    int R, k, has_rank;
    float min_score, max_score, neutral;
    float* cand_dis;              // [nq][R] recall-stage table, rewritten for the replayed queries
    int64_t* cand_ids;
    float* distances;             // [nq][k]
    int64_t* labels;
    unsigned long long* dbg = nullptr;   // phase clocks of the first replayed query (GAMMA_HIP_TIE_DBG)
    int pop_push = 0;             // the heap takes a candidate with heap_pop + heap_push (IVFFLAT / flat scanners) instead
                                  // of heap_replace_top (the IVFPQ scanner)
    int fixed_n = 0;              // pair_off == nullptr (flat): every row has fixed_n entries, a position IS the vector id
    int compact_rows = 0;         // slab row i belongs to the i-th flagged query (list[i]) instead of query i
    int always_sliced = 0;        // ready == nullptr: every query is first G slab entries + slices 1.. (flat search with the
                                  // running bound: first row chunk + the candidates each later pass emitted)
};
int tie_replay_max_k();
int tie_small_max_k();
void launch_tie_list(hipStream_t s, const uint8_t* cut, const uint8_t* extra, int nq, int* list, int* count,
                     unsigned long long* tie_stats);
// test hook: one stream through one heap with each form of the sifts (ties.hip)
void launch_debug_heap_stream(hipStream_t s, int op, int k, int n, const float* vals, uint2* out_arr, uint2* out_sorted);
int tie_replay_max_probes();
void launch_tie_replay(hipStream_t s, bool l2, const TieReplayArgs& a);
void launch_flag_cut_ties(hipStream_t s, const float* slab, int64_t q_stride, const int* q_total, int nq, int K,
                          const float* sel_vals, const int* sel_pos, uint8_t* tflag,
                          int fixed_n = 0, int inside = 0);   // q_total == nullptr: rows of fixed_n entries; inside: also
                                                              // equal values among the selected K
int coarse_heap_max_k();
size_t tie_replay_lds_bytes(int R, int k, int P);
// flat search under exact ties: the chunked paths run for k + 1 results; this copies the first k to the caller's rows and
// lists the queries with two equal distances among the k + 1 (their order, or which of them stays, is the heap's)
void launch_flat_take_flag(hipStream_t s, const float* D1, const int64_t* I1, int nq, int k, float* distances, int64_t* labels,
                           int* list, int* count, unsigned long long* tie_stats);
// exact ties across list shards (ties.hip): cut-tie flags of the merged tables, a shard's export of the flagged queries'
// candidate streams, the owner's assembly of the exports
void launch_flag_merge_cut(hipStream_t s, const float* all_dis, int W, int nq, int R, int q0, int nql, const float* merged,
                           const int64_t* merged_ids, uint8_t* tcut, const uint8_t* shard_flags = nullptr);
void launch_shard_export(hipStream_t s, const int32_t* probe, int nf, int P, const int* list_len, const int64_t* list_off,
                         const uint8_t* list_mask, int nlist, const int64_t* ids, const float* slab, int64_t q_stride,
                         int64_t stride, float* vals, int64_t* out_ids, int32_t* off);
void launch_shard_export_rows(hipStream_t s, const int32_t* probe, int nf, int P, const int* list_len, const uint8_t* list_mask,
                              int nlist, int* max_entries);
void launch_merge_streams(hipStream_t s, int W, int nf, int P, int64_t stride, int64_t mstride, const float* vals, const int64_t* ids,
                          const int32_t* off, float* m_vals, int64_t* m_ids, int32_t* m_off, int64_t* m_base, float sentinel);
void launch_gather_words(hipStream_t s, const void* src, const int* list, int n, int words, void* out);
// out[i] = x[list[i]] for i < n (rows of d floats)
void launch_gather_rows(hipStream_t s, const float* x, const int* list, int n, int d, float* out);
void launch_finalize_topk(hipStream_t s, const float* sel_vals, const int* sel_pos, int nq, int k,
                          const int64_t* src_ids, int64_t src_stride, int64_t id_base,
                          float neutral, float* distances, int64_t* labels);
void launch_finalize_norank(hipStream_t s, const float* cand_dis, const int64_t* cand_ids, int nq,
                            int R, int k, float min_score, float max_score, float neutral,
                            float* distances, int64_t* labels, const TieFlags* ties = nullptr);
void launch_gather_shards(hipStream_t s, const float* all_dis, const int64_t* all_ids, int nshards,
                          int nq, int R, float* dis, int64_t* ids, float sentinel);
// one-kernel merge of the shard tables [W][nq][R] for queries [q0, q0 + nql) -> [nql][R]; false = shape
// not covered (R > 256 or W * R > 2048), use launch_gather_shards + launch_select_topk + launch_take_ids
bool launch_merge_shards(hipStream_t s, bool smallest, const float* all_dis, const int64_t* all_ids, int W,
                         int nq, int R, int q0, int nql, float* out_dis, int64_t* out_ids);
void launch_take_ids(hipStream_t s, const int* pos, const int64_t* src_ids, int64_t src_stride,
                     int nq, int R, int64_t* out);
void launch_bitmap_set(hipStream_t s, uint8_t* bm, const int64_t* docids, int64_t n, int64_t nbits,
                       int value);
void launch_mark_moved(hipStream_t s, int64_t* ids, int64_t pos);
// sparse raw store: pairs [n][2] = (vector id, row); the vid -> row table's entries, and the staged rows into their rows
void launch_raw_slot_scatter(hipStream_t s, const int32_t* pairs, int64_t n, int32_t* tab, int64_t ntab);
void launch_raw_rows_scatter(hipStream_t s, const float* stage, const int32_t* pairs, int64_t n, int d, float* raw, int64_t cap);
// narrow raw store: n staged fp32 rows (checked by the host) into rows first + i, or vids[i] (outside [0, nrows): skipped), of
// `raw` (nrows rows of element type et): rounded to binary16 (ROW_F16), converted exactly (ROW_U8 / ROW_I8: every value is
// storable) or encoded with enc = d x {inv[j], vmin[j]} (ROW_SQ8: every value is finite; enc is unread otherwise).  ROW_F32 is
// refused: fp32 rows are copied, not converted.
void launch_raw_rows_narrow(hipStream_t s, const float* stage, const int64_t* vids, int64_t first, int64_t n, int d, void* raw, int et,
                            const float* enc, int64_t nrows);
// mm[j], mm[d + j] = minimum, maximum of dimension j over n staged rows; first: mm is replaced, else folded in
void launch_sq8_minmax(hipStream_t s, const float* x, int64_t n, int d, float* mm, bool first);
void launch_list_checksum(hipStream_t s, const uint8_t* codes, const int64_t* ids, const int64_t* off, const int* len, int nlist,
                          int M, int max_len, unsigned long long* out);
void launch_repack_lists(hipStream_t s, const uint8_t* oc, const int64_t* oi, uint8_t* nc, int64_t* ni,
                         const int64_t* old_off, const int64_t* new_off, const int* len, int nlist, int M,
                         int max_len);
// per-code table sums of the L2 scan's filter pass and the per-list bound of their magnitude (kernels.hip)
void launch_code_sums_ranges(hipStream_t s, const float* T2, const uint8_t* codes, int M, const int* list_no, const int64_t* pos,
                             const int* n, int nranges, int max_n, float* sums);
void launch_code_sums_one(hipStream_t s, const float* T2, const uint8_t* codes, int M, int list_no, int64_t pos, int n,
                          float* sums);
void launch_code_sums_lists(hipStream_t s, const float* T2, const uint8_t* codes, int M, const int64_t* list_off,
                            const int* list_len, int nlist, int max_len, float* sums);
void launch_t2_rowmax(hipStream_t s, const float* T2, int nlist, int M, float* t2max);
void launch_centroid_update(hipStream_t s, const float* x, int d, const int* order, const int* seg, int k, float* centroids,
                            float* hassign);
void launch_pq_encode(hipStream_t s, const float* x, int64_t n, int d, int M, const int* assign,
                      const float* cc, const float* pqc, uint8_t* codes);

}  // namespace gh
