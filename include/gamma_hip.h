/*
 * gamma_hip.h -- C ABI of libgamma_hip.so, the MI355X (gfx950) device shim behind Gamma's
 * RetrievalModel plugin boundary.
 *
 * The only callers are the plugin classes in gamma_amd/host/ (GammaIVFPQHIPIndex, GammaIVFFlatHIPIndex,
 * GammaFLATHIPIndex -- REGISTER_MODEL(HIPIVFPQ / HIPIVFFLAT / HIPFLAT)), i.e. what a Gamma maintainer
 * compiles into libgamma next to index/impl/gamma_index_ivfpq.cc, and
 * the ctypes binding used by this repo's tests and bench.  Everything is extern "C", plain
 * pointers and sizes, caller-owned buffers, int return codes (0 = ok, <0 = error, see
 * gamma_hip_strerror); no C++/torch types, no exceptions cross this line.
 *
 * Each entry point names the reference interface it stands in for (paths relative to the
 * reference tree; "faiss:" = third_party/faiss-1.7.1.tar.gz, faiss-1.7.1/faiss/).
 *
 * Threading (the retrieval contract of SURVEY.md 8b: Search from any number of client threads while ONE indexing thread
 * adds / updates and API threads delete).  A handle owns one device, a search stream and a writer stream.
 *   - Searches may be called from any number of threads.  They take turns on the search stream (they share its
 *     workspaces); small host-buffer calls that find the handle busy are queued and run as ONE device batch.
 *   - Writers (Add, Update, Delete, raw rows, bitmap, columns) serialise among themselves and run on the writer stream
 *     beside the searches: a search reads the inverted lists through the VERSION of their (offset, length) tables that was
 *     current when it was enqueued, a writer publishes a new version after its copies (realtime_mem_data.cc:299-300).
 *   - The list arena and the raw store grow IN PLACE (mapped address ranges, gamma_hip_ivfpq_arena_growth /
 *     gamma_hip_raw_stats): growth waits for nobody.  Only operations that free or move memory a search may be reading
 *     (the arena repack after compactions, column growth, the reallocating fallbacks) wait for the searches in flight.
 * One handle per GPU; several GPUs behind one index object: gamma_hip_group_* below.
 */
#ifndef GAMMA_HIP_H_
#define GAMMA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAMMA_HIP_METRIC_IP 0 /* DistanceComputeType::INNER_PRODUCT, index/retrieval_model.h:20 */
#define GAMMA_HIP_METRIC_L2 1 /* DistanceComputeType::L2 */

/* error codes */
#define GAMMA_HIP_OK 0
#define GAMMA_HIP_EINVAL (-1)     /* bad argument / unsupported parameter */
#define GAMMA_HIP_ENOTTRAINED (-2)/* search before centroids/codebooks were set */
#define GAMMA_HIP_EDEVICE (-3)    /* a HIP runtime call failed (hipGetLastError text kept) */
#define GAMMA_HIP_ENOMEM (-4)     /* device or host allocation failed */
#define GAMMA_HIP_EFULL (-5)      /* list would exceed bucket_max_size (AddKeys returns false) */
#define GAMMA_HIP_EUNSUPPORTED (-6) /* the request asked for exact_ties = 1 on a shape the replay does not cover */

typedef struct gamma_hip_index gamma_hip_index;

/* RangeQueryResult as the scan sees it (table/range_query_result.h:53-67,96-109): a bitmap
 * relative to min_aligned plus [min,max] and the NOT flag.  Host memory; copied per call. */
typedef struct {
    const uint8_t* bitmap;
    int64_t bitmap_bytes;
    int32_t min_doc, max_doc, min_aligned;
    int32_t b_not_in;
} gamma_hip_range_filter;

/* Scalar range filter evaluated ON the device against a numeric column that lives in HBM
 * (gamma_hip_field_append).  Stands in for the per-request docid bitmap that
 * MultiFieldsRangeIndex::Search produces on the host (table/field_range_index.cc:1015-1200)
 * and for the per-doc check the reference's own GPU model makes through Table
 * (IsInRange<T>, index/impl/gpu/gamma_index_ivfpq_gpu.cc:685-727): same comparison, same
 * include_lower / include_upper rules; several filters are AND-ed; a doc beyond the end of
 * the column does not match.  INT / LONG columns compare lower_i / upper_i, FLOAT / DOUBLE
 * columns lower_f / upper_f (FLOAT in float). */
#define GAMMA_HIP_FIELD_INT 0
#define GAMMA_HIP_FIELD_LONG 1
#define GAMMA_HIP_FIELD_FLOAT 2
#define GAMMA_HIP_FIELD_DOUBLE 3
#define GAMMA_HIP_MAX_FIELD_FILTERS 8
typedef struct {
    int32_t field_id;
    int32_t include_lower, include_upper;
    int32_t reserved;
    int64_t lower_i, upper_i;
    double lower_f, upper_f;
} gamma_hip_field_filter;

/* Term filter on a STRING field evaluated on the device (GammaSearchCondition::term_filters).  The field value and the
 * filter value are lists of items separated by \001; is_union Or = any filter item among the doc's items, And = all of
 * them, as in FilteredByTermFilter (index/impl/gpu/gamma_index_ivfpq_gpu.cc:727-762).  Not (FilterOperator::Not,
 * table/field_range_index.h:23) = NONE of the filter items, which is what the engine's CPU bitmap path computes
 * (the reference's GPU-side FilteredByTermFilter treats Not like And; the device filter follows the bitmap path so that
 * "device_filters": 1 and 0 return the same documents).  Items are dictionary-encoded by the
 * caller (the plugin keeps the dictionary, gamma_amd/host/filter_bridge.h); an item the dictionary does not
 * know is passed as -1.  The doc's items live in HBM (gamma_hip_term_append). */
#define GAMMA_HIP_MAX_TERM_FILTERS 8
#define GAMMA_HIP_MAX_TERM_ITEMS 16
#define GAMMA_HIP_TERM_AND 0
#define GAMMA_HIP_TERM_OR 1
#define GAMMA_HIP_TERM_NOT 2
typedef struct {
    int32_t field_id;
    int32_t op;        /* TermFilter::is_union as the reference passes it: 0 And, 1 Or, 2 Not */
    int32_t n_items;
    int32_t items[GAMMA_HIP_MAX_TERM_ITEMS];
} gamma_hip_term_filter;

/* What GammaSearchCondition + IVFPQRetrievalParameters carry into Search()
 * (common/gamma_common_data.h:39-124, index/impl/gamma_index_ivfpq.h:629-673). */
typedef struct {
    int32_t metric;       /* per-request DistanceComputeType (gamma_index_ivfpq.cc:744-750) */
    int32_t nprobe;       /* resolved by the caller as gamma_index_ivfpq.cc:539-545 does */
    int32_t recall_num;   /* raised to k inside (gamma_index_ivfpq.cc:762-765) */
    int32_t has_rank;     /* GammaSearchCondition::has_rank: exact re-rank of recall_num */
    float min_score;      /* IsSimilarScoreValid window (gamma_common_data.h:95-97) */
    float max_score;
    int32_t coarse_mode;  /* -1: faiss rule nq<20 -> exact per-pair, else GEMM form
                             (faiss:utils/distances.cpp:303,346); 0 exact; 1 GEMM (MFMA) */
    int32_t has_range;    /* range_query_result != nullptr */
    int32_t n_range;      /* number of RangeQueryResult; 0 with has_range => nothing valid */
    const gamma_hip_range_filter* range;
    int32_t n_field;      /* GammaSearchCondition::range_filters evaluated on device columns */
    int32_t n_term;       /* GammaSearchCondition::term_filters evaluated on device columns */
    const gamma_hip_field_filter* field;
    const gamma_hip_term_filter* term;
    int32_t exact_ties;   /* the reference's heap order inside exact distance ties (gamma_hip_set_exact_ties) for this
                             request: 0 = the handle's setting (default on), 1 = on, -1 = off */
} gamma_hip_search_params;

/* ---- lifecycle ------------------------------------------------------------------- */
/* replaces: new GammaIVFPQIndex / GammaFLATIndex + Init (gamma_index_ivfpq.cc:119-214,
 * gamma_index_flat.cc:62-76).  One handle = one device. */
int gamma_hip_create(int device, gamma_hip_index** out);
int gamma_hip_destroy(gamma_hip_index* h);
const char* gamma_hip_strerror(int code);
const char* gamma_hip_last_error(gamma_hip_index* h);
/* hipStream_t the handle launches on (for event timing / overlap by the caller) */
void* gamma_hip_stream(gamma_hip_index* h);
int gamma_hip_synchronize(gamma_hip_index* h);

/* The IVFPQ scan of large batches bounds each query's recall_num-th best distance from its nearest probe group and keeps
 * only the candidates within the bound of the other groups (csrc/scan.hip); queries whose bound turns out too loose (a
 * survivor slice overflows) are scored again and selected from the full candidate row.  Results do not depend on it.  On
 * data where the nearest lists do not hold the best candidates (full-size C5: noise-dominated inner-product vectors) nearly
 * every query falls through and the pre-filter costs more than it saves (41 ms per 4096 queries against 24 without it):
 * the handle counts the queries that fall through and, while they are more than half of the recent ones, scans unbounded,
 * on = 0: no feedback, the pre-filter whenever the shape allows it.
 * re-probing every 256 calls; what it learnt holds for one kind of call (nprobe, recall_num, metric, filter or not).
 * stats: out4 = {queries that fell through, queries that went through the bounded scan -- both of the current kind of call --,
 * times the handle backed off, consumer workgroups that ever gave up waiting for their bound}. */
int gamma_hip_set_scan_bound_feedback(gamma_hip_index* h, int on);
int gamma_hip_scan_bound_stats(gamma_hip_index* h, int64_t* out4);
/* Upper bound in bytes of the per-chunk workspaces (coarse distance matrix, ADC distance buffer);
 * larger calls are processed in chunks of queries.  Default: an eighth of the device memory, 1 to 32 GiB. */
int gamma_hip_set_workspace_budget(gamma_hip_index* h, int64_t bytes);
/* Exact distance ties.  The reference keeps candidates in faiss binary heaps (faiss:utils/Heap.h:46-131): WHICH of
 * several candidates at exactly the same fp32 distance survive a cut, and the order equal distances come out in,
 * is what the heap's sift order leaves -- at the nprobe cut of the coarse quantizer (HeapResultHandler,
 * faiss:impl/ResultHandler.h:112-117), at the recall_num cut of the list scan (KnnSearchResults::add,
 * index/impl/gamma_index_ivfpq.h:363-369) and in compute_dis, which feeds the k-heap in the ARRAY order of the
 * unsorted recall heap (index/impl/gamma_index_ivfpq.cc:646-680).  on != 0 (the DEFAULT): rows / queries in which
 * such a tie can change the result are detected by the regular kernels and redone by replaying the reference's heaps
 * (csrc/ties.hip, csrc/heap_dev.h), so labels and ranks are the reference's, ties included.  on == 0: a top-k is "the
 * k smallest (distance, scan position) pairs" -- the same distances at every rank, the same ids up to the order /
 * membership inside groups of exactly equal distances, and no replay cost (a few queries in a thousand on integer
 * data, none to speak of on real-valued data).  Per request: gamma_hip_search_params.exact_ties.
 * Covers IVFPQ / IVFFLAT / flat search, every batch size, every recall_num and k the ABI accepts (<= 4096), the
 * list-sharded merge and the group.  From 100 probes on the coarse assignment is replayed through faiss's ReservoirTopN
 * (what knn_L2sqr collects through there, faiss:utils/distances.cpp:341-358; csrc/reservoir_dev.h), below through its
 * result heap.  NOT covered: nprobe > 1024, a flat search for k = 4096 or over 2^31 rows.  Such a call never
 * degrades silently: with exact_ties = 1 in the request it fails with GAMMA_HIP_EUNSUPPORTED; when it merely inherits the
 * handle's default it runs with the (distance, position) order inside ties and is counted
 * (gamma_hip_ties_not_honoured). */
int gamma_hip_set_exact_ties(gamma_hip_index* h, int on);
/* Coarse quantizer of large batches (>= 4096 queries, >= 2048 lists, d in {32, 64, 96, 128}, nprobe <= 64) without
 * the [nq][nlist] distance matrix (csrc/coarse.hip).  on: see below.
 * list_cap: capacity of a query's per-strip survivor list, 1..128 (default 128); a query that overflows it is redone
 * by the repair kernel -- tests shrink it to force that path.  Results are identical either way. */
int gamma_hip_set_coarse_fused(gamma_hip_index* h, int on, int list_cap);
/* on: 0 = distance matrix + selection; 1 (default) = matrix-free path with the bf16 filter where the shape and the
 * centroids allow it, the fp32 filter elsewhere; 2 = matrix-free path with the fp32 filter.  Same results in all.
 * out4: {queries the bf16 chain handed to the repair kernels, queries it ran on, times the handle switched itself to
 * the fp32 filter, fp32 calls left before it probes the bf16 filter again} */
int gamma_hip_coarse_filter_stats(gamma_hip_index* h, int64_t* out4);
/* The exact re-rank (has_rank) over a dense fp32 raw store whose rows are a multiple of 16 floats (up to 1536) can run behind
 * a filter: a one-byte image of the rows (d + 8 bytes per row, built by the first call that qualifies, kept in step by
 * raw_append / _write / _update / _update_batch, released by raw_clear, counted in gamma_hip_total_mem_bytes once it exists)
 * proves most of a query's recall_num candidates out of its first k + 1, and only the others are measured against their
 * fp32 rows (csrc/rerank_filter.hip).  Results are the same bit for bit.  mode: 0 = off; 1 (default) = calls of 1024 queries
 * and more; 2 = every call that reaches the fused re-rank kernel.  While more than half of the recent candidates survive, the
 * handle runs the plain kernel for 256 calls and probes again.
 * out5: {candidates the filter saw, candidates that survived it, calls it ran in, times the handle backed off, image rows} */
int gamma_hip_set_rerank_filter(gamma_hip_index* h, int mode);
int gamma_hip_rerank_filter_stats(gamma_hip_index* h, int64_t* out5);
/* The filtered re-rank has two kernels with the same results: one workgroup per query (every shape the filter admits), and one
 * wave per query (rows of 128 floats, at most 256 candidates per query, min(k + 1, candidates) <= 64).
 * form: 0 (default) = automatic, the wave form where it is admitted and the call has enough queries to fill the device with
 * waves (out4[3] says how many); 1 = the workgroup kernel always; 2 = the wave form wherever it is admitted.
 * out4: {the setting, the kernel of the last filtered call (1 workgroup, 2 wave; 0: none yet), filtered calls in the wave form,
 * the query count from which automatic takes the wave form} */
int gamma_hip_set_rerank_filter_form(gamma_hip_index* h, int form);
int gamma_hip_rerank_filter_form(gamma_hip_index* h, int64_t* out4);
/* Flat search (GammaFLATIndex::Search, index/impl/gamma_index_flat.cc:118-300) scores every row; here the passes behind the
 * first row chunk run a bf16 filter on the matrix pipe and only its survivors get the reference's arithmetic
 * (csrc/flat_mfma.hip), so results are the reference's bit for bit.  No handle, no device call:
 * returns 1 if rows of d floats have a filter kernel (1 <= d <= 4096) and writes the row length the filter pads to
 * (ceil32(d); elements >= d are exact zeros) and the constant c of its margin c (|x|^2 + |y|^2); returns 0 otherwise
 * (such rows are scored exactly throughout, as the reference scores them).  The gates of a call -- at least 64 queries,
 * 4096 rows, k <= 256 -- are not part of the answer. */
int gamma_hip_flat_filter_shape(int d, int* d_pad, float* margin);
/* out3 = {filter passes launched, (query, row) pairs those passes scored, passes redone without the running bound after
 * a survivor list overflowed} since creation or the last reset.  Host-side counters: no synchronisation, no device read.
 * The reference has no counterpart (it scores every pair: gamma_index_flat.cc:118-300). */
int gamma_hip_flat_filter_stats(gamma_hip_index* h, int64_t* out3, int reset);
/* Calls of up to 512 queries (nprobe <= 128, recall_num <= 1024) run as a chain of
 * four or five fused kernels instead of eleven (DESIGN.md "small batches").  on: 1 = automatic (default), 0 = always
 * the regular chain, n >= 2 = automatic with the two-level selection of long candidate rows forced on with n slices
 * (tests; by default it is used when nprobe x 1.5 mean list lengths exceed 16384).  Results are identical either way. */
int gamma_hip_set_small_path(gamma_hip_index* h, int on);
/* Flat search over a narrow raw store.  on: 0 (default) = gamma_hip_flat_search, _flat_search_device and
 * _flat_search_device_wait refuse a float16 / uint8 / int8 store (gamma_hip_raw_init_f16 / _i8) with
 * GAMMA_HIP_EUNSUPPORTED, as every other reader of fp32 rows does; 1 = the three serve it: every row is widened to fp32
 * -- exactly -- as it is loaded and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the widened
 * row, so distances and labels are byte-identical to those of an fp32 store that holds the widened rows (DESIGN.md
 * section 15).  Nothing else changes: IVFFLAT search (a switch of its own, below) keeps refusing a narrow store, flat search
 * keeps refusing a sparse store, the shard / merge / export entries and gamma_hip_raw_put / _raw_drop refuse a narrow store
 * unless gamma_hip_set_sparse_narrow_rows (below) says otherwise, and an fp32 store is served as before whatever the switch
 * says. */
int gamma_hip_set_flat_narrow_rows(gamma_hip_index* h, int on);
/* IVFFLAT search over a narrow raw store; a switch of its own, independent of the one above.  on: 0 (default) =
 * gamma_hip_ivfflat_search and _ivfflat_search_device refuse a float16 / uint8 / int8 store with GAMMA_HIP_EUNSUPPORTED,
 * as before; 1 = both serve it.  The reference's lists hold the vectors as fp32 and GammaIVFFlatScanner1::scan_codes
 * (index/impl/gamma_index_ivfflat.h:52-75) calls faiss::fvec_L2sqr / fvec_inner_product on each; here a list holds vids and
 * the rows come from the raw store: a narrow row is widened to fp32 -- exactly -- as it is loaded and is the scanner's yj from
 * then on, so distances and labels are byte-identical to those of an fp32 store that holds the widened rows, exact ties
 * included.  The IVFFLAT shard entries that read rows -- gamma_hip_ivfflat_search_shard and
 * _ivfflat_shard_export, and through them gamma_hip_group_ivfflat_search -- follow the same switch: 0 = they refuse a float16 /
 * uint8 / int8 store, 1 = they serve it, dense or sparse (a sparse narrow store exists only after
 * gamma_hip_set_sparse_narrow_rows, below), byte-identical to shards holding the widened rows as fp32.
 * Nothing else changes: the combining queue keeps refusing a narrow store, IVFFLAT search keeps refusing a sparse store, the
 * IVFPQ shard / merge / export entries and gamma_hip_raw_put / _raw_drop refuse a narrow store unless
 * gamma_hip_set_sparse_narrow_rows says otherwise, an sq8 store is refused at every shard entry, and an fp32 store is served
 * as before whatever the switch says. */
int gamma_hip_set_ivfflat_narrow_rows(gamma_hip_index* h, int on);
/* Raw rows sharded with their lists (gamma_hip_raw_put) in a narrow store; a switch of its own, independent of every other.
 * on: 0 (default) = gamma_hip_raw_put / _raw_drop and gamma_hip_ivfpq_shard_exact / _shard_export_exact refuse a float16 /
 * uint8 / int8 / sq8 store (gamma_hip_raw_init_f16 / _i8 / _sq8) with GAMMA_HIP_EUNSUPPORTED, as before; 1 = they serve it.
 * gamma_hip_raw_put / _raw_drop then keep the sparse fp32 store's semantics -- a held vid is rewritten in place, freed rows are
 * reused before the store grows, the last entry of a vid named twice wins -- and the narrow stores' rules for what a row may
 * hold: the whole batch is checked first (float16: no finite value that rounds to infinity; uint8 / int8: every value
 * converts exactly; sq8: ranges set, every value finite), and a refused row fails the call with nothing of the handle
 * changed.  An sq8 store sets its ranges before its first gamma_hip_raw_put, the empty one included: a sparse store's are fixed.  Rows are converted on the device.  gamma_hip_ivfpq_shard_exact serves a narrow store dense or sparse,
 * _shard_export_exact a sparse one: a row is widened (sq8: decoded through the store's table) exactly as it is loaded and every
 * distance is fvec_L2sqr / fvec_inner_product of the fp32 query and that row, so every result is byte-identical to that of
 * an fp32 store holding the widened rows.  The IVFFLAT shard entries read a sparse float16 / uint8 /
 * int8 store made this way after gamma_hip_set_ivfflat_narrow_rows, and only then; this switch alone
 * leaves them refusing.  Nothing else changes: an fp32 store is served as before
 * whatever the switch says; flat and IVFFLAT search, gamma_hip_raw_gets / _raw_append / _raw_write keep refusing a sparse store,
 * the merges with has_rank and no travelled distances a narrow one, and 4-bit and OPQ handles every shard entry. */
int gamma_hip_set_sparse_narrow_rows(gamma_hip_index* h, int on);
/* The list scan of the IVFFLAT search (GammaIVFFlatScanner1::scan_codes, index/impl/gamma_index_ivfflat.h:52-75: one
 * fvec_L2sqr / fvec_inner_product per entry of a probed list) has a list-major form -- a list's rows are read once per tile
 * of the queries probing it instead of once per query (csrc/ivfflat.hip, DESIGN.md sections 9 and 22) -- for some row
 * lengths.  No handle, no device call: *kind = 0 none (d % 16 != 0 or d > 4096: one workgroup per (query, probe) pair
 * always), 1 = fixed-length (d in {16, 32, 64, 96, 128}: the whole row in registers), 2 = row-sliced (every other multiple of
 * 16 up to 4096); *slab = the elements of a row held in registers at a time (kind 1: d), *qtile = the queries per tile; both 0
 * with kind 0.  The gates of a call -- at least 2 nlist (query, probe) pairs, no list mask -- are not part of the answer.
 * Results are the same bits in every form.  Returns GAMMA_HIP_OK, GAMMA_HIP_EINVAL for a null pointer. */
int gamma_hip_ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile);
/* out4 = {IVFFLAT calls served by the small path, query chunks of the chunked path scanned by the pair kernel, by the
 * fixed-length list-major kernel, by the row-sliced one} since creation or the last reset.  Host-side counters: no
 * synchronisation, no device read.  The reference has no counterpart (its scanner walks one list for one query:
 * gamma_index_ivfflat.h:52-75). */
int gamma_hip_ivfflat_scan_stats(gamma_hip_index* h, int64_t* out4, int reset);
/* Flat search over a scalar-quantised raw store (gamma_hip_raw_init_sq8); a switch of its own, independent of the two above.
 * on: 0 (default) = gamma_hip_flat_search, _flat_search_device and _flat_search_device_wait refuse an sq8 store with
 * GAMMA_HIP_EUNSUPPORTED, as before and whatever gamma_hip_set_flat_narrow_rows says; 1 = the three serve it: every code is
 * decoded as it is loaded, w = vmin[j] + float(code) * step[j] -- a multiply, then an add, each rounded in fp32, never an fma
 * and never folded into the query -- and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the decoded
 * row, so distances and labels are byte-identical to those of an fp32 store that holds the decoded rows, exact ties included
 * (DESIGN.md section 20).  The reference has no scalar-quantised flat model; the yardstick is its flat search
 * (gamma_index_flat.cc:118-300) over the rows the store holds.  Nothing else changes: IVFFLAT search (a switch of its own,
 * below), the shard / merge / export entries, gamma_hip_raw_put / _raw_drop, the combining queue and a sparse store keep
 * refusing an sq8 store, and an fp32, float16 or byte store is served or refused as before whatever this switch says. */
int gamma_hip_set_flat_sq8_rows(gamma_hip_index* h, int on);
/* IVFFLAT search over a scalar-quantised raw store (gamma_hip_raw_init_sq8); a switch of its own, independent of
 * gamma_hip_set_ivfflat_narrow_rows and gamma_hip_set_flat_sq8_rows.  on: 0 (default) = gamma_hip_ivfflat_search and
 * _ivfflat_search_device refuse an sq8 store with GAMMA_HIP_EUNSUPPORTED, as before and whatever the two other switches say;
 * 1 = both serve it, on every path (small path, list-major scan in both forms, pair scan, list masks, exact ties on and off,
 * score window, delete bitmap, filters, vid -> doc map, entries with bit 63): every code is decoded as it is loaded,
 * w = vmin[j] + float(code) * step[j] -- a multiply, then an add, each rounded in fp32, never an fma and never folded into
 * the query -- and is the scanner's yj (GammaIVFFlatScanner1::scan_codes, index/impl/gamma_index_ivfflat.h:52-75) from then
 * on, so distances and labels are byte-identical to those of an fp32 store that holds the decoded rows over the same lists,
 * exact ties included.  Only the store is quantised: coarse assignment sees the caller's fp32 rows.
 * Nothing else changes: the shard / merge / export entries, gamma_hip_raw_put / _raw_drop, the combining queue and a sparse
 * store keep refusing an sq8 store, and an fp32, float16 or byte store is served or refused as before whatever this switch
 * says. */
int gamma_hip_set_ivfflat_sq8_rows(gamma_hip_index* h, int on);
/* out3 = {coarse rows redone, queries whose recall_num cut went through a tie, queries replayed} since creation
 * or the last reset; meaningful with exact ties on */
int gamma_hip_tie_stats(gamma_hip_index* h, int64_t* out3, int reset);
/* search calls since creation (or the last reset) that ran WITHOUT the exact-ties mode although the handle's default asked
 * for it, because their shape is beyond the replay's range (see gamma_hip_set_exact_ties); the reference has no such
 * limit (faiss:utils/Heap.h:103-131, index/impl/gamma_index_ivfpq.cc:762-770) */
int gamma_hip_ties_not_honoured(gamma_hip_index* h, int64_t* out_calls, int reset);
/* Calls (searches, Add / assign, k-means iterations' assignments) whose GEMM-form coarse distances fell into a shape for
 * which the compiled library's sgemm_ kernel is NOT restated (faiss:utils/distances.cpp:215-296 through MKL: K > 768 or an
 * odd split, K = 384 with a database remainder block of 9..512 rows, remainder blocks of 1..7 rows -- nq mod 4096 or
 * nlist mod 1024).  There the coarse distances of a few entries can differ from the library's by an ulp (measured:
 * tests/test_oracle_vs_ref.py::test_unrestated_blas_corners_differ_by_ulps); every other shape is the library's bit for
 * bit.  Counted, never silent; the plugins log a new count. */
int gamma_hip_blas_form_not_restated(gamma_hip_index* h, int64_t* out_calls, int reset);

/* ---- numeric scalar columns for on-device range filters (docid = row).  The engine side
 *      appends a doc's value when the doc is added (Table::Add, table/table.cc) ----------- */
int gamma_hip_field_append(gamma_hip_index* h, int field_id, int dtype, int64_t n, const void* values);
int gamma_hip_field_update(gamma_hip_index* h, int field_id, int64_t docid, const void* value);
int64_t gamma_hip_field_count(gamma_hip_index* h, int field_id);
/* STRING columns for on-device term filters: n more docs (docid = row), doc i with counts[i] dictionary-encoded
 * items, all items concatenated in `items` (Table::Add -> the plugin's dictionary, filter_bridge.h) */
int gamma_hip_term_append(gamma_hip_index* h, int field_id, int64_t n_docs, const int32_t* counts,
                          const int32_t* items);
int64_t gamma_hip_term_count(gamma_hip_index* h, int field_id);
/* a doc's items rewritten after its STRING field was updated in the table (Table::Update, table/table.cc:420-470):
 * in place when they fit, else at the end of the item array; the doc's row switches over with one 8-byte store */
int gamma_hip_term_update(gamma_hip_index* h, int field_id, int64_t docid, int32_t count, const int32_t* items);

/* ---- raw vector store (VectorReader::Gets / MemoryRawVector, vector/raw_vector.cc:99-109,
 *      vector/memory_raw_vector.cc:90-142): device mirror, vid = row ------------------- */
int gamma_hip_raw_init(gamma_hip_index* h, int d);
int gamma_hip_raw_append(gamma_hip_index* h, int64_t n, const float* vecs);
int gamma_hip_raw_update(gamma_hip_index* h, int64_t vid, const float* vec);
/* n rows rewritten with one wait for the device (vids the mirror has not reached yet are skipped) */
int gamma_hip_raw_update_batch(gamma_hip_index* h, int64_t n, const int64_t* vids, const float* vecs);
/* rows [first_vid, first_vid + n) written at their own position: idempotent (a repeated or overlapping
 * call rewrites the same rows with the same bytes), the row count only ever grows to first_vid + n.
 * first_vid may not leave a gap (first_vid <= gamma_hip_raw_count).  This is what a mirror of the engine's
 * vector store needs when Search (brute force before training) and the indexing thread's Add race. */
int gamma_hip_raw_write(gamma_hip_index* h, int64_t first_vid, int64_t n, const float* vecs);
/* VectorReader::Gets (vector/raw_vector.cc:99-109, vector/memory_raw_vector.cc:136-142): rows vids[0..n) of the device
 * store copied to out [n][d] (the rows compute_dis reads); GAMMA_HIP_EINVAL for a vid outside [0, gamma_hip_raw_count) */
int gamma_hip_raw_gets(gamma_hip_index* h, int64_t n, const int64_t* vids, float* out);
/* Raw vectors SHARDED WITH THEIR LISTS (round 6; SURVEY 8(e): "shard by the same owner"): a list shard of a multi-GPU job keeps
 * the rows of the vectors in ITS lists only -- rows vecs[i] of vector ids vids[i], in any order, appended to the store with a
 * vid -> row table (4 bytes per vector id) beside it; C4 on 8 GPUs: 6.4 GB of rows per GPU instead of 51.2.  The first call
 * turns the (empty) store into that form for good.  Such a handle serves gamma_hip_ivfpq_shard_exact / _shard_export_exact; what
 * needs every row -- has_rank inside a search on this handle, flat / IVFFLAT search, raw_gets / raw_write / raw_update --
 * answers GAMMA_HIP_EUNSUPPORTED.  Replaces MemoryRawVector::GetVector for the rows a shard owns
 * (vector/memory_raw_vector.cc:136-142). */
int gamma_hip_raw_put(gamma_hip_index* h, int64_t n, const int64_t* vids, const float* vecs);
/* A sparse store's rows can be rewritten, dropped and reused (a realtime Update that moves a vector to a list of another
 * shard takes its row along).  gamma_hip_raw_put on a vector id the store already holds rewrites that row IN PLACE (named twice
 * in one call: the last one wins); gamma_hip_raw_drop makes the store forget rows -- vector ids it does not hold are ignored --
 * and later puts reuse the freed rows before the store grows.  A store that holds rows by vector id (raw_append / raw_write)
 * answers GAMMA_HIP_EINVAL to a drop.  A search enqueued before such a call never reads a half-written row: a rewrite in place
 * and the reuse of a freed row wait for the searches in flight, a new row at the end of the store is listed only afterwards
 * (DESIGN.md 9). */
int gamma_hip_raw_drop(gamma_hip_index* h, int64_t n, const int64_t* vids);
/* empties the store -- rows, vid -> row table, free list -- back to the state after gamma_hip_raw_init (neither dense nor
 * sparse yet: a store mirrored by vector id before training can become a sparse one).  Waits for the searches in flight. */
int gamma_hip_raw_clear(gamma_hip_index* h);
/* out3 = {rows that hold a vector, rows handed out so far, freed rows waiting for reuse} of a sparse store (zeros otherwise) */
int gamma_hip_raw_sparse_stats(gamma_hip_index* h, int64_t* out3);
/* rows of a store by vector id; of a sparse store the rows that hold a vector */
int64_t gamma_hip_raw_count(gamma_hip_index* h);
/* out4 = {rows (a sparse store: rows handed out so far), rows the mapped / allocated memory holds, reallocations that MOVED the store so far, 1 when the store
 * grows in place (virtual memory management: physical chunks mapped behind the rows, nothing ever moves or waits for
 * the searches in flight -- what the reference gets from its 500 000-vector segments, vector/memory_raw_vector.cc:90-142)} */
int gamma_hip_raw_stats(gamma_hip_index* h, int64_t* out4);
/* A store of IEEE binary16 rows instead of gamma_hip_raw_init's fp32 rows: half the bytes held, half the bytes the exact
 * re-rank gathers (the reference's lossy store of its own is "compress" / ZFP, vector/raw_vector.h:179-213, decompressed for
 * compute_dis; this replaces MemoryRawVector's fp32 rows, vector/memory_raw_vector.cc:90-142, the same way).  The element type
 * is fixed here.  The writers (raw_append / raw_write / raw_update / raw_update_batch) take fp32 and round on the writer
 * stream: round to nearest even, subnormal halves kept -- what numpy's float32 -> float16 gives; a FINITE value whose half is
 * infinite (|x| >= 65520) fails the call with GAMMA_HIP_EINVAL before anything of the store changes; NaN and +-inf are stored
 * as they convert.  Only the store is rounded: training, assignment, residuals and codes see the caller's fp32.  The exact
 * distance of a has_rank IVFPQ search is fvec_L2sqr / fvec_inner_product of the fp32 query and float(half row) (the widening
 * is exact) in the reference's operation order, so given the rounded rows every result is the reference's, ties included.
 * gamma_hip_raw_gets widens.  Served: gamma_hip_ivfpq_search and its device-pointer forms (8-bit, 4-bit, OPQ handles).
 * GAMMA_HIP_EUNSUPPORTED: gamma_hip_raw_put / _raw_drop, flat and IVFFLAT search, gamma_hip_ivfpq_shard_exact /
 * _shard_export_exact, _merge_rerank / _merge_replay with has_rank and no travelled distances. */
int gamma_hip_raw_init_f16(gamma_hip_index* h, int d);
/* bytes of one element of the raw store: 4 (gamma_hip_raw_init), 2 (gamma_hip_raw_init_f16), 1 (gamma_hip_raw_init_i8, gamma_hip_raw_init_sq8), 0 before
 * any of them */
int gamma_hip_raw_elem_bytes(gamma_hip_index* h);
/* A store of one byte per element: uint8 rows, range [0, 255] (is_signed = 0), or int8 rows, range [-128, 127] (is_signed = 1) --
 * a quarter of the fp32 store's bytes, and LOSSLESS OR REFUSED: the writers (raw_append / raw_write / raw_update /
 * raw_update_batch) take fp32 and store a value only if it is finite, integral and inside the element type's range, which is
 * exactly when float(T(x)) == x (-0.0 is accepted and stored as 0).  Any other value -- NaN, +-inf, a fraction, a value out of
 * range -- fails the call with GAMMA_HIP_EINVAL before anything changes: no byte of the store, no counter, no list; last_error
 * names the offending position.  The element type is fixed at the first init; a second init with another type or d answers
 * GAMMA_HIP_EINVAL.  Only the store is narrow: training, assignment, residuals and codes see the caller's fp32.  A byte widens
 * to fp32 exactly, so the exact distance of a has_rank IVFPQ search -- fvec_L2sqr / fvec_inner_product of the fp32 query and the
 * widened row in the reference's operation order -- and with it every result, ties included, is what the fp32 store gives.
 * gamma_hip_raw_gets widens.  Served and refused as for gamma_hip_raw_init_f16: served are gamma_hip_ivfpq_search and its
 * device-pointer forms (8-bit, 4-bit, OPQ handles); GAMMA_HIP_EUNSUPPORTED: gamma_hip_raw_put / _raw_drop, flat and IVFFLAT
 * search, gamma_hip_ivfpq_shard_exact / _shard_export_exact, _merge_rerank / _merge_replay with has_rank and no travelled
 * distances. */
int gamma_hip_raw_init_i8(gamma_hip_index* h, int d, int is_signed);
/* element type of the raw store: 0 fp32 (also before any init), 1 float16, 2 uint8, 3 int8, 4 sq8 (gamma_hip_raw_init_sq8) */
int gamma_hip_raw_elem_type(gamma_hip_index* h);
/* The byte store's acceptance predicate, as the writers apply it: GAMMA_HIP_OK when every one of the n values is storable in
 * uint8 (is_signed = 0) or int8 (is_signed = 1); otherwise GAMMA_HIP_EINVAL, and *first_bad (when not null) is the index of the
 * first value that is refused.  Pure host code: no handle, no device call. */
int gamma_hip_raw_i8_check(const float* x, int64_t n, int is_signed, int64_t* first_bad);
/* A SCALAR-QUANTISED store of one byte per element for float data (element type 4, "sq8"): a quarter of the fp32 store's bytes,
 * and LOSSY.  Per dimension j the store keeps vmin[j] <= vmax[j] (fp32, finite) and, derived on the host in fp32 with one IEEE
 * operation each (gamma_hip_raw_sq8_params): span = vmax - vmin, step = span / 255, inv = 255 / span; a dimension whose span
 * is 0 or whose inv is not finite is constant, step = inv = 0.
 *   encode (the writers, on the device): c = inv[j] == 0 ? 0 : (uint8) min(max(rintf((x - vmin[j]) * inv[j]), 0), 255) -- a
 *            subtract, a multiply, a round-half-to-even and a clamp, each rounded in fp32, no fma; values outside the range clip;
 *   decode (the readers):                w = vmin[j] + (float)c * step[j] -- a multiply, then an add, each rounded in fp32.
 * The exact distance of a has_rank IVFPQ search is fvec_L2sqr / fvec_inner_product of the fp32 query and the DECODED row in the
 * reference's operation order, so every result, ties included, is what an fp32 store of the decoded rows gives.  Only the store
 * is quantised: training, assignment, residuals and codes see the caller's fp32.  The writers (raw_append / raw_write /
 * raw_update / raw_update_batch) take fp32; a non-finite value fails the call with GAMMA_HIP_EINVAL before anything changes, and
 * so does a writer called with n > 0 before the ranges exist.  gamma_hip_raw_gets returns decoded rows.  The element type is
 * fixed at the first init.  Served: gamma_hip_ivfpq_search and its device-pointer forms (8-bit, 4-bit, OPQ handles).
 * GAMMA_HIP_EUNSUPPORTED: gamma_hip_raw_put / _raw_drop, flat and IVFFLAT search (whatever gamma_hip_set_flat_narrow_rows /
 * _set_ivfflat_narrow_rows say; each serves an sq8 store after its own switch, gamma_hip_set_flat_sq8_rows /
 * _set_ivfflat_sq8_rows), gamma_hip_ivfpq_shard_exact / _shard_export_exact, _merge_rerank / _merge_replay with has_rank
 * and no travelled distances. */
int gamma_hip_raw_init_sq8(gamma_hip_index* h, int d);
/* The ranges of an sq8 store: d floats each.  set is allowed only while the store holds no row (after the init, or after
 * gamma_hip_raw_clear, which keeps the ranges); otherwise, and for a non-finite bound, vmin > vmax or a span that is not
 * finite, GAMMA_HIP_EINVAL.  get answers GAMMA_HIP_EINVAL before any ranges exist. */
int gamma_hip_raw_sq8_set_ranges(gamma_hip_index* h, const float* vmin, const float* vmax);
int gamma_hip_raw_sq8_get_ranges(gamma_hip_index* h, float* vmin, float* vmax);
/* sets the ranges to the per-dimension minimum and maximum of n host rows (n > 0, every value finite), reduced on the device;
 * minimum and maximum do not depend on the order of the reduction, so the result is exact (a zero comes back as +0.0) */
int gamma_hip_raw_sq8_train(gamma_hip_index* h, int64_t n, const float* x);
/* The sq8 store's acceptance predicate, as the writers apply it: GAMMA_HIP_OK when every one of the n values is finite;
 * otherwise GAMMA_HIP_EINVAL, and *first_bad (when not null) is the index of the first value that is refused.  Pure host code:
 * no handle, no device call. */
int gamma_hip_raw_sq8_check(const float* x, int64_t n, int64_t* first_bad);
/* step_out[j], inv_out[j] of the ranges, by the derivation above (either output may be null).  GAMMA_HIP_EINVAL for a
 * non-finite bound, vmin > vmax or a span that is not finite.  Pure host code. */
int gamma_hip_raw_sq8_params(int d, const float* vmin, const float* vmax, float* step_out, float* inv_out);

/* ---- delete bitmap (bitmap::BitmapManager, util/bitmap_manager.cc:171-192): bit = docid,
 *      byte docid>>3, mask 1<<(docid&7) --------------------------------------------------- */
int gamma_hip_bitmap_upload(gamma_hip_index* h, const uint8_t* bitmap, int64_t nbits);
int gamma_hip_bitmap_set(gamma_hip_index* h, const int64_t* docids, int64_t n, int value);

/* ---- IVFPQ model state (faiss::IndexIVFPQ members the scanner reads) --------------- */
/* replaces GammaIVFPQIndex::Init's parameter checks (gamma_index_ivfpq.cc:119-214);
 * nbits must be 8, d % M == 0 (HNSW quantizer / padding are rejected: EINVAL; an OPQ rotation is set afterwards,
 * gamma_hip_opq_set) */
int gamma_hip_ivfpq_init(gamma_hip_index* h, int d, int nlist, int M, int nbits, int metric,
                         int bucket_init_size, int bucket_max_size);
/* 4-bit PQ codes.  Replaces GammaIVFPQIndex::Init with nbits_per_idx = 4 (gamma_index_ivfpq.cc:167-170: the value goes
 * straight into faiss::ProductQuantizer; the scanner is templated over the PQ decoder, gamma_index_ivfpq.h:540-601):
 * ksub = 16, code_size = (4 M + 7) / 8, sub-quantizer m in bits [4m, 4m + 4) of the code -- an even m in the low nibble of
 * byte m / 2 -- as PQEncoderGeneric packs them (faiss:impl/ProductQuantizer-inl.h:10-44); with an odd M the last high
 * nibble is 0.  Requires d % M == 0, d / M <= 64 and code_size <= 64 (EINVAL otherwise).  After this init the entry points
 * of an 8-bit handle serve the handle, sized by its ksub: _set_trained (pq_centroids M x 16 x dsub, table nlist x M x 16),
 * _get_precomputed_table, _train (16 centroids per sub-quantizer from the residuals of at most 256 * 16 points,
 * faiss:IndexIVFPQ.cpp:67-131), _add, _encode, _encode_each, _update_batch, _apply_updates, _add_keys(_batch), _get_list,
 * _code_size, _delete, _compact_if_need, the raw store, _search, _search_device(_wait) and _last_stages.  Results are the
 * reference's bit for bit, ties included, as for 8 bits.  GAMMA_HIP_EUNSUPPORTED with a message, never a silent
 * fall-back: the shard, merge and export entry points, gamma_hip_ivfpq_set_list_mask, and this init itself when the
 * precomputed table nlist * M * 16 * 4 bytes would exceed precomputed_table_max_bytes (table mode 0).  The group
 * (gamma_hip_group_*) stays 8-bit.  gamma_hip_ivfpq_init keeps refusing nbits != 8. */
int gamma_hip_ivfpq4_init(gamma_hip_index* h, int d, int nlist, int M, int metric, int bucket_init_size,
                          int bucket_max_size);
/* ---- OPQ rotation ("opq": {"nsubvector": N} of the reference's IVFPQ model) ---------------------------------------
 * Replaces faiss::OPQMatrix* opq_ as GammaIVFPQIndex uses it (index/impl/gamma_index_ivfpq.h:745, gamma_index_ivfpq.cc:
 * 155-166): every vector is rotated before the coarse quantizer and the PQ encoder (Add :424-512, Update :375-422), every
 * query before the coarse quantizer and the scan (:514-566); the exact re-rank (compute_dis :646-680) keeps reading the
 * raw store with the raw query.
 * Arithmetic (ours, fixed by contract; DESIGN.md "OPQ"): xt[i] = sum_j A[i*d + j] * x[j] as ONE fp32 accumulator starting
 * at +0, j ascending, one fmaf per term -- independent of the batch size, of the row's position in the batch and of the
 * kernel that serves the shape.  The reference's LinearTransform::apply_noalloc (faiss:VectorTransform.cpp:41-80) is one
 * sgemm_ call whose summation order its BLAS picks from the shape: the same vector rotates to different bits there in
 * Update (n = 1) and in Add, so there is no reference bit pattern to restate; within d fmaf roundings of the exact product
 * both are.  Everything downstream of the rotated vectors stays the reference's bit for bit.
 * _set: A is d x d row-major.  Valid on an 8-bit IVFPQ handle after gamma_hip_ivfpq_init while its lists are empty
 *   (GAMMA_HIP_EINVAL once they hold entries: their codes are of unrotated vectors).  GAMMA_HIP_EUNSUPPORTED with a message on
 *   an IVFFLAT, binary or 4-bit handle, on a list shard (gamma_hip_ivfpq_set_list_mask) and on a member of a group.
 *   Afterwards gamma_hip_ivfpq_add, _encode, _encode_each, _update_batch and the searches gamma_hip_ivfpq_search,
 *   _search_device, _search_device_wait rotate inside the library: their callers keep passing raw vectors.
 *   gamma_hip_ivfpq_train, gamma_hip_kmeans and gamma_hip_assign take vectors as given (the reference hands them the rotated
 *   set, gamma_index_ivfpq.cc:336-346); flat search is untouched.  GAMMA_HIP_EUNSUPPORTED with a message, never silent, on a
 *   handle with a matrix: the shard, merge and export entry points, gamma_hip_ivfpq_coarse_device and
 *   gamma_hip_ivfpq_set_list_mask.  A handle without a matrix takes exactly the paths it took before.
 * _get: 1 and the matrix in A_out (may be NULL) when one is set, 0 when none is, < 0 on error.
 * _apply: xt = x A^T for n host rows (the plugin rotates its training set with it); _apply_device: device pointers,
 *   enqueued on the handle's stream, no sync, x and xt distinct.  GAMMA_HIP_EINVAL without a matrix. */
int gamma_hip_opq_set(gamma_hip_index* h, const float* A);
int gamma_hip_opq_get(gamma_hip_index* h, float* A_out);
int gamma_hip_opq_apply(gamma_hip_index* h, int64_t n, const float* x, float* xt);
int gamma_hip_opq_apply_device(gamma_hip_index* h, int64_t n, const float* d_x, float* d_xt);
/* replaces OPQMatrix::train (faiss:VectorTransform.cpp:986-1200) as GammaIVFPQIndex::Indexing runs it on OPQMatrix(d, M_opq, d)
 * (gamma_index_ivfpq.cc:155-166,336-340): at most 65536 points (rand_perm, seed 1234), centred; a random orthonormal start
 * from a fixed seed; niter (<= 0: 50) alternations of { rotate; train an 8-bit PQ of M_opq sub-quantizers -- 256-centroid
 * k-means, 40 iterations in the first alternation and 4 afterwards from the previous centroids, max_points_per_centroid 1000;
 * encode and decode; the d x d cross-product of the set and its reconstruction; its orthogonal polar factor as the next
 * rotation }.  The set stays on the device for the rotation, the k-means, the assignment, the decode and the cross-product;
 * the polar factor is a one-sided Jacobi SVD in double on the host (in-tree: the library links no BLAS or LAPACK),
 * orthonormalised in double and rounded once to fp32.  The library's sgeqrf / sgesvd are not bit-reproducible across thread
 * counts (its own source says so, :997-1012), so parity with it is a matter of QUALITY -- the PQ error of the trained rotation
 * lies within the spread of the library's own runs from different starts (tests/test_gpu_opq_train.py) -- while two calls on
 * the same input return the same bytes.  x: n*d fp32 host, n >= 256 and d % M_opq == 0 (GAMMA_HIP_EINVAL with a message
 * otherwise); A_out: d*d row-major, xt = A x; objective_out (may be NULL): mean squared PQ error of the last alternation.
 * Needs no _init and changes nothing on the handle: set the result with gamma_hip_opq_set. */
int gamma_hip_opq_train(gamma_hip_index* h, int d, int64_t n, const float* x, int M_opq, int niter, float* A_out,
                        float* objective_out);
/* quantizer->xb (nlist*d), pq.centroids (M*ksub*dsub), and the precomputed table
 * (faiss:IndexIVFPQ.cpp:412-479; NULL => computed on device with identical arithmetic) */
int gamma_hip_ivfpq_set_trained(gamma_hip_index* h, const float* coarse_centroids,
                                const float* pq_centroids, const float* precomputed_table);
int gamma_hip_ivfpq_get_precomputed_table(gamma_hip_index* h, float* out);
/* L2 table mode (faiss::IndexIVFPQ::use_precomputed_table as train / Load leave it, faiss:IndexIVFPQ.cpp:132-135,
 * index/impl/gamma_index_ivfpq.cc:1033-1034).  Replaces the extern `faiss::precomputed_table_max_bytes`
 * (faiss:IndexIVFPQ.cpp:379, 2 GiB; process-wide here too): an index whose table nlist * nsubvector * 1 KiB would be
 * LARGER keeps mode 0 (faiss:IndexIVFPQ.cpp:441-449) -- no table is built or held, gamma_hip_ivfpq_get_precomputed_table
 * returns GAMMA_HIP_EUNSUPPORTED, and L2 searches score every (query, list) pair with the distance table of the residual
 * x - centroid (index/impl/gamma_index_ivfpq.h:239-245: compute_residual + pq.compute_distance_table, dis0 = 0), whose
 * fp32 values differ from mode 1's by rounding.  The rule is applied by gamma_hip_ivfpq_init (it depends on nlist, M and
 * the limit only): set the limit before Init.  _use_precomputed_table: 0 / 1, GAMMA_HIP_EINVAL before Init. */
int gamma_hip_set_precomputed_table_max_bytes(int64_t bytes);
int64_t gamma_hip_get_precomputed_table_max_bytes(void);
int gamma_hip_ivfpq_use_precomputed_table(gamma_hip_index* h);
/* shape of an initialised model: dimension, number of lists, bytes per code (nsubvector; 1 for IVFFLAT); 0 before Init */
int gamma_hip_ivfpq_dim(gamma_hip_index* h);
int gamma_hip_ivfpq_nlist(gamma_hip_index* h);
int gamma_hip_ivfpq_code_size(gamma_hip_index* h);

/* ---- realtime inverted lists (realtime::RTInvertIndex, realtime/realtime_invert_index.h)
 *      resident in HBM ----------------------------------------------------------------- */
/* RTInvertIndex::AddKeys for one bucket (realtime_mem_data.cc:264-303) */
int gamma_hip_ivfpq_add_keys(gamma_hip_index* h, int list_no, int n, const int64_t* vids,
                             const uint8_t* codes);
/* many buckets at once: vids/codes grouped by list, list_nos[i] has counts[i] entries */
int gamma_hip_ivfpq_add_keys_batch(gamma_hip_index* h, int nlists, const int32_t* list_nos,
                                   const int32_t* counts, const int64_t* vids,
                                   const uint8_t* codes);
/* RTInvertIndex::Update (realtime_mem_data.cc:305-327) */
int gamma_hip_ivfpq_update(gamma_hip_index* h, int list_no, int64_t vid, const uint8_t* code);
/* The two halves of Update for a list-sharded index, where the list a vector leaves and the list it joins may
 * live on different shards (gamma_amd/dist.py sharded_update): _has_vid: out[i] = 1 when this handle holds a live
 * entry of vids[i]; _remove: the first half of RealTimeMemData::Update (:318-321) alone -- the entry is flagged
 * as moved away and counted as deleted; unknown vids are ignored like Update ignores them (:307-311). */
int gamma_hip_ivfpq_has_vid(gamma_hip_index* h, const int64_t* vids, int n, uint8_t* out);
/* GammaIVFPQIndex::Update for a batch of n vectors (gamma_index_ivfpq.cc:375-422; the engine drains up to 20 000
 * updated vids per pass, vector/vector_manager.cc:355-380): every vector is assigned and encoded the way a call of
 * its own assigns it (quantizer->assign(1, ..), the exact form), in ONE device pass; then RTInvertIndex::Update for
 * each (vid, list, code) in order, one publish of the lists' tables, one wait for the device.  vecs: n*d fp32. */
int gamma_hip_ivfpq_update_batch(gamma_hip_index* h, int n, const int64_t* vids, const float* vecs);
/* the encode half alone (list_nos[n], codes[n*code_size] to host), and the list half alone with the codes supplied:
 * ops[i] = 0 Update (a vid this handle does not hold is ignored, realtime_mem_data.cc:307-311), 1 = the vid is held by
 * ANOTHER shard of a list-sharded index and joins list_nos[i] here (AddKeys), 2 = the vid leaves this shard (the first
 * half of Update: flagged as moved, counted as deleted); ops == NULL: all 0.  (gamma_hip_group_ivfpq_update) */
int gamma_hip_ivfpq_encode_each(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos, uint8_t* codes);
int gamma_hip_ivfpq_apply_updates(gamma_hip_index* h, int n, const int32_t* list_nos, const int64_t* vids,
                                  const uint8_t* codes, const uint8_t* ops);
int gamma_hip_ivfpq_remove(gamma_hip_index* h, int64_t vid);
/* RTInvertIndex::Delete (realtime_mem_data.cc:329-335,190-199): counter only */
int gamma_hip_ivfpq_delete(gamma_hip_index* h, const int64_t* vids, int n);
/* RTInvertIndex::CompactIfNeed (realtime_mem_data.cc:354-381,119-150); needs the delete
 * bitmap the handle mirrors */
int gamma_hip_ivfpq_compact_if_need(gamma_hip_index* h);
/* Extents abandoned by list growth and compaction (the reference frees them 1 s after the swap,
 * realtime_mem_data.cc:457-466) stay inside the arena until they exceed half of what is in use and
 * `min_waste_entries` (default 65536): then every list moves into a fresh tight arena.  out4 = {capacity, in use,
 * abandoned, repacks so far}, in list entries (code_size + 8 bytes each).  Setting the threshold re-checks at once. */
int gamma_hip_ivfpq_arena_stats(gamma_hip_index* h, int64_t* out4);
int gamma_hip_ivfpq_set_repack_threshold(gamma_hip_index* h, int64_t min_waste_entries);
/* out2 = {repack targets read back before their version of the list tables was published, read-backs that DIFFERED from
 * the source}.  A repack moves every list (realtime/realtime_mem_data.cc:426-474 swaps a bucket's pointer only after the
 * copy); the new version is published only after per-list checksums of ids + codes, recomputed through the new mapping in
 * a launch of their own, equal those of the source.  A difference keeps the old version, retires the target's address
 * ranges and repeats the move into ordinary allocations; the plugins log a non-zero second value. */
int gamma_hip_ivfpq_repack_verify_stats(gamma_hip_index* h, int64_t* out2);
/* How the arena grows: out2 = {growths that MOVED the arena (reallocation + copy under the exclusive lock), 1 when the
 * arena's arrays are mapped address ranges that grow in place (chunks mapped behind them: no copy, no second arena, no
 * wait for the searches in flight -- the reference grows bucket by bucket for the same reason,
 * realtime/realtime_mem_data.cc:152-188,426-474)}.  GAMMA_HIP_NO_ARENA_VMM=1 in the environment forces the fallback. */
int gamma_hip_ivfpq_arena_growth(gamma_hip_index* h, int64_t* out2);
int64_t gamma_hip_ivfpq_list_size(gamma_hip_index* h, int list_no);
int64_t gamma_hip_ivfpq_list_capacity(gamma_hip_index* h, int list_no);
/* RealTimeMemData::RetrieveCodes ("for unit test", realtime_mem_data.h:95-96) */
int gamma_hip_ivfpq_get_list(gamma_hip_index* h, int list_no, int64_t* vids, uint8_t* codes);
/* restrict the scan to the lists a shard owns (multi-GPU list sharding): owner[l] != 0.  With a mask
 * set, gamma_hip_ivfpq_add keeps only the vectors assigned to owned lists: every shard is handed the same
 * batch, which routes realtime inserts to the owner of the list without any exchange. */
int gamma_hip_ivfpq_set_list_mask(gamma_hip_index* h, const uint8_t* owned);

/* device-side Add path (gamma_index_ivfpq.cc:424-512): assign + residual + PQ encode +
 * AddKeys for n vectors with consecutive vids starting at first_vid. */
int gamma_hip_ivfpq_add(gamma_hip_index* h, int64_t n, const float* vecs, int64_t first_vid);
int gamma_hip_ivfpq_encode(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos,
                           uint8_t* codes);

/* Training helper (GammaIVFPQIndex::Indexing -> faiss::Clustering's assignment step,
 * gamma_index_ivfpq.cc:272-354): nearest of k centroids (squared L2, GEMM form on MFMA) for n
 * host vectors of dimension d; the Lloyd update stays on the host.  dis may be NULL. */
int gamma_hip_assign(gamma_hip_index* h, int d, int64_t n, const float* x, int k,
                     const float* centroids, int32_t* assign, float* dis);

/* Training on the device: faiss::Clustering::train (faiss:Clustering.cpp:255-560; nredo 1, L2, no weights) as
 * GammaIVFPQIndex::Indexing runs it through IndexIVFPQ::train (gamma_index_ivfpq.cc:272-354) -- subsample_training_set
 * to k * max_points_per_centroid with rand_perm(seed), centroids initialised from rand_perm(seed + 1), niter times
 * { assign (the coarse quantizer's kernels), compute_centroids (float sums in point order), split_clusters }.  The
 * training set is uploaded once; x: n*d fp32 host, centroids: k*d fp32 host out, objective (may be NULL): sum of the
 * distances of the last assignment.  Bit-identical to the oracle's go_kmeans, which is pinned against compiled faiss. */
int gamma_hip_kmeans(gamma_hip_index* h, int d, int64_t n, const float* x, int k, int niter, int64_t seed,
                     int max_points_per_centroid, float* centroids, float* objective);
/* IndexIVFPQ::train as GammaIVFPQIndex::Indexing runs it (index/impl/gamma_index_ivfpq.cc:272-354, faiss:IndexIVFPQ.cpp:
 * 67-131): coarse k-means (niter 10), residuals of at most 65536 subsampled points, one 256-centroid k-means (niter 25)
 * per sub-quantizer -- every k-means the gamma_hip_kmeans above.  x: n*d fp32 host; coarse: nlist*d, pq: M*256*(d/M) fp32
 * host out.  Bit-identical to the oracle's go_ivfpq_train, which is bit-identical to the compiled library's
 * IndexIVFPQ::train at its default BLAS threshold (tests/test_training_cpu.py). */
int gamma_hip_ivfpq_train(gamma_hip_index* h, int d, int64_t n, const float* x, int nlist, int M, float* coarse, float* pq);
/* faiss::rand_perm (faiss:utils/random.cpp:136-146; std::mt19937): the permutation IndexIVFPQ::train_residual_o
 * subsamples its training set with (host only) */
void gamma_hip_rand_perm(int32_t* perm, int64_t n, int64_t seed);

/* ---- multi-vector documents (VIDMgr, vector/raw_vector_common.h:36-110) -------------------------
 * A table whose documents carry several vectors per field has vid != docid; every validity test of the path --
 * the delete bitmap, the per-request range bitmaps, the device columns (GammaSearchCondition::IsValid,
 * common/gamma_common_data.h:99-108) and the realtime lists' delete accounting (realtime_mem_data.cc:102,294) --
 * is on the DOC id.  Append the docid of vids [count, count + n) in vid order; never called = single-vector
 * documents (docid == vid).  Labels returned by the searches stay vector ids, as in the reference. */
int gamma_hip_vid2docid_append(gamma_hip_index* h, int64_t n, const int32_t* docids);
int64_t gamma_hip_vid2docid_count(gamma_hip_index* h);

/* ---- IVFFLAT (index/impl/gamma_index_ivfflat.{h,cc}) ----------------------------------------
 * The reference's IVFFLAT lists carry the vectors themselves (code_size = 4 d, gamma_index_ivfflat.cc:155); here a
 * list carries vector ids (plus one dummy code byte so that the realtime-list code is shared) and the rows come
 * from the raw store (gamma_hip_raw_*), which must hold every indexed vector.  After _init the list entry points
 * above serve the handle unchanged: gamma_hip_ivfpq_add (= GammaIndexIVFFlat::Add :305-355: assign + AddKeys),
 * _encode (list_nos = quantizer->assign; codes = dummy bytes), _add_keys / _update / _delete /
 * _compact_if_need / _get_list / _list_size.  nprobe, metric, filters and the score window come from
 * gamma_hip_search_params (recall_num / has_rank are ignored: every scanned entry gets its exact distance). */
int gamma_hip_ivfflat_init(gamma_hip_index* h, int d, int nlist, int metric, int bucket_init_size,
                           int bucket_max_size);
/* quantizer->xb (nlist*d): IndexIVFFlat::train == the coarse k-means only */
int gamma_hip_ivfflat_set_trained(gamma_hip_index* h, const float* coarse_centroids);
/* replaces GammaIndexIVFFlat::Search (gamma_index_ivfflat.cc:392-421 + search_preassigned :423-612, pmode 0):
 * x nq*d fp32 host; distances/labels nq*k host, best first, -1 / heap neutral padded */
int gamma_hip_ivfflat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                             float* distances, int64_t* labels);
int gamma_hip_ivfflat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                    int k, float* d_distances, int64_t* d_labels);

/* ---- binary IVF (index/impl/gamma_index_binary_ivf.{h,cc}, faiss 1.7.1 IndexBinaryIVF) ------------------------------
 * Codes of nbits bits (nbits % 8 == 0, at most 2048; VectorValueType::BINARY), Hamming distances.  The lists are the
 * realtime lists of the other models with code_size = nbits / 8 (RTInvertIndex(nlist, code_size, ..), :103-106): after
 * _init the list entry points above serve the handle unchanged -- gamma_hip_ivfpq_add_keys(_batch), _delete (Delete
 * only counts, :275-279; this model never compacts), _get_list, _list_size, _list_capacity, _arena_stats.  The entry
 * points of the float models (PQ / IVFFLAT training, encode, add, update_batch, searches) answer GAMMA_HIP_EINVAL on a
 * binary handle.  Update, Dump and Load are no-ops in the reference (gamma_index_binary_ivf.h:99-104); they have no
 * counterpart here. */
/* replaces Init (:82-124): nlist = ncentroids, bucket_init_size = max(1000, indexing_size / ncentroids), bucket_max 1280000 */
int gamma_hip_binivf_init(gamma_hip_index* h, int nbits, int nlist, int bucket_init_size, int bucket_max_size);
/* replaces IndexBinaryIVF::train as Indexing runs it (:208-266, faiss:IndexBinaryIVF.cpp:241-280): the codes decoded to
 * +-1 on the device, the k-means of gamma_hip_kmeans (niter 10, seed 1234, 256 points per centroid; n == nlist copies),
 * real_to_binary.  codes: n x nbits / 8 host; centroid_codes: nlist x nbits / 8 host out.  Needs no _init. */
int gamma_hip_binivf_train(gamma_hip_index* h, int nbits, int64_t n, const uint8_t* codes, int nlist, uint8_t* centroid_codes);
/* quantizer->add of the trained centroid codes (nlist x nbits / 8) */
int gamma_hip_binivf_set_trained(gamma_hip_index* h, const uint8_t* centroid_codes);
/* replaces quantizer->search (IndexBinaryFlat::search, faiss:IndexBinaryFlat.cpp:33-59): the k nearest centroids of n
 * codes, best first, equal distances in the heap's order; k > nlist pads with label -1 / distance INT32_MAX.  k = 1 is
 * quantizer->assign (the lowest centroid index among equal distances).  distances may be NULL.  k <= 4096. */
int gamma_hip_binivf_assign(gamma_hip_index* h, int64_t n, const uint8_t* codes, int k, int32_t* distances, int64_t* labels);
/* replaces Add (:148-206): assign + AddKeys, vids first_vid .. first_vid + n - 1; GAMMA_HIP_ENOTTRAINED before training */
int gamma_hip_binivf_add(gamma_hip_index* h, int64_t n, const uint8_t* codes, int64_t first_vid);
/* replaces Search + search_knn_hamming_heap (:281-404): x nq x nbits / 8 host; distances / labels nq x k host, best first,
 * empty slots label -1 / distance 2147483648.0f ((float)INT32_MAX).  Of gamma_hip_search_params it uses nprobe (the
 * request's if it lies in (0, nlist], else 20), min_score / max_score (IsSimilarScoreValid on the Hamming distance; the
 * default window [FLT_MIN, FLT_MAX] excludes distance 0), the range filters, the device field and term filters; metric,
 * recall_num, has_rank, coarse_mode and exact_ties are ignored -- the reference's heap order is the only mode.
 * k > 4096 (the scan's heap is in LDS) or nprobe > 4096: GAMMA_HIP_EUNSUPPORTED. */
int gamma_hip_binivf_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* x, int k,
                            float* distances, int64_t* labels);
/* same, all pointers in device memory, enqueued on the handle's stream, no sync */
int gamma_hip_binivf_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int k,
                                   float* d_distances, int64_t* d_labels);
/* {queries searched, heap admissions of their scans} since the last reset (the serial part of a query's scan); counted
 * only by searches made while gamma_hip_profile_enable is on */
int gamma_hip_binivf_stats(gamma_hip_index* h, int64_t* out2, int reset);
/* Which kernels run GammaIVFBinaryScannerL2::scan_codes (gamma_index_binary_ivf.cc:333-448) for a search; the answer --
 * labels, distance bits, the order inside ties, the admissions gamma_hip_binivf_stats counts -- is the same in every mode.
 * 0: one wave per query walks its probed lists.  1: the query's row sequence (probed lists in coarse order, entries in list
 * order) is cut into chunks that never span two lists and spread over the device: per-chunk distance histograms, the
 * bounds they give, the rows below the bounds collected in order, the heap replayed over those alone (DESIGN.md section
 * 23); a call whose workspace (sized from nq x nprobe x the longest list, nothing is read back from the device) exceeds
 * half of gamma_hip_set_workspace_budget, or of more than 65535 queries, runs as mode 0.  -1 (the default): mode 1 for
 * calls of up to auto_max_nq queries (gamma_hip_binivf_scan_shape), mode 0 beyond.  Any other mode, or a handle that is
 * not a binary IVF handle: GAMMA_HIP_EINVAL.  GAMMA_HIP_NO_BIN_SPREAD=1 in the environment makes every mode run as 0. */
int gamma_hip_binivf_set_scan_mode(gamma_hip_index* h, int mode);
/* the mode set (-1, 0 or 1) of a binary IVF handle (the scans of gamma_index_binary_ivf.cc:333-448).  Any other handle
 * answers GAMMA_HIP_EINVAL, whose value is also the automatic mode's: ask binary IVF handles only. */
int gamma_hip_binivf_scan_mode(const gamma_hip_index* h);
/* the spread scan's shape (gamma_index_binary_ivf.cc:407-448 is the loop it spreads): *chunk_rows = rows per chunk,
 * *auto_max_nq = the largest call mode -1 spreads (measured).  Either pointer may be NULL. */
int gamma_hip_binivf_scan_shape(int* chunk_rows, int* auto_max_nq);
/* {queries the spread chain answered, their chunks, their candidates (rows replayed through scan_codes' heap,
 * gamma_index_binary_ivf.cc:407-448), queries that ran as mode 0 under mode 1 or -1 for lack of workspace} since the
 * last reset; counted only by searches made while gamma_hip_profile_enable is on */
int gamma_hip_binivf_scan_stats(gamma_hip_index* h, int64_t* out4, int reset);

/* ---- exact Hamming (binary flat) search (faiss:IndexBinaryFlat.cpp, utils/hamming.cpp:230-265) ------------------------
 * Every stored code in vid order, and over them the answer GammaIVFBinaryScannerL2::scan_codes
 * (gamma_index_binary_ivf.cc:333-448) gives for ONE list that holds every code in vid order: IsValid on the vid (delete
 * bitmap, range results including NOT, device columns, vid -> docid), the Hamming distance, IsSimilarScoreValid,
 * `dis < simi[0]` -> heap_pop + heap_push, heap_reorder -- labels and distance bits at every rank, ties included.  One
 * query is spread over the whole device. */
/* the store behind IndexBinaryFlat (faiss:IndexBinaryFlat.cpp: xb, code_size = nbits / 8).  nbits % 8 == 0, at most 2048.
 * On a fresh handle or on a binary IVF handle (before or after gamma_hip_binivf_init; the nbits must match); a handle of a
 * float model answers GAMMA_HIP_EINVAL.  Repeating the call with the same nbits is a no-op. */
int gamma_hip_binflat_init(gamma_hip_index* h, int nbits);
/* IndexBinaryFlat::add (faiss:IndexBinaryFlat.cpp).  codes: n x nbits / 8 host; the new vids are count .. count + n - 1.
 * A search never reads a half-written row: the rows go up on the writer stream and the count is published after them;
 * growth that frees or moves memory waits for the searches in flight. */
int gamma_hip_binflat_append(gamma_hip_index* h, int64_t n, const uint8_t* codes);
/* IndexBinaryFlat::ntotal: rows stored; -1 before _init */
int64_t gamma_hip_binflat_count(gamma_hip_index* h);
/* IndexBinaryFlat::search (faiss:IndexBinaryFlat.cpp, hammings_knn_hc faiss:utils/hamming.cpp:230-265) with the scanner's
 * admission and validity rules (gamma_index_binary_ivf.cc:333-448).  x nq x nbits / 8 host; distances / labels nq x k host,
 * best first, empty slots label -1 / distance 2147483648.0f ((float)INT32_MAX).  Of gamma_hip_search_params it uses
 * min_score / max_score (the default window [FLT_MIN, FLT_MAX] excludes distance 0), the range filters, the device field
 * and term filters; metric, nprobe, recall_num, has_rank, coarse_mode and exact_ties are ignored.  k > 4096:
 * GAMMA_HIP_EUNSUPPORTED.  The candidate counts of a call are data dependent; the queries run in sub-batches that fit
 * gamma_hip_set_workspace_budget (never wrong, only slower). */
int gamma_hip_binflat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* x, int k,
                             float* distances, int64_t* labels);
/* same, all pointers in device memory, on the handle's stream; the call reads its candidate totals back once per round
 * of queries (one small copy), what follows is enqueued without a sync */
int gamma_hip_binflat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int k,
                                    float* d_distances, int64_t* d_labels);
/* rows per chunk of the search kernels: the unit of the candidate bounds that let scan_codes' heap
 * (gamma_index_binary_ivf.cc:407-448) be replayed over a part of the rows only */
int gamma_hip_binflat_chunk_rows(void);
/* {queries searched, candidates collected, heap admissions of the replays (scan_codes' `dis < simi[0]`,
 * gamma_index_binary_ivf.cc:407-448), query sub-batches} since the last reset */
int gamma_hip_binflat_stats(gamma_hip_index* h, int64_t* out4, int reset);

/* ---- search ------------------------------------------------------------------------ */
/* replaces GammaIVFPQIndex::Search (gamma_index_ivfpq.cc:514-566 + search_preassigned
 * :701-890).  x: nq*d fp32 host; distances/labels: nq*k host, best first, unused slots
 * label -1 / distance = heap neutral (FLT_MAX for L2, -FLT_MAX for IP).
 * Re-entrant like the reference's Search: any number of threads may call it on one handle.  Calls of up to 256 queries
 * that find the handle busy are queued and run as ONE device batch per set of equal parameters (each caller gets the
 * result of its own call, bit for bit); a call that finds it idle runs on the caller's thread, its queries and results
 * staged in pinned memory (no pageable copies).  The buffers need not be pinned. */
int gamma_hip_ivfpq_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                           const float* x, int k, float* distances, int64_t* labels);
/* same, all pointers in device memory, enqueued on the handle's stream, no sync */
int gamma_hip_ivfpq_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                  const float* d_x, int k, float* d_distances, int64_t* d_labels);
/* Streaming callers of gamma_hip_ivfpq_search_device (exact ties on): with deferred replay the queries flagged for the
 * heap replay (a fraction of a percent; one query's replay is a ~0.2 ms chain of dependent sifts, §4 of DESIGN.md) are
 * redone on a side stream, and the handle's stream waits for them only before the next kernel that touches what the
 * replay reads -- in the NEXT call (or the next chunk of a large call), after its coarse quantizer and query tables.
 * The contract while it is on: d_distances / d_labels of a call are complete -- and d_x may be reused -- after the
 * next search call on the handle, gamma_hip_join (the handle's stream waits for the pending replay; no host wait) or
 * gamma_hip_synchronize.  Host-buffer calls are not affected.  Default: off. */
int gamma_hip_set_deferred_replay(gamma_hip_index* h, int on);
/* The reference's Search is re-entrant and returns a COMPLETE result to each of its client threads (tests/test.h:1033-1062,
 * tools/perf.cc:364-395).  _search_device_wait is that contract for device buffers: it returns when THIS call's
 * d_distances / d_labels are complete (it waits on the host for the call's own completion event) -- and while it waits
 * the handle is free: the tie replay of this call (serial by nature, ~200 waves on the whole device) runs on the side
 * stream and the NEXT caller's coarse quantizer, query tables and scan run beside it, exactly as under
 * gamma_hip_set_deferred_replay, with no contract on the callers but "wait for your own call".  Two client threads
 * alternating on one handle thus hide each other's replay tail; one thread alone gets what _search_device +
 * gamma_hip_synchronize gives.  d_x must stay untouched until the call returns.
 * Any number of callers may overlap, here and in gamma_hip_flat_search_device_wait: a call owns its completion event (and the
 * flat call its overflow word) from the moment it is enqueued until its own waiter is through with them; the handle creates
 * one such pair per call in flight at the same time and reuses them (call_slots.h). */
int gamma_hip_ivfpq_search_device_wait(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                       const float* d_x, int k, float* d_distances, int64_t* d_labels);
/* the same contract for the flat search (GammaFLATIndex::Search, gamma_index_flat.cc:118-300): complete on return, and the call's
 * heap replay -- a third of a 1024-query call over 1 M rows -- runs on the side stream beside the next caller's filter passes.
 * What the replay reads (the first row chunk's slab, the survivor log, the flag list, the candidate tables) exists twice: a call
 * that finds a flat replay pending works in the other bank. */
int gamma_hip_flat_search_device_wait(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                      const float* d_x, int k, float* d_distances, int64_t* d_labels);
int gamma_hip_join(gamma_hip_index* h);
/* stage outputs of the LAST search for parity tests / sharded merge (device->host):
 * coarse_dis/idx [nq*nprobe], recall_dis/ids [nq*recall_num] (sorted best first, -1 pad) */
int gamma_hip_ivfpq_last_stages(gamma_hip_index* h, float* coarse_dis, int64_t* coarse_idx,
                                float* recall_dis, int64_t* recall_ids);
/* sharded search, stage 1: coarse + owned-list scan + local top-recall_num, results left in
 * device buffers d_recall_dis/d_recall_ids [nq*recall_num] for the all-gather */
int gamma_hip_ivfpq_search_shard(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                 const float* d_x, int k, float* d_recall_dis,
                                 int64_t* d_recall_ids);
/* sharded search with the query batch split over the ranks: stage 0 = the coarse quantizer alone
 * (IndexFlatL2::search, faiss:IndexFlat.cpp:35-55) for this rank's slice of the queries; outputs
 * [nq*nprobe] in device memory, exchanged with an all-gather */
int gamma_hip_ivfpq_coarse_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                  const float* d_x, float* d_coarse_dis, int32_t* d_probe);
/* stage 1 with the coarse assignment supplied = search_preassigned restricted to the owned lists
 * (gamma_index_ivfpq.cc:701-890): tables + scan + local top-recall_num.  Enqueued like every device-pointer call, except
 * when the batch does not fit the workspace budget at the general slab stride (nprobe x the longest list; a W-rank job hands
 * every rank W x the queries but ~nprobe / W of their probes): then the longest candidate row of THIS batch over THIS shard's
 * lists is measured on the device and read back (one word; the call waits for the work enqueued before it) and stride and
 * chunks are sized by it -- full-size C4, 8 shards: 1-2 chunks instead of 20. */
int gamma_hip_ivfpq_search_shard_preassigned(gamma_hip_index* h, const gamma_hip_search_params* p,
                                             int nq, const float* d_x, const float* d_coarse_dis,
                                             const int32_t* d_probe, int k, float* d_recall_dis,
                                             int64_t* d_recall_ids);
/* Stage 1 in TWO PHASES with a bound of the GLOBAL recall_num-th best (round 6).  A list shard on its own can only
 * bound its LOCAL recall_num-th best -- with W shards about W times looser than what one GPU holding every list gets from
 * the query's nearest probes -- so all its probes take the expensive exact path and it exports recall_num candidates per
 * query of which the merge keeps ~1 / W.  Here the shard first scores only the query's nearest `GAMMA_HIP_SHARD_G1`
 * (default 2) probes it OWNS, which bound its local recall_num-th best exactly as the single-GPU producers do
 * (gamma_index_ivfpq.h:351-370: anything worse than the recall_num-th best seen can never enter the R-heap), writes that
 * bound per query to d_bound [nq] (+inf / -inf: none), and calls `reduce` ONCE: the caller's collective replaces d_bound[q]
 * by the minimum (L2; take_max = 0) or maximum (inner product; take_max = 1) over all shards -- every shard's value is an
 * upper bound of the global recall_num-th best, so the tightest one is too -- enqueued on `stream` (the handle's).
 * The shard's other probes then run as consumers of that bound (byte-table filter pass, list-major for long lists) and
 * the shard's table holds its candidates within the bound, best first, padded with (sentinel, -1): a SUPERSET of the
 * shard's part of the global top-recall_num, so the merge (gamma_hip_ivfpq_merge_rerank) and the tie machinery are
 * unchanged.  Results are identical to _search_shard_preassigned's after the merge.  `reduce` is called exactly once per
 * call -- with neutral values when the call cannot run in two phases (several chunks) -- so the shards' collectives
 * always pair up; NULL reduce = a single shard (the bounds stay local).  d_bound holds the reduced bounds on return
 * (stream order).  Replaces the per-shard scan of faiss:IndexShards.cpp:283-345 /
 * index/impl/gpu/gamma_gpu_cloner.cpp:200-253, where every shard scans with its own heap threshold. */
typedef int (*gamma_hip_bound_reduce_fn)(void* user, float* d_bound, int nq, int take_max, void* stream);
int gamma_hip_ivfpq_search_shard_bounded(gamma_hip_index* h, const gamma_hip_search_params* p,
                                         int nq, const float* d_x, const float* d_coarse_dis,
                                         const int32_t* d_probe, int k, float* d_recall_dis,
                                         int64_t* d_recall_ids, float* d_bound,
                                         gamma_hip_bound_reduce_fn reduce, void* user);
/* building block of a reduce callback without a collective library (the in-process group's peer-copy transport):
 * d_acc[i] = min (take_max = 0) / max (1) of d_acc[i] and d_in[i], i < n, enqueued on `stream` of the calling thread's
 * current device.  Takes no handle and no lock: it is called from inside _search_shard_bounded's callback. */
int gamma_hip_bound_combine(void* stream, float* d_acc, const float* d_in, int n, int take_max);
/* compute_dis's exact distances (gamma_index_ivfpq.cc:646-680: fvec_L2sqr / fvec_inner_product on the raw query, then
 * IsSimilarScoreValid) where the ROWS are: d_exact[q][r] for candidate d_ids[q][r] (device, [nq][R]; -1 = none) of query
 * d_x[q] -- the sentinel (+inf L2 / -inf inner product) for an empty slot, a score outside the request's window, or a vector
 * this handle's sharded store does not hold.  With raw vectors sharded by list owner every shard calls this on the candidates
 * it is about to send (after the two-phase scan: ~recall_num / W per query) and the distances travel with them. */
int gamma_hip_ivfpq_shard_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                const int64_t* d_ids, int R, float* d_exact);
/* gamma_hip_ivfpq_merge_rerank for candidates that arrive WITH their exact distances (d_all_exact laid out like d_all_dis):
 * the global top-recall_num by ADC value as ever, then compute_dis's k-heap fed from the travelled distances -- the owner of
 * the query slice needs no raw row.  Same results, flags and tie list as _merge_rerank on a handle that holds every row. */
int gamma_hip_ivfpq_merge_rerank_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq,
                                       const float* d_x, int k, const float* d_all_dis, const int64_t* d_all_ids,
                                       const float* d_all_exact, int q0, int nq_local, float* d_distances, int64_t* d_labels);
/* the tie phase with sharded raw vectors: after gamma_hip_ivfpq_shard_export the shard computes the exact distance (no score
 * window) of every exported entry whose ADC value lies within the query's bound d_bound_f[f] (NaN: of every entry) and whose
 * vector it holds -- the only entries that can end up in the recall_num-heap -- into d_ex [nf][stride], NaN elsewhere;
 * gamma_hip_ivfpq_merge_replay_exact assembles those streams beside the ADC values and the replay reads a member's distance
 * there instead of its row.  A member without a travelled distance fails the call (never silent). */
int gamma_hip_ivfpq_shard_export_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                       const float* d_vals, const int64_t* d_ids, const int32_t* d_off, int64_t stride,
                                       const float* d_bound_f, float* d_ex);
int gamma_hip_ivfpq_merge_replay_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf,
                                       const float* d_x_slice, int64_t stride, const float* d_vals_all, const int64_t* d_ids_all,
                                       const int32_t* d_off_all, const float* d_ex_all, int k, const int32_t* d_list,
                                       float* d_distances, int64_t* d_labels);
/* sharded search, stage 2: merge nshards*recall_num candidates per query (layout
 * [shard][nq][recall_num]) into the global top-recall_num, then compute_dis (re-rank or
 * truncate, gamma_index_ivfpq.cc:642-697) for queries [q0, q0+nq_local) */
int gamma_hip_ivfpq_merge_rerank(gamma_hip_index* h, const gamma_hip_search_params* p,
                                 int nshards, int nq, const float* d_x, int k,
                                 const float* d_all_dis, const int64_t* d_all_ids, int q0,
                                 int nq_local, float* d_distances, int64_t* d_labels);

/* replaces GammaFLATIndex::Search (gamma_index_flat.cc:118-300) over the raw store */
int gamma_hip_flat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                          const float* x, int k, float* distances, int64_t* labels);
int gamma_hip_flat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                 const float* d_x, int k, float* d_distances, int64_t* d_labels);

/* Test hook: n keys (smaller is better; payload = position) through ONE heap of k <= 1024 entries with one form of the
 * device's sifts -- op 0: heap_replace_top stream through the pipelined walk (csrc/heap_dev.h HeapWalk), 1: heap_pop +
 * heap_push through ParHeap (all lanes per sift), 2: the same through the sequential forms, 3: heap_replace_top through
 * ParHeap's sift, 4: faiss's ReservoirTopN (what knn_L2sqr collects through from 100 results on; arr = sorted = its
 * to_result output, n >= 1).  arr_*: the heap ARRAY when the stream is through ((FLT_MAX, -1) = empty); sorted_*: after heap_reorder.
 * tests/test_gpu_heaps.py compares them with the oracle's heaps (= the compiled library's, faiss:utils/Heap.h). */
int gamma_hip_debug_heap_stream(gamma_hip_index* h, int op, int k, int n, const float* vals, float* arr_vals, int32_t* arr_ids,
                                float* sorted_vals, int32_t* sorted_ids);
/* Exact ties across list shards.  gamma_hip_ivfpq_merge_rerank (exact ties on) leaves a list of the slice's queries whose
 * result a tie can change: two equal exact distances among the first k + 1 (or equal ADC distances among the taken ones
 * without re-rank), or the cut of the merged top-recall_num going through a group of equal distances (also when a shard's
 * own cut may have dropped members of the group).  Those are replayed through the reference's heaps over the stream its
 * scanner saw (faiss:utils/Heap.h:103-131, gamma_index_ivfpq.h:363-369, gamma_index_ivfpq.cc:664-696) -- which is
 * spread over the shards:
 *   shard_cut_flags after a shard search of nq queries: d_flags[q] != 0 = the shard's own top-recall_num cut went through
 *                   a group of equal distances (it may have dropped members of the group);
 *   merge_set_shard_flags  before merge_rerank: those flags of every shard for the merge's queries, [nshards][nq] (the
 *                   layout of d_all_dis without the recall_num axis); without them a shard table that ends at the merged
 *                   cut value is assumed to have cut a tie (more queries replayed, same results);
 *   merge_flagged   n_flagged (host; waits for the handle's stream) and the device list of flagged slice-local query
 *                   indices (valid until the next search-type call on the handle);
 *   gather_rows     d_dst[i] = row d_list[i] of d_src (rows of row_words 32-bit words): the flagged queries' vectors and
 *                   assignment rows for the shards;
 *   shard_export_rows  on every shard: the longest export row of the nf flagged queries (entries of the probed lists this
 *                   shard owns; host value, waits for the stream): the callers take `stride` = the maximum over the shards;
 *   shard_export    on EVERY shard: for the nf flagged queries (vectors d_xf, assignment d_cdis_f / d_probe_f [nf][nprobe])
 *                   the ADC distances (+-inf = filtered entry) and vector ids of the probed lists this shard owns, in list
 *                   order: rows of `stride` entries, d_off[f][p .. p + 1) = the entries of probe p (empty for a list of
 *                   another shard);
 *   merge_replay    on the slice's owner: the exports of all shards ([nshards][nf][stride], [nshards][nf][nprobe + 1])
 *                   are assembled probe by probe into the streams and replayed; rows d_list[f] of d_distances /
 *                   d_labels (the slice's result rows) are rewritten.  d_x_slice: the slice's query vectors. */
int gamma_hip_ivfpq_shard_cut_flags(gamma_hip_index* h, int nq, uint8_t* d_flags);
int gamma_hip_ivfpq_merge_set_shard_flags(gamma_hip_index* h, const uint8_t* d_flags);
int gamma_hip_ivfpq_merge_flagged(gamma_hip_index* h, int* n_flagged, const int32_t** d_list);
int gamma_hip_gather_rows(gamma_hip_index* h, const void* d_src, int row_words, const int32_t* d_list, int n, void* d_dst);
int gamma_hip_ivfpq_max_list_len(gamma_hip_index* h);
int gamma_hip_ivfpq_shard_export_rows(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const int32_t* d_probe_f,
                                      int64_t* max_entries);
int gamma_hip_ivfpq_shard_export(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                 const float* d_cdis_f, const int32_t* d_probe_f, int64_t stride, float* d_vals,
                                 int64_t* d_ids, int32_t* d_off);
int gamma_hip_ivfpq_merge_replay(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf,
                                 const float* d_x_slice, int64_t stride, const float* d_vals_all, const int64_t* d_ids_all,
                                 const int32_t* d_off_all, int k, const int32_t* d_list, float* d_distances,
                                 int64_t* d_labels);

/* ---- IVFFLAT over list shards: one handle per shard (gamma_hip_ivfpq_set_list_mask), the single-handle building blocks.
 * Every pointer is a device address.  The rows of a shard come from a dense store (rows replicated on every shard) or from a
 * SPARSE one (gamma_hip_raw_put: the rows live with their lists): fp32 rows, or -- after gamma_hip_set_ivfflat_narrow_rows(h, 1),
 * where the single-handle search serves them -- float16 / uint8 / int8 rows, widened exactly as they are loaded (results
 * byte-identical to shards holding the widened rows as fp32).  With that switch off a float16 or 8-bit store answers
 * GAMMA_HIP_EUNSUPPORTED with last_error naming the store, and an sq8 store always does (ivfflat_search_shard and
 * ivfflat_shard_export: the entries that read rows).  Limits on k and nprobe are gamma_hip_ivfflat_search's.  What the
 * existing entries answer is unchanged: gamma_hip_ivfflat_search* on a sparse store stays refused.
 *   ivfflat_coarse_device  the coarse quantizer alone for a slice of the queries, [nq * nprobe] outputs
 *                   (gamma_hip_ivfpq_coarse_device refuses an IVFFLAT handle; this is its sibling);
 *   ivfflat_search_shard   search_preassigned (index/impl/gamma_index_ivfflat.cc) restricted to the lists this handle holds
 *                   and its mask owns -- what faiss:IndexShards.cpp:283-345 / index/impl/gpu/gamma_gpu_cloner.cpp:200-253 run
 *                   per shard: [nq][k] best first, padded with (neutral, -1), the score window applied in the scan, local exact
 *                   ties honoured as in the single-handle search.  The list-major kernels serve it under a mask (an unowned list
 *                   is an empty list).  d_coarse_dis is not read (kept for the shape of the IVFPQ entry; may be null).  With
 *                   exact ties on it leaves one cut flag per query of the whole call, whatever the chunking
 *                   (gamma_hip_set_workspace_budget): the shard's own k cut went through a group of equal distances;
 *   gamma_hip_ivfpq_shard_cut_flags / _merge_set_shard_flags / _merge_flagged / gamma_hip_gather_rows serve an IVFFLAT handle
 *                   as they are (they read nothing of the model): the flags after ivfflat_search_shard, before / after
 *                   ivfflat_merge;
 *   ivfflat_merge   the W x k candidates per query, [shard][nq][k], for queries [q0, q0 + nq_local): the global top-k best first,
 *                   padded with (neutral, -1).  With exact ties on a query is FLAGGED when two of the merged first k + 1
 *                   distances are equal -- two equal among the k taken, or the merged cut passing through a group of equal
 *                   distances -- or when a shard table whose own cut went through a tie (its cut flag; without the shards' flags
 *                   every table counts) ends at the merged k-th value.  With exact_ties off the result is the merged top-k:
 *                   distances identical to one handle's at every rank, ids possibly different inside groups of equal distances;
 *   ivfflat_shard_export_rows / _shard_export  on EVERY shard for the nf flagged queries: the longest export row (host value),
 *                   and the rows: exact distances (+-inf = filtered, deleted, superseded or outside the window) and vector ids
 *                   of the probed lists this shard holds, in list order, rows of `stride` entries, d_off[f][p .. p + 1) = probe p
 *                   (empty for a list of another shard) -- gamma_hip_ivfpq_shard_export's layout;
 *   ivfflat_merge_replay   on the slice's owner: the exports are assembled probe by probe into the stream the reference's
 *                   scanner saw and replayed through ITS heap -- heap_pop + heap_push when dis < top, then heap_reorder
 *                   (index/impl/gamma_index_ivfflat.h:52-75), not the IVFPQ scanner's heap_replace_top; rows d_list[f] of
 *                   d_distances / d_labels are rewritten. */
int gamma_hip_ivfflat_coarse_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                    float* d_coarse_dis, int32_t* d_probe);
int gamma_hip_ivfflat_search_shard(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                   const float* d_coarse_dis, const int32_t* d_probe, int k, float* d_dis, int64_t* d_ids);
int gamma_hip_ivfflat_shard_export_rows(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const int32_t* d_probe_f,
                                        int64_t* max_entries);
int gamma_hip_ivfflat_shard_export(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                   const int32_t* d_probe_f, int64_t stride, float* d_vals, int64_t* d_ids, int32_t* d_off);
int gamma_hip_ivfflat_merge(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq, int k,
                            const float* d_all_dis, const int64_t* d_all_ids, int q0, int nq_local, float* d_distances,
                            int64_t* d_labels);
int gamma_hip_ivfflat_merge_replay(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf,
                                   const float* d_x_slice, int64_t stride, const float* d_vals_all, const int64_t* d_ids_all,
                                   const int32_t* d_off_all, int k, const int32_t* d_list, float* d_distances,
                                   int64_t* d_labels);

/* ---- several GPUs in ONE process: a group of handles, the index sharded by IVF list ----------------------------
 * What the reference's GPU model does with faiss's IndexShards / GpuClonerOptions (index/impl/gpu/gamma_gpu_cloner.cpp:200-269,
 * index/impl/gpu/gamma_index_ivfpq_gpu.cc:356-436, faiss:IndexShards.cpp:283-345): one index object, a host thread per
 * GPU, every search fanned out and merged.  Here member i is an ordinary handle on devices[i] (several members may
 * share a device: tests) that owns the lists owner(l) == i; centroids, codebooks, T2, the delete bitmap and the raw
 * vectors are replicated (broadcast the replicated state yourself through gamma_hip_group_member, as the plugins do).
 * A search: every member runs the coarse quantizer for its slice of the queries, the assignment is exchanged
 * (device-to-device copies), every member scans the probed lists it owns for the whole batch and keeps a local
 * top-recall_num, each member pulls the candidates of ITS query slice from all members, merges them (k_merge_shards) and
 * runs compute_dis, then the tie phase above (flagged queries' streams exported by every member, replayed at the owner).
 * Results equal those of one handle holding every list.  The multi-process form of the same steps over RCCL is gamma_amd/dist.py.
 * Threading: group-level calls (search, add, update, delete, compaction) may come from any thread but run ONE AT A TIME
 * (a call occupies every member's worker thread and their barriers): concurrent client threads queue behind each other
 * and behind the indexing thread, and small calls are not combined -- batch queries above the group, as the reference's
 * GPU model does (its GPUItem queue, index/impl/gpu/gamma_index_ivfpq_gpu.cc:356-436).  A member that fails in any phase
 * ends the call with that member's error on every thread (the go / no-go of each phase is one snapshot all members share). */
typedef struct gamma_hip_group gamma_hip_group;
int gamma_hip_group_create(const int* devices, int n, gamma_hip_group** out);
int gamma_hip_group_destroy(gamma_hip_group* g);
int gamma_hip_group_size(const gamma_hip_group* g);
gamma_hip_index* gamma_hip_group_member(gamma_hip_group* g, int i);
const char* gamma_hip_group_last_error(gamma_hip_group* g);
/* Transport of the two exchanges of a sharded search (the assignment, the per-shard top-recall_num tables of every owner's
 * slice).  0 (default): device-to-device copies ordered by events and host barriers.  1: RCCL over xGMI -- ONE in-place
 * ncclAllGather of the assignment and one grouped ncclSend / ncclRecv exchange of the tables, one communicator per member
 * (ncclCommInitAll), resolved from librccl.so at run time; formed at the next sharded search, and only when every member
 * has a device of its own (otherwise, or when the library cannot be loaded, the group stays on copies and says why in
 * gamma_hip_group_transport_note).  The environment variable GAMMA_HIP_GROUP_RCCL=1 selects 1 for every new group.
 * gamma_hip_group_transport: out2 = {1 when a communicator is in use, searches whose exchanges went through RCCL}.
 * The rare tie-phase exports stay on copies.  Results do not depend on the transport. */
int gamma_hip_group_set_transport(gamma_hip_group* g, int rccl);
int gamma_hip_group_transport(gamma_hip_group* g, int64_t* out2);
const char* gamma_hip_group_transport_note(gamma_hip_group* g);
/* list -> member.  weights[nlist] (expected or actual list sizes: the training set's assignment counts, the sizes in a
 * dump) are balanced greedily, heaviest list first -- probe popularity follows list size, so this balances scan
 * bytes; NULL: l mod n.  Call once, after gamma_hip_ivfpq_init on every member and before the first Add. */
int gamma_hip_group_set_owners(gamma_hip_group* g, const int64_t* weights);
/* Placement, before gamma_hip_group_set_owners.  0 (default): sharded by list as above.  1: REPLICATED -- every member
 * holds every list (Add / AddKeys / Update / Delete go to all members, one encode), a search splits the QUERIES: member
 * i answers its slice with the ordinary single-handle search, so results are those of one handle bit for bit (exact
 * ties included) and nothing is exchanged but the slice and its k results.  The choice for an index that is small next
 * to one GPU's memory: list sharding leaves the per-query fixed work (table, bound, selection) on every member for
 * every query, replicas divide it (multi-GPU).  The per-list getters read member 0. */
int gamma_hip_group_set_placement(gamma_hip_group* g, int replicate);
int gamma_hip_group_placement(const gamma_hip_group* g);
int gamma_hip_group_owner(const gamma_hip_group* g, int list_no);
/* GammaIVFPQIndex::Add: ONE encode (members take turns), then AddKeys at the owner of every assigned list */
int gamma_hip_group_ivfpq_add(gamma_hip_group* g, int64_t n, const float* vecs, int64_t first_vid);
/* AddKeys / list read-back at the owner (Load / Dump) */
int gamma_hip_group_ivfpq_add_keys(gamma_hip_group* g, int list_no, int n, const int64_t* vids, const uint8_t* codes);
int64_t gamma_hip_group_ivfpq_list_size(gamma_hip_group* g, int list_no);
int gamma_hip_group_ivfpq_get_list(gamma_hip_group* g, int list_no, int64_t* vids, uint8_t* codes);
/* GammaIVFPQIndex::Update: one encode; the member holding the old entry flags it, the owner of the new list appends */
int gamma_hip_group_ivfpq_update(gamma_hip_group* g, int n, const int64_t* vids, const float* vecs);
int gamma_hip_group_ivfpq_delete(gamma_hip_group* g, const int64_t* vids, int n);
int gamma_hip_group_ivfpq_compact_if_need(gamma_hip_group* g);
/* GammaIVFPQIndex::Search over all members; host buffers as gamma_hip_ivfpq_search */
int gamma_hip_group_ivfpq_search(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* x, int k,
                                 float* distances, int64_t* labels);
/* the same with the queries and the result buffers in the memory of member 0's device; returns when the results are there */
int gamma_hip_group_ivfpq_search_device(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* d_x,
                                        int k, float* d_distances, int64_t* d_labels);
/* GammaIVFFlatIndex::Search over all members (members initialised with gamma_hip_ivfflat_init; the storage entries above
 * -- gamma_hip_group_ivfpq_add / _add_keys / _get_list / _update / _delete / _compact_if_need, gamma_hip_group_raw_put -- serve
 * IVFFLAT members unchanged: code_size is 1, the codes are dummies).  The IVFPQ search's sequence with the same barriers: every
 * member runs the coarse quantizer of its slice (coarse_mode resolved on the whole call's nq), the assignment is exchanged, every
 * member runs gamma_hip_ivfflat_search_shard over the whole batch -- rows from its dense store (raw placement 0) or from its
 * sparse one (raw placement 1) -- each member pulls the [W][per][k] tables and cut flags of its slice, merges
 * (gamma_hip_ivfflat_merge) and the tie phase runs in rounds of at most 256 flagged queries (_shard_export / _merge_replay).
 * Results equal one handle's at every rank, exact ties included.  A member that fails in any phase still arrives at every
 * meeting point, and the call returns that member's error.  With gamma_hip_group_set_placement(1) every member answers its
 * slice with gamma_hip_ivfflat_search_device.  The exchanges are device-to-device copies ordered by events; a group set to RCCL
 * uses copies for these calls all the same and says so in gamma_hip_group_transport_note.  A library built without the
 * IVFFLAT shard entries answers GAMMA_HIP_EUNSUPPORTED. */
int gamma_hip_group_ivfflat_search(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* x, int k,
                                   float* distances, int64_t* labels);
/* the same with the queries and the result buffers in the memory of member 0's device; returns when the results are there */
int gamma_hip_group_ivfflat_search_device(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* d_x,
                                          int k, float* d_distances, int64_t* d_labels);
int64_t gamma_hip_group_total_mem_bytes(gamma_hip_group* g);
/* Raw vectors of a list-sharded group.  0 (default): REPLICATED -- every member mirrors every row (the caller writes them
 * through gamma_hip_group_member, as the plugins do).  1: SHARDED -- every row lives exactly once, in the sparse store
 * (gamma_hip_raw_put) of the member that owns its vector's list: gamma_hip_group_ivfpq_add puts the rows beside the keys,
 * gamma_hip_group_ivfpq_update rewrites the row of a vector that stays on its member in place and moves the row of one that
 * leaves (put at the new owner, gamma_hip_raw_drop at the old one), and a has_rank search computes the exact distances where
 * the rows are (gamma_hip_ivfpq_shard_exact / _shard_export_exact) and sends them with the candidates to the owner of the
 * query slice (_merge_rerank_exact / _merge_replay_exact); with has_rank = 0 nothing more is computed or sent.  Results stay
 * those of one handle holding every list and every row.  Allowed only while no member holds a row and not together with
 * gamma_hip_group_set_placement(1) (GAMMA_HIP_EINVAL); every member's raw store must be initialised (gamma_hip_raw_init). */
int gamma_hip_group_set_raw_placement(gamma_hip_group* g, int sharded);
int gamma_hip_group_raw_placement(const gamma_hip_group* g);
/* rows for callers that add keys without vectors (gamma_hip_group_ivfpq_add_keys after a Load): row vecs[i] goes to the member
 * that lists vector id vids[i] (gamma_hip_ivfpq_has_vid); ids nobody lists are skipped and counted in *n_skipped (may be NULL).
 * Sharded raw placement only. */
int gamma_hip_group_raw_put(gamma_hip_group* g, int64_t n, const int64_t* vids, const float* vecs, int64_t* n_skipped);

/* ---- accounting (GetTotalMemBytes, index/retrieval_model.h:287; PerfTool :23-50) ------ */
int64_t gamma_hip_total_mem_bytes(gamma_hip_index* h);
/* per-stage HIP-event timing of the kernels launched by search calls */
#define GAMMA_HIP_STAGE_COARSE 0
#define GAMMA_HIP_STAGE_TABLES 1
#define GAMMA_HIP_STAGE_SCAN 2
#define GAMMA_HIP_STAGE_SELECT 3
#define GAMMA_HIP_STAGE_RERANK 4
#define GAMMA_HIP_STAGE_FLAT 5
#define GAMMA_HIP_NUM_STAGES 6
/* on: 0 off; 1 every stage, plus the counter of scanned codes behind gamma_hip_profile_scan_bytes; 2 the scan stage alone --
 * two events around the scan launch and nothing else.  (Under rocprofv3's kernel trace an event pair between two kernels
 * shows as a 10-16 us gap; without the tracer the call rate is the same with 0, 1 and 2 -- bench.py --timed-events, 60
 * steps of 16384 queries each: 1.635 / 1.629 / 1.642 ms.) */
int gamma_hip_profile_enable(gamma_hip_index* h, int on);
int gamma_hip_profile_reset(gamma_hip_index* h);
/* total milliseconds and number of timed launches of a stage since the last reset;
 * scan_bytes = algorithmic list-scan bytes (sum over probed pairs of len*code_size) */
int gamma_hip_profile_get(gamma_hip_index* h, int stage, double* total_ms, int64_t* launches);
int gamma_hip_profile_scan_bytes(gamma_hip_index* h, int64_t* bytes, int64_t* pairs);

#ifdef __cplusplus
}
#endif
#endif /* GAMMA_HIP_H_ */
