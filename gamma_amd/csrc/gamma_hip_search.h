// gamma_hip_search.h -- what the search translation units of libgamma_hip.so share: gamma_hip_search.cpp (filters, the
// helpers below, the IVFPQ pipeline and its entry points), gamma_hip_search_ivfflat.cpp, gamma_hip_search_flat.cpp,
// gamma_hip_search_shard.cpp (list shards, merge, export, replay), gamma_hip_combine.cpp (the combining queue of small
// concurrent calls) and the binary searches (gamma_hip_binivf.cpp, gamma_hip_binflat.cpp).  Everything declared here is
// defined in gamma_hip_search.cpp unless a comment names another unit.
#pragma once
#include "gamma_hip_internal.h"
#include "pq4.h"

namespace ghi {

// What the scan needs to know about the validity predicates of a call: the device filter table, the
// optional query -> entry map (combined batches of requests with their own filters), and whether
// anything but the delete bitmap can reject an entry.
struct FiltCtx {
    const gh::FilterDesc* d_tab = nullptr;
    const int* d_qf = nullptr;
    bool any_clause = false;
    FiltCtx at(int q0) const {   // the same context for the queries from q0 on
        FiltCtx c = *this;
        if (c.d_qf) c.d_qf += q0;
        return c;
    }
};

int build_filter(H* h, const gamma_hip_search_params* p, gh::FilterDesc* f, size_t* off_io = nullptr, int64_t est_codes = 0);
int filt_ctx_single(H* h, const gh::FilterDesc& f, FiltCtx* c);
int check_params(H* h, const gamma_hip_search_params* p, int nq, int k);
int ivfpq_check(H* h, const gamma_hip_search_params* p, int nq, int k);

// A request's exact-ties choice (gamma_hip_search_params.exact_ties: 0 = the handle's setting, 1 on, -1 off) is resolved
// ONCE per call, at the entry point, into the call's own copy of the parameter block (exact_ties = 1 / -1); everything
// below reads tie_on(p) -- the handle is not touched.  in_range: the shape is one the replay covers (every recall_num / k
// the ABI accepts; nprobe <= 1024).  Beyond it a request that asked for the mode explicitly gets GAMMA_HIP_EUNSUPPORTED;
// one that relies on the handle's default runs with the (distance, position) order inside ties and is COUNTED
// (gamma_hip_ties_not_honoured) -- never silently.
static inline bool tie_on(const gamma_hip_search_params* p) { return p->exact_ties > 0; }
int resolve_ties(H* h, const gamma_hip_search_params* p, gamma_hip_search_params* pp, bool in_range, const char* what);

// what a result slot without an entry holds before the output kernels turn it into the reference's empty slot
static inline float neutral_of(bool l2) { return l2 ? 3.402823466e+38f : -3.402823466e+38f; }

// the assignment is complete on the stream (the heap replay of tied rows may still be running on the side stream)
int coarse_join(H* h);
// defer_join: the caller has kernels to launch that do not read the assignment and calls coarse_join itself
int ivfpq_coarse(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, float* out_dis = nullptr,
                 int* out_probe = nullptr, bool defer_join = false);

// Two-phase list-shard search (round 6): between the producers (the query's nearest probes OWNED BY THIS SHARD: they
// bound the shard's recall_num-th best) and the consumers (all its other probes) the bounds of all shards are reduced
// -- min for L2, max for inner product: one float per query -- so that every shard filters against a bound of the GLOBAL
// recall_num-th best instead of its own, W times looser one.  `reduce` is the caller's collective (RCCL all-reduce in
// gamma_amd/dist.py, peer reads in the in-process group); it is called exactly ONCE per shard call, with neutral values
// when this call cannot run in two phases.
struct BoundXchg {
    float* d_bound = nullptr;                  // [nq of the whole call] the caller's buffer; holds the reduced bounds afterwards
    gamma_hip_bound_reduce_fn fn = nullptr;
    void* user = nullptr;
    bool called = false;
    bool two_phase = false;                    // this call runs in two phases (one chunk, bounded scan possible)
    int P_in = 0;                              // row length of the supplied assignment (p->nprobe is the compacted rows')
    int G1 = 2;                                // probes of the producers' group
    int reduce(H* h, int nq, bool l2) {
        called = true;
        const int rc = fn ? fn(user, d_bound, nq, l2 ? 0 : 1, (void*)h->stream) : 0;
        return rc ? fail(h, GAMMA_HIP_EDEVICE, "bound reduction callback failed") : GAMMA_HIP_OK;
    }
};

// a 4-bit handle (gamma_hip_ivfpq4_init) behind an entry point that is 8-bit only: never silent
static inline int pq4_refuse(H* h, const char* what) {
    h->err = std::string("4-bit handle: ") + what + " is 8-bit only";
    return GAMMA_HIP_EUNSUPPORTED;
}
// a handle with an OPQ matrix (gamma_hip_opq_set) behind an entry point that takes vectors or candidates of several handles:
// the list shards and their merge rotate nothing -- refused, never silent
static inline int opq_refuse(H* h, const char* what) {
    h->err = std::string("handle with an OPQ matrix: ") + what + " is not supported";
    return GAMMA_HIP_EUNSUPPORTED;
}
// (every entry point that refuses the one refuses the other: the shard, merge and export entries)
#define GH_NO_PQ4(h, what)                                                \
    do {                                                                  \
        if ((h)->ksub == gh::kPq4Ksub) return pq4_refuse((h), (what));    \
        if ((h)->d_opq) return opq_refuse((h), (what));                   \
    } while (0)

// A narrow raw store behind a reader of fp32 rows -- float16 (gamma_hip_raw_init_f16), uint8 / int8 (gamma_hip_raw_init_i8)
// or scalar-quantised (gamma_hip_raw_init_sq8): the exact re-rank of the IVFPQ search and its tie replay read such rows,
// the flat and IVFFLAT searches where their switch says so, nothing else does -- refused, never silent.
// Is the handle's store one the search reads?  narrow_rows / sq8_rows: the search's switches for the two kinds of narrow
// store (false: the search has no reader for them).
static inline bool raw_store_served(const H* h, bool narrow_rows, bool sq8_rows) {
    if (h->raw_et == gh::ROW_SQ8) return sq8_rows;
    if (h->raw_narrow()) return narrow_rows;   // float16, uint8, int8
    return true;   // fp32 rows
}
// the shard's exact entries (gamma_hip_ivfpq_shard_exact / _shard_export_exact): fp32 rows always, a narrow store of either kind
// after gamma_hip_set_sparse_narrow_rows
static inline bool shard_exact_served(const H* h) { return raw_store_served(h, h->sparse_narrow_rows, h->sparse_narrow_rows); }
static inline int raw_store_refuse(H* h, const char* what) {
    const int t = h->raw_elem_type();
    const char* store = t == 4 ? "sq8 raw store (gamma_hip_raw_init_sq8): "
                        : t == 1 ? "float16 raw store (gamma_hip_raw_init_f16): "
                                 : "8-bit raw store (gamma_hip_raw_init_i8): ";
    h->err = std::string(store) + what + " reads fp32 rows and is not supported";
    return GAMMA_HIP_EUNSUPPORTED;
}

// ---- IVFPQ stages (bodies in gamma_hip_search.cpp) ----
// pre_dis / pre_probe: coarse assignment computed elsewhere (sharded search: the rank owning the
// query slice), device pointers [nq*nprobe]; nullptr = run the coarse quantizer here
int ivfpq_stage_a(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nq,
                  const float* d_x, int R, const float* pre_dis = nullptr, const int* pre_probe = nullptr,
                  bool shard = false, float* out_dis = nullptr, int64_t* out_ids = nullptr, BoundXchg* bx = nullptr);
// tie_mode 1: flag + replay; 2: flag only (merge of shards: w_tcut / w_tlist set up by the caller)
int ivfpq_stage_b(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int R, int k,
                  const float* cand_dis, const int64_t* cand_ids, float* d_distances,
                  int64_t* d_labels, const int* qperm = nullptr, int tie_mode = 0);

// queries per internal chunk: the coarse distance matrix (nlist floats per query) and the ADC distance
// slab (nprobe x longest list floats per query) each stay inside the workspace budget
int coarse_chunk(H* h, int nq);
int scan_chunk(H* h, int nq, int P);
int query_chunk(H* h, int nq, int P);

// floats per query of the distance slab of a call that scans P lists per query: P x the longest list, rows 16-byte aligned
// (the small-batch chains and the IVFFLAT search; ivfpq_stage_a caps its own by the measured stride, scan_chunk sizes
// chunks by the unrounded product)
static inline int64_t slab_q_stride(const H* h, int P) {
    return (std::max<int64_t>(1, (int64_t)P * std::max(1, h->max_list_len)) + 3) & ~(int64_t)3;
}
// long candidate rows of the small-batch chains: two-level selection (select.hip, slices of SM_SLICE = 16384 positions);
// how many slices per query, 0 = one level
static inline int small_presel_slices(const H* h, int P, int nq) {
    const int64_t slice = 16384;   // select.hip SM_SLICE
    const int64_t est = (int64_t)P * (h->ntotal / std::max(1, h->nlist)) * 3 / 2;
    const int64_t bound = (int64_t)P * std::max(1, h->max_list_len);
    if (h->small_presel > 0) return h->small_presel;
    if (est > slice) return (int)std::min<int64_t>(std::min<int64_t>(64, (bound + slice - 1) / slice), std::max(2, 4096 / nq));
    return 0;
}

// Large filtered batches: the lists are cut down to the entries that pass -- once per call, the predicate does not
// depend on the query (kernels.hip k_compact_lists) -- and the call runs unfiltered over the shadow lists.  Worth it
// when the call tests several times as many entries as the index holds; GAMMA_HIP_LIST_COMPACT=0/1 never / always.
// The handle's list pointers are swapped until the ListCompaction object goes out of scope (the caller holds the
// search lock and h->mu for the whole enqueue).
struct ListCompaction {
    H* h;
    uint8_t* codes;
    int64_t* ids;
    int* len;
    float* sums;
    bool on = false;
    explicit ListCompaction(H* h_) : h(h_), codes(h_->d_codes), ids(h_->d_ids), len(h_->d_list_len), sums(h_->d_sums) {}
    ~ListCompaction() {
        if (on) {
            h->d_codes = codes;
            h->d_ids = ids;
            h->d_list_len = len;
            h->d_sums = sums;
            h->prefiltered = false;
            h->cmp_has_sums = false;
        }
    }
};
int compact_lists_for_call(H* h, FiltCtx* fc, int64_t est, bool allowed, ListCompaction* lc);

// the replay of a query of the exact scanners (IVFFLAT: P > 0, the slab in probe order; flat: P == 0, fixed_n rows in
// vid order): the k-heap IS the result heap, score window and filters are already in the slab (sentinels)
void flat_tie_args(H* h, gh::TieReplayArgs* tr, bool l2, int nq, int64_t q_stride, int P, int k, const float* d_x, float* cand_dis,
                   int64_t* cand_ids, float* d_distances, int64_t* d_labels, int fixed_n = 0);
// given != nullptr: the filter context of a combined batch (p's own filter clauses are ignored)
int ivfpq_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int k, float* d_distances,
                               int64_t* d_labels, const FiltCtx* given = nullptr);
int flat_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int k, float* d_distances,
                              int64_t* d_labels);
// a whole host-buffer call on the caller's thread (search lock, staging, wait)
int flat_search_host_locked(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                            float* distances, int64_t* labels);
int ivfpq_search_host_locked(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                             float* distances, int64_t* labels);
// small host-buffer calls that find the handle busy share device batches (gamma_hip_combine.cpp); kind 0 IVFPQ, 1 flat
constexpr int COMB_MAX_NQ = 256, COMB_MAX_TOTAL = 4096;
int combined_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k, float* distances,
                    int64_t* labels, int kind = 0);

// host-pointer wrapper shared by ivfpq / flat
// sync = false: everything is only enqueued (pinned host buffers); the caller synchronises the stream
// lk != nullptr: the caller's SearchLock; its mu is released once everything is enqueued, so writers go on while
// this call waits for the GPU (search_mu stays: the workspaces are in use)
// a deferred tie replay (gamma_hip_set_deferred_replay) is complete on the search stream
inline int replay_join(H* h) {
    if (h->replay_pending) {
        GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_rdone, 0));
        h->replay_pending = false;
    }
    return GAMMA_HIP_OK;
}

template <typename F>
int host_search(H* h, int nq, int d, const float* x, int k, float* distances, int64_t* labels, F&& f,
                bool sync = true, SearchLock* lk = nullptr, float* mapped_d = nullptr, int64_t* mapped_i = nullptr) {
    if (nq <= 0 || k <= 0) return f(nullptr, nullptr, nullptr);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(replay_join(h));
    GH_CHECK(h, h->w_x.ensure((size_t)nq * d * sizeof(float)));
    GH_CHECK(h, h->w_outd.ensure((size_t)nq * k * sizeof(float)));
    GH_CHECK(h, h->w_outl.ensure((size_t)nq * k * sizeof(int64_t)));
    // Small synchronous calls (a client thread's single query): the caller's buffers are pageable, and a pageable
    // copy is a blocking staged transfer -- three of them cost more than the search chain.  Queries and results go
    // through a pinned staging area instead: the copies are true asynchronous transfers in stream order, the thread
    // blocks once, and the results are copied out by the CPU.
    const size_t bx = (size_t)nq * d * sizeof(float), bd = (size_t)nq * k * sizeof(float), bi = (size_t)nq * k * sizeof(int64_t);
    const size_t off_i = (bx + 63) & ~(size_t)63, off_d = off_i + ((bi + 63) & ~(size_t)63), need = off_d + bd;
    static const bool no_pin = getenv("GAMMA_HIP_NO_PINNED_CALLS") != nullptr;
    if (sync && !no_pin && need <= ((size_t)1 << 20)) {
        if (need > h->dir_pin_bytes) {
            if (h->dir_pin) (void)hipHostFree(h->dir_pin);
            h->dir_pin = nullptr;
            h->dir_pin_bytes = 0;
            GH_CHECK(h, hipHostMalloc(&h->dir_pin, std::max<size_t>(need * 2, 65536), hipHostMallocDefault));
            h->dir_pin_bytes = std::max<size_t>(need * 2, 65536);
            h->dir_pin_dev = nullptr;
            if (hipHostGetDevicePointer(&h->dir_pin_dev, h->dir_pin, 0) != hipSuccess) h->dir_pin_dev = nullptr;
        }
        char* base = static_cast<char*>(h->dir_pin);
        std::memcpy(base, x, bx);
        GH_CHECK(h, hipMemcpyAsync(h->w_x.p, base, bx, hipMemcpyHostToDevice, h->stream));
        // results: the last kernel of the chain stores them straight into the staging area (pinned host memory is
        // mapped into the device's address space; a few KB of posted writes) -- no copy back at all
        static const bool no_map = getenv("GAMMA_HIP_NO_MAPPED_RESULTS") != nullptr;
        if (!no_map && h->dir_pin_dev) {
            char* db = static_cast<char*>(h->dir_pin_dev);
            GH_TRY(f(h->w_x.as<float>(), reinterpret_cast<float*>(db + off_d), reinterpret_cast<int64_t*>(db + off_i)));
        } else {
            GH_TRY(f(h->w_x.as<float>(), h->w_outd.as<float>(), h->w_outl.as<int64_t>()));
            GH_CHECK(h, hipMemcpyAsync(base + off_d, h->w_outd.p, bd, hipMemcpyDeviceToHost, h->stream));
            GH_CHECK(h, hipMemcpyAsync(base + off_i, h->w_outl.p, bi, hipMemcpyDeviceToHost, h->stream));
        }
        if (lk) lk->enqueued();
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        std::memcpy(distances, base + off_d, bd);
        std::memcpy(labels, base + off_i, bi);
        return GAMMA_HIP_OK;
    }
    GH_CHECK(h, hipMemcpyAsync(h->w_x.p, x, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (mapped_d && mapped_i) {   // distances / labels are pinned and mapped (the combining queue's staging set): stored in place
        GH_TRY(f(h->w_x.as<float>(), mapped_d, mapped_i));
        if (lk) lk->enqueued();
        if (sync) GH_CHECK(h, hipStreamSynchronize(h->stream));
        return GAMMA_HIP_OK;
    }
    GH_TRY(f(h->w_x.as<float>(), h->w_outd.as<float>(), h->w_outl.as<int64_t>()));
    GH_CHECK(h, hipMemcpyAsync(distances, h->w_outd.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipMemcpyAsync(labels, h->w_outl.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (lk) lk->enqueued();
    if (sync) GH_CHECK(h, hipStreamSynchronize(h->stream));
    return GAMMA_HIP_OK;
}
}  // namespace ghi
