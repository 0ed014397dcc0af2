// gamma_hip_search_flat.cpp -- the flat (brute force) search of libgamma_hip.so over the raw store's rows: the small path,
// the chunked paths (running bound with the matrix-pipe filter, row chunks + merge), their exact-ties phase with the two
// buffer banks of overlapping callers, and the entry points of the C ABI (include/gamma_hip.h).  The exact scanners'
// helper (flat_tie_args) and the filters are gamma_hip_search.cpp's (gamma_hip_search.h).
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

namespace ghi {
namespace {

// ---- flat ------------------------------------------------------------------------------
// w_flat_meta of one query chunk of the running bound: tau[nc] | cnt[nc * CS] | overflow -- the counters one 128-byte line
// apart: ~140 appends per query and pass are returning atomics, and 32 queries' counters on one line serialised 4500 of them
// (C2 exact passes 49 / 66 / 84 -> 30 / 31 / 37 us)
struct FlatMeta {
    static constexpr int CS = 32;   // ints from one query's counter to the next (gh::FlatEmit's stride)
    int* base;
    int nc;
    static size_t bytes(int nc) { return (size_t)(nc + (size_t)nc * CS + 1) * sizeof(int); }
    uint32_t* tau() const { return reinterpret_cast<uint32_t*>(base); }
    int* cnt() const { return base + nc; }
    int* over() const { return cnt() + (size_t)nc * CS; }   // set when a candidate list overflowed
};

// One flat search call: what its phases read, fixed at construction (pure arithmetic: nothing is enqueued there).
struct FlatCall {
    H* const h;
    const gamma_hip_search_params* const p;   // the call's own copy (exact_ties resolved)
    const gh::FilterDesc& filt;
    const gh::RowsRef rows;   // the store's rows as every reader below takes them: pointer + element type (fp32 rows: the launches they always were)
    const int nq;
    const float* const d_x;
    float* const d_distances;
    int64_t* const d_labels;
    const int d;
    const int64_t N;
    const bool l2;
    const float neutral, sentinel;
    const hipStream_t s;
    // the plan of the chunked paths: query chunks x row chunks so the distance slab stays inside the budget
    const bool mfma_filter;   // the call's shape has a variant of the matrix-pipe filter (a query chunk's: uses_filter)
    const int64_t rows_chunk;
    const int qc, nchunks;
    // exact ties: the chunked paths order results on (distance, row id); the reference's heap (heap_pop + heap_push in
    // vid order, heap_reorder: gamma_index_flat.cc:118-300) orders equal distances its own way and decides which members
    // of a tie at the cut stay.  Run for k + 1 results, list the queries with two equal distances among them and replay
    // those through the heap over a freshly computed distance row (k_tie_replay).
    const bool ties;
    const int k_out;    // the caller's k: the width of its buffers
    const int k_work;   // the width the chunked paths select: k_out + 1 with ties
    // Overlapping callers (gamma_hip_flat_search_device_wait): this call's tie replay goes to the side stream when the call is one
    // query chunk; a call that finds a FLAT replay pending does not wait for it -- it works in the other bank of the buffers the
    // replay reads and waits, in stream order, only for the replay that last read that bank.
    const bool defer;
    const int cap;       // items of a query's candidate list (running bound)
    const int log_nsl;   // slices of the log: one per pass of the running bound (+ slice 0, the first chunk's slab)

    // pass sizes: every pass scores (growth - 1) x the rows scored so far -- with a bound from r rows a pass over g r more
    // lets ~k ln(1 + g) new candidates per query through; fewer, larger passes pay fewer fixed launches (bounds, filter
    // ramp, exact, compact: ~100 us each at C2)
    // (C2, ms per call at growth 2 / 3 / 4 / 6: 2.26 / 2.19 / 2.15 / 2.24)
    static constexpr int flat_growth = 4;

    FlatCall(H* h_, const gamma_hip_search_params* p_, const gh::FilterDesc& filt_, int nq_, const float* d_x_, int k,
             float* d_distances_, int64_t* d_labels_)
        : h(h_), p(p_), filt(filt_), rows(raw_rows_ref(h_)), nq(nq_), d_x(d_x_), d_distances(d_distances_), d_labels(d_labels_),
          d(h_->raw_d), N(h_->nraw), l2(p_->metric == GAMMA_HIP_METRIC_L2), neutral(neutral_of(l2)),
          sentinel(l2 ? INFINITY : -INFINITY), s(h_->stream),
          // (decided on the caller's k; the running bound itself is gated on the working width: bound_applies)
          mfma_filter(k <= 256 && N < ((int64_t)1 << 32) && gh::flat_filter_supported(nq, d, N)),
          rows_chunk((std::max<int64_t>(256, std::min<int64_t>(N, (int64_t)1 << first_chunk_log2(mfma_filter, d))) + 255) / 256 * 256),
          qc((int)std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(h->dist_budget_bytes / (rows_chunk * sizeof(float)))))),
          nchunks((int)std::max<int64_t>(1, (N + rows_chunk - 1) / rows_chunk)),
          ties(tie_on(p) && N > 0), k_out(k), k_work(ties ? k + 1 : k),
          defer(h->defer_now && h->side2 != nullptr && ties && qc >= nq), cap(gh::flat_list_cap()), log_nsl(count_log_slices()) {}

    // The matrix-pipe filter (flat_mfma.hip: bf16 hi / lo products with a proven margin, exact distances of the ~k survivors
    // per query and pass) takes the passes behind the first row chunk when the shape has a variant; the first chunk -- scored
    // exactly for every query, the only part still on the vector ALU -- is then 16384 rows instead of 65536.
    // (long rows: the first chunk's exact kernel runs at ~1.3 TFLOP/s -- 1024 rows of d = 768 instead of 16384: C5 flat, 1 M x 768,
    //  1024 queries: 15.6 / 16.1 / 16.8 / 18.4 ms per call with a first chunk of 2^10 / 2^11 / 2^12 / 2^13 rows)
    // (the lengths of k_flat_filter_any, d <= 128: no k_pairwise_lds variant scores the first chunk -- it runs on the generic
    //  kernel at the long rows' rate, so it is 2^12 rows, the smallest the filter's gate ny >= 4096 leaves room behind)
    static int first_chunk_log2(bool mfma_filter, int d) {
        static const int fl_any = [] {   // (measurements of the any-length shapes only: DESIGN section 19)
            const char* e = getenv("GAMMA_HIP_FLAT_ANYD_FIRST_LOG2");
            const int v = e ? atoi(e) : 0;
            return v >= 8 && v <= 16 ? v : 0;
        }();
        const bool new_shape = gh::flat_filter_new_shape(d);
        return mfma_filter ? (new_shape && fl_any ? fl_any : (d > 128 ? 10 : (new_shape ? 12 : 14))) : 16;
    }
    int64_t pass_rows(int64_t r) const { return std::min<int64_t>((int64_t)(flat_growth - 1) * r, N - r); }
    int count_log_slices() const {
        int n = 1;
        for (int64_t r = rows_chunk; r < N; r += pass_rows(r)) n++;
        return n;
    }
    int64_t whole_row_stride() const { return (N + 3) & ~(int64_t)3; }   // a slab row that holds the whole store
    const float* queries(int q0) const { return d_x + (size_t)q0 * d; }
    // where the chunked paths write their [nc][k_work] result of query chunk q0 (with ties: for the tie phase to take)
    float* outD(int q0) const { return ties ? h->w_fD.as<float>() : d_distances + (size_t)q0 * k_out; }
    int64_t* outI(int q0) const { return ties ? h->w_fI.as<int64_t>() : d_labels + (size_t)q0 * k_out; }
    FlatMeta meta(int nc) const { return FlatMeta{h->w_flat_meta.as<int>(), nc}; }
    // the passes of this query chunk's running bound go through the matrix-pipe filter
    bool uses_filter(int nc) const { return mfma_filter && gh::flat_filter_supported(nc, d, N); }
    bool bound_applies(int nc, bool mf) const {
        return !h->flat_no_bound && k_work <= 256 && N > rows_chunk && N < ((int64_t)1 << 32) &&
               (gh::pairwise_can_emit(nc, d, N - rows_chunk) || mf);
    }

    bool small_ok() const;
    int small_path();
    int join_or_switch_bank();
    int ensure_workspaces();
    int empty_result(int q0, int nc);
    int unbounded(int q0, int nc);
    int bounded(int q0, int nc, bool mf);
    int overflowed(int nc, bool* yes);
    int defer_overflow_word(int nc, bool mf);
    int tie_phase(int q0, int nc, bool redo);
    int tie_recompute(int q0, const gh::TieReplayArgs& tr);
    int replay(const gh::TieReplayArgs& tr);
};

// small calls: the whole store as ONE row chunk, then the small-batch chains' selection -- three or four launches
// instead of three per 65536 rows (1 M x 128, one query: 49 launches, 1.1 ms)
bool FlatCall::small_ok() const {
    static const bool off = getenv("GAMMA_HIP_NO_SMALL_PATH") != nullptr;
    return !off && h->small_path && nq <= 64 && k_out <= 1024 && N >= 1 && N <= ((int64_t)1 << 22) && !h->profile &&
           (size_t)nq * whole_row_stride() * sizeof(float) <= std::min<size_t>(h->dist_budget_bytes, (size_t)1 << 30);
}

int FlatCall::small_path() {
    const int64_t stride = whole_row_stride();
    GH_TRY(replay_join(h));
    GH_CHECK(h, h->w_dist.ensure((size_t)nq * stride * sizeof(float)));
    GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq * k_out * sizeof(int)));
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq * k_out * sizeof(float)));
    GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq * k_out * sizeof(int64_t)));
    StageScope t(h, GAMMA_HIP_STAGE_FLAT);
    gh::launch_pairwise_filtered(s, l2, d_x, nq, d, rows, N, h->w_dist.as<float>(), stride, filt, p->min_score,
                                 p->max_score, 0);
    int smax = h->small_presel > 0 ? h->small_presel : (N > 16384 ? (int)std::min<int64_t>(64, (N + 16383) / 16384) : 0);
    if (smax > 0) {
        GH_CHECK(h, h->w_selv.ensure((size_t)nq * smax * k_out * sizeof(float)));
        GH_CHECK(h, h->w_selp.ensure(((size_t)nq * smax * k_out + (size_t)nq * smax) * sizeof(int)));   // + a cut flag per slice
    }
    // exact ties: a query with equal distances at the k cut or among its k results is replayed through the
    // reference's heap over the whole row (gamma_index_flat.cc:118-300: heap_pop + heap_push in vid order)
    gh::TieReplayArgs tr;
    const bool small_ties = tie_on(p) && k_out <= gh::tie_small_max_k();   // (this path's gate: k <= 1024)
    if (small_ties) {
        flat_tie_args(h, &tr, l2, nq, stride, 0, k_out, d_x, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), d_distances,
                      d_labels, (int)N);
        tr.d = d;
    }
    // (has_rank = 0: the tail selects from the slab and reads no row -- its fp32 row pointer is null for a narrow store)
    gh::launch_small_tail(s, l2, h->w_dist.as<float>(), stride, nullptr, nq, k_out, 0, nullptr, nullptr, nullptr, nullptr,
                          h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>(), h->w_cand_ids.as<int64_t>(), 0, d_x, d,
                          h->raw_f32(), N, k_out, p->min_score, p->max_score, neutral, d_distances, d_labels, smax,
                          smax ? h->w_selv.as<float>() : nullptr, smax ? h->w_selp.as<int>() : nullptr, (int)N,
                          small_ties ? &tr : nullptr, h->d_tie_stats);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

// a replay of an earlier call may still be running on the side stream: join it, or (see `defer`) leave it alone and work in
// the other bank of the buffers it reads
int FlatCall::join_or_switch_bank() {
    if (!h->replay_pending) return GAMMA_HIP_OK;
    if (!(defer && h->replay_is_flat)) return replay_join(h);
    DevBuf* cur[5] = {&h->w_dist, &h->w_flog, &h->w_tlist, &h->w_cand_dis, &h->w_cand_ids};
    for (int i = 0; i < 5; i++) std::swap(*cur[i], h->fbank[i]);
    h->flat_bank ^= 1;
    if (h->bank_used[h->flat_bank]) GH_CHECK(h, hipStreamWaitEvent(s, h->ev_bank[h->flat_bank], 0));
    // (replay_pending stays: whoever comes next and cannot switch banks joins)
    return GAMMA_HIP_OK;
}

// the tie replay of a query chunk: on the call's stream, or (`defer`) on the side stream, marking the bank it reads
int FlatCall::replay(const gh::TieReplayArgs& tr) {
    if (!defer) {
        gh::launch_tie_replay(s, l2, tr);
        return GAMMA_HIP_OK;
    }
    const int b = h->flat_bank;
    if (!h->ev_bank[b]) GH_CHECK(h, hipEventCreateWithFlags(&h->ev_bank[b], hipEventDisableTiming));
    GH_CHECK(h, hipEventRecord(h->ev_rfork, s));
    GH_CHECK(h, hipStreamWaitEvent(h->side2, h->ev_rfork, 0));
    gh::launch_tie_replay(h->side2, l2, tr);
    GH_CHECK(h, hipEventRecord(h->ev_rdone, h->side2));
    GH_CHECK(h, hipEventRecord(h->ev_bank[b], h->side2));
    h->bank_used[b] = true;
    h->replay_pending = true;
    h->replay_is_flat = true;
    return GAMMA_HIP_OK;
}

int FlatCall::ensure_workspaces() {
    GH_CHECK(h, h->w_dist.ensure((size_t)qc * rows_chunk * sizeof(float)));
    GH_CHECK(h, h->w_part_v.ensure((size_t)qc * nchunks * k_work * sizeof(float)));
    GH_CHECK(h, h->w_part_i.ensure((size_t)qc * nchunks * k_work * sizeof(int64_t)));
    GH_CHECK(h, h->w_selv.ensure((size_t)qc * k_work * sizeof(float)));
    GH_CHECK(h, h->w_selp.ensure((size_t)qc * k_work * sizeof(int)));
    GH_CHECK(h, h->w_cand_pos.ensure((size_t)qc * k_work * sizeof(int)));
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)qc * k_work * sizeof(float)));
    if (ties) {
        GH_CHECK(h, h->w_fD.ensure((size_t)qc * k_work * sizeof(float)));
        GH_CHECK(h, h->w_fI.ensure((size_t)qc * k_work * sizeof(int64_t)));
        GH_CHECK(h, h->w_tlist.ensure(((size_t)qc + 1) * sizeof(int)));
        GH_CHECK(h, h->w_cand_ids.ensure((size_t)qc * k_work * sizeof(int64_t)));
    }
    return GAMMA_HIP_OK;
}

// nothing to scan: all-empty result
int FlatCall::empty_result(int q0, int nc) {
    GH_CHECK(h, hipMemsetAsync(h->w_selp.p, 0xff, (size_t)nc * k_work * sizeof(int), s));
    gh::launch_finalize_topk(s, h->w_selv.as<float>(), h->w_selp.as<int>(), nc, k_work, nullptr, 0, 0,
                             neutral, outD(q0), outI(q0));
    return GAMMA_HIP_OK;
}

// the reference's loop: every row, one query at a time, a k-heap (gamma_index_flat.cc:118-300).
// Here: distance slab of one row chunk -> per-chunk top-k -> merge of the chunks' tables.
int FlatCall::unbounded(int q0, int nc) {
    const float* xq = queries(q0);
    for (int c = 0; c < nchunks; c++) {
        const int64_t r0 = (int64_t)c * rows_chunk;
        const int64_t nr = std::min<int64_t>(rows_chunk, N - r0);
        gh::launch_pairwise_filtered(s, l2, xq, nc, d, rows.at(r0, d), nr, h->w_dist.as<float>(),
                                     rows_chunk, filt, p->min_score, p->max_score, r0);
        // per-chunk top-k: values + positions relative to the chunk
        gh::launch_select_topk(s, l2, h->w_dist.as<float>(), rows_chunk, nullptr, (int)nr, (int)nr, nc, k_work,
                               h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>());
        // scatter into the partial table [q][chunk][k] with global ids
        // (reuse finalize_topk: labels = pos, then offset by r0 on the fly below)
        gh::launch_finalize_topk(s, h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>(), nc, k_work, nullptr,
                                 0, r0, sentinel, h->w_selv.as<float>(),
                                 h->w_part_i.as<int64_t>() + (size_t)c * nc * k_work);
        GH_CHECK(h, hipMemcpyAsync(h->w_part_v.as<float>() + (size_t)c * nc * k_work, h->w_selv.p,
                                   (size_t)nc * k_work * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // merge: layout [chunk][q][k] == the sharded layout [shard][nq][R]
    GH_CHECK(h, h->w_m_dis.ensure((size_t)nc * nchunks * k_work * sizeof(float)));
    GH_CHECK(h, h->w_m_ids.ensure((size_t)nc * nchunks * k_work * sizeof(int64_t)));
    gh::launch_gather_shards(s, h->w_part_v.as<float>(), h->w_part_i.as<int64_t>(), nchunks, nc, k_work,
                             h->w_m_dis.as<float>(), h->w_m_ids.as<int64_t>(), sentinel);
    gh::launch_select_topk(s, l2, h->w_m_dis.as<float>(), (int64_t)nchunks * k_work, nullptr, nchunks * k_work,
                           nchunks * k_work, nc, k_work, h->w_selv.as<float>(), h->w_selp.as<int>());
    gh::launch_finalize_topk(s, h->w_selv.as<float>(), h->w_selp.as<int>(), nc, k_work,
                             h->w_m_ids.as<int64_t>(), (int64_t)nchunks * k_work, 0, neutral,
                             outD(q0), outI(q0));
    return GAMMA_HIP_OK;
}

// Running bound: only the first chunk goes through a distance slab.  Its k-th best bounds the
// answer; the remaining rows are scored in passes that double the rows seen so far, each pass
// appending only the distances within the current bound to the query's candidate list (about k
// per pass and query) and ending with a compaction that tightens the bound.  The k smallest
// (distance, row id) items are the same either way.  A list that overflows (rows arriving in
// improving order) is detected and the call redone without a bound.
// mf: uses_filter(nc)
int FlatCall::bounded(int q0, int nc, bool mf) {
    const float* xq = queries(q0);
    GH_CHECK(h, h->w_flat_cand.ensure((size_t)nc * cap * sizeof(unsigned long long)));
    GH_CHECK(h, h->w_flat_meta.ensure(FlatMeta::bytes(nc)));
    const FlatMeta m = meta(nc);
    uint32_t* tau = m.tau();
    int* over = m.over();
    gh::FlatEmit em{tau, h->w_flat_cand.as<unsigned long long>(), m.cnt(), cap, FlatMeta::CS};
    GH_CHECK(h, hipMemsetAsync(over, 0, sizeof(int), s));
    gh::FlatLog lg;
    if (ties) {   // what every pass appends is kept for the replay (slice `pass` of the query)
        GH_CHECK(h, h->w_flog.ensure((size_t)nc * log_nsl * cap * sizeof(unsigned long long) +
                                     (size_t)nc * (log_nsl + 1) * sizeof(int)));
        lg.items = h->w_flog.as<unsigned long long>();
        lg.cnt = reinterpret_cast<int*>(lg.items + (size_t)nc * log_nsl * cap);
        lg.kept = lg.cnt + (size_t)nc * log_nsl;
        lg.nsl = log_nsl;
        GH_CHECK(h, hipMemsetAsync(lg.cnt, 0, (size_t)nc * log_nsl * sizeof(int), s));
    }
    gh::launch_pairwise_filtered(s, l2, xq, nc, d, rows, rows_chunk, h->w_dist.as<float>(), rows_chunk, filt,
                                 p->min_score, p->max_score, 0);
    gh::launch_select_topk(s, l2, h->w_dist.as<float>(), rows_chunk, nullptr, (int)rows_chunk, (int)rows_chunk,
                           nc, k_work, h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>());
    gh::launch_flat_init(s, l2, h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>(), nc, k_work, 0, em, tau, lg.kept);
    const int64_t pcap = gh::flat_filter_pair_cap(nc);
    float* bnd = nullptr;
    int* npairs = nullptr;
    if (mf) {   // once per query chunk: norms and the queries' bf16 hi / lo image
        GH_CHECK(h, h->w_xn.ensure((size_t)nc * sizeof(float)));
        GH_CHECK(h, h->w_fq.ensure(gh::flat_filter_query_image_bytes(nc, d)));
        GH_CHECK(h, h->w_fraw.ensure((size_t)pcap * 8));
        GH_CHECK(h, h->w_frcnt.ensure(gh::flat_filter_counter_bytes() + gh::flat_filter_bounds_bytes(nc)));   // pair counters | bounds
        npairs = h->w_frcnt.as<int>();
        bnd = reinterpret_cast<float*>(h->w_frcnt.as<char>() + gh::flat_filter_counter_bytes());
        gh::launch_row_norms(s, xq, nc, d, h->w_xn.as<float>());
        gh::launch_flat_prep_queries(s, xq, nc, d, h->w_fq.p);
    }
    for (int64_t r = rows_chunk; r < N;) {
        const int64_t nr = pass_rows(r);
        if (mf) {
            GH_CHECK(h, hipMemsetAsync(npairs, 0, (size_t)gh::flat_filter_counter_bytes(), s));
            gh::launch_flat_filter(s, l2, d, h->w_fq.p, h->w_xn.as<float>(), tau, bnd, nc, rows.at(r, d), nr, r,
                                   h->w_fraw.p, npairs, pcap);
            gh::launch_flat_exact(s, l2, h->w_fraw.p, npairs, pcap, xq, nc, d, rows, filt, p->min_score, p->max_score,
                                  em, over);
            h->ff_passes.fetch_add(1, std::memory_order_relaxed);
            h->ff_pairs.fetch_add((int64_t)nc * nr, std::memory_order_relaxed);
        } else {
            gh::launch_pairwise_emit(s, l2, xq, nc, d, rows.at(r, d), nr, filt, p->min_score, p->max_score, r, em);
        }
        lg.pass++;
        gh::launch_flat_compact(s, nc, k_work, em, tau, over, ties ? &lg : nullptr);
        r += nr;
    }
    gh::launch_flat_final(s, l2, nc, k_work, em, neutral, outD(q0), outI(q0));
    GH_CHECK(h, hipGetLastError());
    // (whether a list overflowed -- then the call is redone without a bound -- is read back by the caller AFTER it has
    //  enqueued the tie phase: the device never waits for the host)
    return GAMMA_HIP_OK;
}

// the synchronous read-back of the chunk's overflow word
int FlatCall::overflowed(int nc, bool* yes) {
    int h_over = 0;
    GH_CHECK(h, hipMemcpyAsync(&h_over, meta(nc).over(), sizeof(int), hipMemcpyDeviceToHost, s));
    GH_CHECK(h, hipStreamSynchronize(s));
    *yes = h_over != 0;
    return GAMMA_HIP_OK;
}

// overlapping callers: the word goes to the caller's pinned slot instead
// (the caller reads the word after the call's completion event, with the handle free: no host wait under the lock)
int FlatCall::defer_overflow_word(int nc, bool mf) {
    h->flat_over_passes = mf ? log_nsl - 1 : 0;   // (counted by the caller if the word says so)
    GH_CHECK(h, hipMemcpyAsync(h->flat_over_dst, meta(nc).over(), sizeof(int), hipMemcpyDeviceToHost, s));
    return GAMMA_HIP_OK;
}

// exact ties: the chunk's [nc][k_work] result goes to the caller's buffers, the queries with two equal distances among the
// k_work are listed and replayed.  redo: the chunk ran without a bound
int FlatCall::tie_phase(int q0, int nc, bool redo) {
    int* count = h->w_tlist.as<int>();
    int* list = count + 1;
    GH_CHECK(h, hipMemsetAsync(count, 0, sizeof(int), s));
    gh::launch_flat_take_flag(s, h->w_fD.as<float>(), h->w_fI.as<int64_t>(), nc, k_out, d_distances + (size_t)q0 * k_out,
                              d_labels + (size_t)q0 * k_out, list, count, h->d_tie_stats);
    gh::TieReplayArgs tr;
    flat_tie_args(h, &tr, l2, nc, rows_chunk, 0, k_out, queries(q0), h->w_cand_dis.as<float>(),
                  h->w_cand_ids.as<int64_t>(), d_distances + (size_t)q0 * k_out, d_labels + (size_t)q0 * k_out, (int)N);
    tr.d = d;
    tr.list = list;
    tr.count = count;
    if (redo && nchunks == 1) return replay(tr);   // the one slab holds every row
    if (redo) return tie_recompute(q0, tr);
    // the running bound: the stream the heap saw = the first row chunk (its slab is intact) + what every
    // later pass appended to the query's list, in row order
    tr.G = (int)rows_chunk;
    tr.always_sliced = 1;
    tr.surv = h->w_flog.as<unsigned long long>();
    tr.gcnt = reinterpret_cast<const int*>(tr.surv + (size_t)nc * log_nsl * cap);
    tr.nsl = log_nsl;
    tr.slice_cap = cap;
    return replay(tr);
}

// several row chunks through one slab: the rows of the flagged queries are computed again
int FlatCall::tie_recompute(int q0, const gh::TieReplayArgs& tr) {
    GH_TRY(replay_join(h));
    int nflag = 0;
    GH_CHECK(h, hipMemcpyAsync(&nflag, tr.count, sizeof(int), hipMemcpyDeviceToHost, s));
    GH_CHECK(h, hipStreamSynchronize(s));
    const int64_t stride = whole_row_stride();
    const int fcap = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (int64_t)(h->dist_budget_bytes / ((size_t)stride * sizeof(float)))));
    for (int f0 = 0; f0 < nflag; f0 += fcap) {
        const int nf = std::min(fcap, nflag - f0);
        GH_CHECK(h, h->w_fx.ensure((size_t)nf * d * sizeof(float)));
        GH_CHECK(h, h->w_fslab.ensure((size_t)nf * stride * sizeof(float)));
        gh::launch_gather_rows(s, queries(q0), tr.list + f0, nf, d, h->w_fx.as<float>());
        gh::launch_pairwise_filtered(s, l2, h->w_fx.as<float>(), nf, d, rows, N, h->w_fslab.as<float>(), stride, filt,
                                     p->min_score, p->max_score, 0);
        gh::TieReplayArgs t2 = tr;
        t2.nq = nf;
        t2.slab = h->w_fslab.as<float>();
        t2.q_stride = stride;
        t2.list = tr.list + f0;
        t2.compact_rows = 1;
        gh::launch_tie_replay(s, l2, t2);
    }
    return GAMMA_HIP_OK;
}

}  // namespace

int flat_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int k,
                              float* d_distances, int64_t* d_labels) {
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    // (a narrow store is served only after gamma_hip_set_flat_narrow_rows, an sq8 store only after gamma_hip_set_flat_sq8_rows,
    //  whatever the other switch says: the refusal is what every caller had before)
    if (!raw_store_served(h, h->flat_narrow_rows, h->flat_sq8_rows)) return raw_store_refuse(h, "flat search");
    GH_TRY(check_params(h, p, nq, k));
    gamma_hip_search_params pp;   // (the chunked paths run for k + 1 results: k = 4096, the ABI's largest, is beyond the mode)
    GH_TRY(resolve_ties(h, p, &pp, k + 1 <= gh::tie_replay_max_k() && h->nraw < ((int64_t)1 << 31),
                        "exact_ties = 1 with k = 4096 or 2^31 rows (flat search)"));
    if (!h->has_raw_rows() && h->nraw > 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, &pp, &filt, nullptr, (int64_t)nq * h->nraw));
    FlatCall c(h, &pp, filt, nq, d_x, k, d_distances, d_labels);
    if (c.small_ok()) return c.small_path();
    GH_TRY(c.join_or_switch_bank());
    GH_TRY(c.ensure_workspaces());
    StageScope t(h, GAMMA_HIP_STAGE_FLAT);
    for (int q0 = 0; q0 < nq; q0 += c.qc) {
        const int nc = std::min(c.qc, nq - q0);
        if (c.N == 0) {
            GH_TRY(c.empty_result(q0, nc));
            continue;
        }
        const bool mf = c.uses_filter(nc);   // once per query chunk: the launch choice and both counters
        if (c.bound_applies(nc, mf)) {
            GH_TRY(c.bounded(q0, nc, mf));
            if (c.ties) GH_TRY(c.tie_phase(q0, nc, false));   // enqueued before the host learns whether a list overflowed
            if (c.defer && h->flat_over_dst) {
                GH_TRY(c.defer_overflow_word(nc, mf));
                continue;
            }
            bool redo = false;
            GH_TRY(c.overflowed(nc, &redo));
            if (!redo) continue;
            if (mf) h->ff_redone.fetch_add(c.log_nsl - 1, std::memory_order_relaxed);
            GH_TRY(replay_join(h));   // (a replay on the side stream writes the rows that are about to be redone)
        }
        GH_TRY(c.unbounded(q0, nc));
        if (c.ties) GH_TRY(c.tie_phase(q0, nc, true));
    }
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int flat_search_host_locked(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                                  float* distances, int64_t* labels) {
    SearchLock lk(h);
    GH_TRY(check_params(h, p, nq, k));
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    if (nq > 0 && k > 0 && (!x || !distances || !labels)) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    return host_search(h, nq, h->raw_d, x, k, distances, labels, [&](const float* dx, float* dd, int64_t* dl) {
        return flat_search_device_locked(h, p, nq, dx, k, dd, dl);
    }, true, &lk);
}

}  // namespace ghi

using namespace ghi;

extern "C" {

int gamma_hip_flat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                 const float* d_x, int k, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    return flat_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
}

// the slot's event behind everything of the call that was just enqueued
// (the main stream carries the copy of the overflow word; the side stream, if a replay is pending, the last writes)
static int arm_behind_call(H* h, CallSlot* slot) {
    if (h->replay_pending) {
        GH_CHECK(h, hipEventRecord(h->ev_rfork, h->stream));
        GH_CHECK(h, hipStreamWaitEvent(h->side2, h->ev_rfork, 0));
    }
    GH_CHECK(h, CallSlots::arm(slot, h->replay_pending ? h->side2 : h->stream));
    return GAMMA_HIP_OK;
}

int gamma_hip_flat_search_device_wait(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                      const float* d_x, int k, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    CallTicket t(h->call_slots);   // this call's event and overflow word: its own until it has read the word (call_slots.h)
    int over_passes = 0;   // filter passes of this call: redone if its overflow word is set
    {
        SearchLock lk(h);
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, t.take());
        h->defer_now = h->side2 != nullptr;
        h->flat_over_dst = t.slot()->over;
        h->flat_over_passes = 0;
        int rc = flat_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
        over_passes = h->flat_over_passes;
        h->defer_now = false;
        h->flat_over_dst = nullptr;
        if (rc == GAMMA_HIP_OK) rc = arm_behind_call(h, t.slot());
        if (rc != GAMMA_HIP_OK) {
            // (the copy into the slot's word may be on its way already: the slot goes back to the pool only behind it)
            (void)hipStreamSynchronize(h->stream);
            return rc;
        }
    }
    if (CallSlots::wait(t.slot()) != hipSuccess) return GAMMA_HIP_EDEVICE;
    const int over = CallSlots::word(t.slot());
    t.done();   // (the slot goes to the next call before the redo, if there is one)
    if (over) {   // a survivor list overflowed (adversarial data): the call again without a bound, the plain way
        SearchLock lk(h);
        h->ff_redone.fetch_add(over_passes, std::memory_order_relaxed);
        h->flat_no_bound = true;
        int rc = replay_join(h);
        if (rc == GAMMA_HIP_OK) rc = flat_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
        h->flat_no_bound = false;
        if (rc != GAMMA_HIP_OK) return rc;
        GH_CHECK(h, hipStreamSynchronize(h->stream));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_flat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x,
                          int k, float* distances, int64_t* labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    // small unfiltered calls from concurrent client threads share device batches (see gamma_hip_ivfpq_search)
    // (a narrow store is never combined, whatever gamma_hip_set_flat_narrow_rows says)
    if (h->combine && p && nq > 0 && nq <= COMB_MAX_NQ && k > 0 && x && distances && labels && h->raw_d > 0 && !h->raw_narrow() &&
        !p->has_range && p->n_range == 0 && p->n_field == 0 && p->n_term == 0)
        return combined_search(h, p, nq, x, k, distances, labels, /*kind=*/1);
    return flat_search_host_locked(h, p, nq, x, k, distances, labels);
}

}  // extern "C"
