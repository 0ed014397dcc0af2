// gamma_hip_search_shard.cpp -- the IVFPQ search over list shards, entry points of the C ABI (include/gamma_hip.h): a
// shard's stage A (own coarse quantizer, preassigned, bounded with the reduction of the shards' bounds), the merge of the
// shards' candidate tables with the re-rank, the exact distances and candidate streams a shard exports, and the tie replay
// of a merged slice (with gamma_hip_gather_rows, the gather its callers assemble the flagged queries' rows with).  The
// stages themselves are gamma_hip_search.cpp's (gamma_hip_search.h).
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

using namespace ghi;

extern "C" {

int gamma_hip_ivfpq_search_shard(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                 const float* d_x, int k, float* d_recall_dis, int64_t* d_recall_ids) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_search_shard");
    GH_TRY(replay_join(h));
    GH_TRY(ivfpq_check(h, p, nq, k));
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    if (!d_x || !d_recall_dis || !d_recall_ids) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    GH_CHECK(h, hipSetDevice(h->device));
    const int R = std::max(p->recall_num, k);
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    if (pp.coarse_mode < 0) pp.coarse_mode = nq < 20 ? 0 : 1;   // decided on the whole call, not per chunk
    if (pp.coarse_mode == 1 && blas_form_not_restated(nq, h->nlist, h->d)) h->blas_unrestated++;
    p = &pp;
    const int chunk = query_chunk(h, nq, p->nprobe);
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nc = std::min(chunk, nq - q0);
        GH_TRY(ivfpq_stage_a(h, p, fc.at(q0), nc, d_x + (size_t)q0 * h->d, R, nullptr, nullptr, /*shard=*/true,
                             d_recall_dis + (size_t)q0 * R, d_recall_ids + (size_t)q0 * R));
        h->last_nq = nc;
    }
    h->last_P = p->nprobe;
    h->last_R = R;
    return GAMMA_HIP_OK;
}

static int shard_preassigned(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                             const float* d_x, const float* d_coarse_dis,
                             const int32_t* d_probe, int k, float* d_recall_dis,
                             int64_t* d_recall_ids, BoundXchg* bx) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    // (a call with a reduction makes it exactly once, whatever happens: the other shards are waiting in theirs)
    struct ReduceOnce {
        H* h; BoundXchg* bx; int nq; bool l2;
        ~ReduceOnce() {
            if (bx && !bx->called && bx->d_bound && nq > 0) {
                gh::launch_fill_f32(h->stream, bx->d_bound, nq, l2 ? INFINITY : -INFINITY);
                (void)bx->reduce(h, nq, l2);
            }
        }
    } reduce_once{h, bx, nq, p && p->metric == GAMMA_HIP_METRIC_L2};
    GH_NO_PQ4(h, "gamma_hip_ivfpq_search_shard_preassigned / _bounded");
    GH_TRY(replay_join(h));
    GH_TRY(ivfpq_check(h, p, nq, k));
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    if (!d_coarse_dis || !d_probe) return fail(h, GAMMA_HIP_EINVAL, "null coarse assignment");
    if (!d_x || !d_recall_dis || !d_recall_ids) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (bx && !bx->d_bound) return fail(h, GAMMA_HIP_EINVAL, "null bound buffer");
    GH_CHECK(h, hipSetDevice(h->device));
    const int R = std::max(p->recall_num, k), P = p->nprobe;
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, P <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    int chunk = query_chunk(h, nq, P);
    struct StrideScope {   // the measured stride holds for this call only
        H* h;
        ~StrideScope() { h->q_stride_cap = 0; }
    } stride_scope{h};
    static const bool no_two = getenv("GAMMA_HIP_NO_TWO_PHASE") != nullptr;
    if (chunk < nq || (bx && !no_two)) {
        // A shard scans ~P / W of a query's probes, but the slab stride of the general path is P x the longest list:
        // the budget then cuts the batch (W times the queries of one rank) into many chunks, each with its own launches
        // and its own handful of fallback queries (full-size C4, W = 8: 20 chunks, 5.7 ms of a 37 ms step).  The
        // assignment is on the device: one small kernel measures the longest candidate row of THIS batch over THIS
        // shard's lists, the host reads the one word back (the call is tens of milliseconds long) and sizes the chunks
        // by it.
        GH_CHECK(h, h->w_shard_cut.ensure(std::max<size_t>((size_t)nq, 16)));   // (its first word; the flags come later)
        gh::launch_max_local_total(h->stream, d_probe, nq, P, h->d_list_len, h->d_list_mask, h->nlist, h->w_shard_cut.as<int>());
        int mx[2] = {0, 0};
        GH_CHECK(h, hipMemcpyAsync(mx, h->w_shard_cut.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        h->q_stride_cap = (std::max<int64_t>(mx[0], 1) + 3) & ~(int64_t)3;
        const int64_t by_dist = (int64_t)(h->dist_budget_bytes / ((size_t)h->q_stride_cap * sizeof(float)));
        chunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_dist, coarse_chunk(h, nq)), nq));
        if (bx && !no_two && chunk < nq && (int64_t)nq <= coarse_chunk(h, nq)) {
            // Two phases need the batch in ONE chunk (one reduction per call).  The slab of a W-rank job's batch -- W x the
            // queries of a rank, each with its longest-case row -- can exceed the general workspace budget (full-size C4, 8
            // shards: ~40 GB against 32); a list shard holds 1 / W of the index, so the memory is there: up to half of what
            // is free now (the workspace stays allocated for the calls that follow).
            size_t free_b = 0, total_b = 0;
            const size_t need = (size_t)nq * (size_t)h->q_stride_cap * sizeof(float);
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= h->w_dist.cap + free_b / 2) chunk = nq;
            else (void)hipGetLastError();
        }
        if (bx && !no_two && chunk >= nq) {
            // two phases (ivfpq_stage_a, BoundXchg): the batch runs as ONE chunk, so the reduction is one collective; the scan
            // behind sees a search of P' probes -- the most owned probes any query of the batch has -- all of them dense
            const char* g1e = getenv("GAMMA_HIP_SHARD_G1");   // (read per call: tools sweep it inside one process)
            const int g1_env = g1e ? atoi(g1e) : 2;
            bx->two_phase = true;
            bx->P_in = P;
            bx->G1 = std::max(1, g1_env);
            const int g = bx->G1;
            pp.nprobe = std::max(1, std::min(P, ((std::max(mx[1], 1) + g - 1) / g) * g));
        }
    }
    const int P_in = P;
    const int Pe = pp.nprobe;   // rows of the compacted assignment the scan sees (P unless two phases)
    bool all_cut = true;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nc = std::min(chunk, nq - q0);
        GH_TRY(ivfpq_stage_a(h, p, fc.at(q0), nc, d_x + (size_t)q0 * h->d, R, d_coarse_dis + (size_t)q0 * P_in,
                             d_probe + (size_t)q0 * P_in, /*shard=*/true, d_recall_dis + (size_t)q0 * R,
                             d_recall_ids + (size_t)q0 * R, (bx && bx->two_phase) ? bx : nullptr));
        h->last_nq = nc;
        if (chunk < nq && h->shard_cut_nq == nc) {   // a call of several chunks: the cut-tie flags of all of them
            GH_CHECK(h, h->w_shard_cut.ensure((size_t)nq));
            GH_CHECK(h, hipMemcpyAsync(h->w_shard_cut.as<uint8_t>() + q0, h->w_tcut.p, (size_t)nc, hipMemcpyDeviceToDevice, h->stream));
        } else if (chunk < nq) {
            all_cut = false;
        }
    }
    h->shard_cut_chunked = chunk < nq && all_cut;
    if (h->shard_cut_chunked) h->shard_cut_nq = nq;
    h->last_P = Pe;
    h->last_R = R;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_search_shard_preassigned(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                             const float* d_x, const float* d_coarse_dis,
                                             const int32_t* d_probe, int k, float* d_recall_dis,
                                             int64_t* d_recall_ids) {
    return shard_preassigned(h, p, nq, d_x, d_coarse_dis, d_probe, k, d_recall_dis, d_recall_ids, nullptr);
}

int gamma_hip_bound_combine(void* stream, float* d_acc, const float* d_in, int n, int take_max) {
    if (n < 0 || (n > 0 && (!d_acc || !d_in))) return GAMMA_HIP_EINVAL;
    gh::launch_bound_combine(static_cast<hipStream_t>(stream), d_acc, d_in, n, take_max);
    return hipGetLastError() == hipSuccess ? GAMMA_HIP_OK : GAMMA_HIP_EDEVICE;
}

int gamma_hip_ivfpq_search_shard_bounded(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                         const float* d_x, const float* d_coarse_dis, const int32_t* d_probe, int k,
                                         float* d_recall_dis, int64_t* d_recall_ids, float* d_bound,
                                         gamma_hip_bound_reduce_fn reduce, void* user) {
    BoundXchg bx;
    bx.d_bound = d_bound;
    bx.fn = reduce;
    bx.user = user;
    return shard_preassigned(h, p, nq, d_x, d_coarse_dis, d_probe, k, d_recall_dis, d_recall_ids, &bx);
}

static int merge_rerank_impl(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq,
                             const float* d_x, int k, const float* d_all_dis, const int64_t* d_all_ids, const float* d_all_exact,
                             int q0, int nq_local, float* d_distances, int64_t* d_labels);
int gamma_hip_ivfpq_merge_rerank(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq,
                                 const float* d_x, int k, const float* d_all_dis, const int64_t* d_all_ids,
                                 int q0, int nq_local, float* d_distances, int64_t* d_labels) {
    return merge_rerank_impl(h, p, nshards, nq, d_x, k, d_all_dis, d_all_ids, nullptr, q0, nq_local, d_distances, d_labels);
}
int gamma_hip_ivfpq_merge_rerank_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq,
                                       const float* d_x, int k, const float* d_all_dis, const int64_t* d_all_ids,
                                       const float* d_all_exact, int q0, int nq_local, float* d_distances, int64_t* d_labels) {
    if (!d_all_exact) return GAMMA_HIP_EINVAL;
    return merge_rerank_impl(h, p, nshards, nq, d_x, k, d_all_dis, d_all_ids, d_all_exact, q0, nq_local, d_distances, d_labels);
}
static int merge_rerank_impl(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq,
                             const float* d_x, int k, const float* d_all_dis, const int64_t* d_all_ids, const float* d_all_exact,
                             int q0, int nq_local, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_merge_rerank(_exact)");
    if (!raw_store_served(h, false, false) && p && p->has_rank && !d_all_exact) return raw_store_refuse(h, "gamma_hip_ivfpq_merge_rerank without travelled distances");
    GH_TRY(replay_join(h));
    GH_TRY(ivfpq_check(h, p, nq, k));
    if (nshards <= 0 || q0 < 0 || nq_local < 0 || q0 + nq_local > nq) return fail(h, GAMMA_HIP_EINVAL, "bad shard/query range");
    if (k <= 0 || nq_local == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    const int R = std::max(p->recall_num, k);
    if ((int64_t)nshards * R > (int64_t)1 << 24) return fail(h, GAMMA_HIP_EINVAL, "too many candidates");
    hipStream_t s = h->stream;
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq_local * R * sizeof(float)));
    GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq_local * R * sizeof(int64_t)));
    {
        StageScope t(h, GAMMA_HIP_STAGE_SELECT);
        static const bool no_merge_kernel = getenv("GAMMA_HIP_NO_MERGE_KERNEL") != nullptr;
        if (no_merge_kernel ||
            !gh::launch_merge_shards(s, l2, d_all_dis, d_all_ids, nshards, nq, R, q0, nq_local,
                                     h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>())) {
            // general shapes: transpose to [nq][W * R], select, translate positions to ids
            GH_CHECK(h, h->w_m_dis.ensure((size_t)nq * nshards * R * sizeof(float)));
            GH_CHECK(h, h->w_m_ids.ensure((size_t)nq * nshards * R * sizeof(int64_t)));
            GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq_local * R * sizeof(int)));
            gh::launch_gather_shards(s, d_all_dis, d_all_ids, nshards, nq, R, h->w_m_dis.as<float>(),
                                     h->w_m_ids.as<int64_t>(), l2 ? INFINITY : -INFINITY);
            const int64_t stride = (int64_t)nshards * R;
            gh::launch_select_topk(s, l2, h->w_m_dis.as<float>() + (size_t)q0 * stride, stride, nullptr,
                                   (int)stride, (int)stride, nq_local, R, h->w_cand_dis.as<float>(),
                                   h->w_cand_pos.as<int>());
            gh::launch_take_ids(s, h->w_cand_pos.as<int>(), h->w_m_ids.as<int64_t>() + (size_t)q0 * stride, stride,
                                nq_local, R, h->w_cand_ids.as<int64_t>());
        }
        GH_CHECK(h, hipGetLastError());
    }
    // exact ties: the slice's queries whose result a tie can change are listed (gamma_hip_ivfpq_merge_flagged); the
    // caller gathers their candidate streams from the shards and has them replayed (gamma_hip_ivfpq_merge_replay)
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    const bool ties = tie_on(p);
    h->merge_flags = ties;
    h->merge_nql = nq_local;
    if (ties) {
        GH_CHECK(h, h->w_tcut.ensure((size_t)nq_local));
        GH_CHECK(h, h->w_tlist.ensure(((size_t)nq_local + 1) * sizeof(int)));
        GH_CHECK(h, hipMemsetAsync(h->w_tlist.p, 0, sizeof(int), s));
        gh::launch_flag_merge_cut(s, d_all_dis, nshards, nq, R, q0, nq_local, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(),
                                  h->w_tcut.as<uint8_t>(), h->merge_shard_flags);
    }
    h->merge_shard_flags = nullptr;   // one merge, with ties or without
    if (d_all_exact && p->has_rank) {
        // raw vectors sharded with their lists: the exact distance of every candidate travelled with it (computed by the shard
        // that holds the row, score window applied there).  compute_dis (gamma_index_ivfpq.cc:646-680) from those: the merged
        // candidates' distances are looked up in the shard tables, then the non-fused finish of stage B -- top-k of the row of
        // exact distances (equal distances keep the ADC order), output, tie flags.
        const float neutral = neutral_of(l2);
        StageScope t(h, GAMMA_HIP_STAGE_RERANK);
        GH_CHECK(h, h->w_exact.ensure((size_t)nq_local * R * sizeof(float)));
        GH_CHECK(h, h->w_selv.ensure((size_t)nq_local * k * sizeof(float)));
        GH_CHECK(h, h->w_selp.ensure((size_t)nq_local * k * sizeof(int)));
        gh::launch_lookup_exact(s, l2, d_all_dis, d_all_ids, d_all_exact, nshards, nq, R, q0, nq_local, h->w_cand_dis.as<float>(),
                                h->w_cand_ids.as<int64_t>(), h->w_exact.as<float>());
        gh::launch_select_topk(s, l2, h->w_exact.as<float>(), R, nullptr, R, R, nq_local, k, h->w_selv.as<float>(), h->w_selp.as<int>());
        gh::launch_finalize_topk(s, h->w_selv.as<float>(), h->w_selp.as<int>(), nq_local, k, h->w_cand_ids.as<int64_t>(), R, 0, neutral,
                                 d_distances, d_labels);
        if (ties) {
            gh::TieFlags tf;
            tf.cut = h->w_tcut.as<uint8_t>();
            tf.count = h->w_tlist.as<int>();
            tf.list = h->w_tlist.as<int>() + 1;
            tf.stats = h->d_tie_stats;
            GH_CHECK(h, h->w_textra.ensure((size_t)nq_local));
            GH_CHECK(h, hipMemsetAsync(h->w_textra.p, 0, (size_t)nq_local, s));
            gh::launch_flag_cut_ties(s, h->w_exact.as<float>(), R, nullptr, nq_local, k, h->w_selv.as<float>(), h->w_selp.as<int>(),
                                     h->w_textra.as<uint8_t>(), R, 1);
            gh::launch_tie_list(s, tf.cut, h->w_textra.as<uint8_t>(), nq_local, tf.list, tf.count, tf.stats);
        }
        GH_CHECK(h, hipGetLastError());
        return GAMMA_HIP_OK;
    }
    return ivfpq_stage_b(h, p, nq_local, d_x + (size_t)q0 * h->d, R, k, h->w_cand_dis.as<float>(),
                         h->w_cand_ids.as<int64_t>(), d_distances, d_labels, nullptr, ties ? 2 : 0);
}

int gamma_hip_ivfpq_shard_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                const int64_t* d_ids, int R, float* d_exact) {
    if (!h || !p) return GAMMA_HIP_EINVAL;
    if (nq <= 0 || R <= 0) return GAMMA_HIP_OK;
    if (!d_x || !d_ids || !d_exact) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_shard_exact");
    if (!shard_exact_served(h)) return raw_store_refuse(h, "gamma_hip_ivfpq_shard_exact");
    GH_TRY(replay_join(h));
    if (!h->has_raw_rows() || h->raw_d != h->d) return fail(h, GAMMA_HIP_EINVAL, "no raw store");
    GH_CHECK(h, hipSetDevice(h->device));
    // (a dense store answers for every id; a sharded one for the vectors it holds, the sentinel elsewhere)
    gh::launch_rerank_dist(h->stream, p->metric == GAMMA_HIP_METRIC_L2, d_x, nq, h->d, raw_rows_ref(h), h->nraw, d_ids, R, p->min_score,
                           p->max_score, d_exact, h->raw_sparse ? h->d_raw_slot.get() : nullptr, h->raw_sparse ? h->raw_slot_cap() : 0);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_shard_export_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                       const float* d_vals, const int64_t* d_ids, const int32_t* d_off, int64_t stride,
                                       const float* d_bound_f, float* d_ex) {
    if (!h || !p) return GAMMA_HIP_EINVAL;
    if (nf <= 0) return GAMMA_HIP_OK;
    if (!d_xf || !d_vals || !d_ids || !d_off || !d_bound_f || !d_ex || stride < 1) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_shard_export_exact");
    if (!shard_exact_served(h)) return raw_store_refuse(h, "gamma_hip_ivfpq_shard_export_exact");
    if (!h->has_raw_rows() || h->raw_d != h->d || !h->raw_sparse) return fail(h, GAMMA_HIP_EINVAL, "export of exact distances: a sharded raw store (gamma_hip_raw_put)");
    GH_CHECK(h, hipSetDevice(h->device));
    gh::launch_export_exact(h->stream, p->metric == GAMMA_HIP_METRIC_L2, d_xf, nf, h->d, raw_rows_ref(h), h->d_raw_slot, h->raw_slot_cap(),
                            d_vals, d_ids, stride, d_off, p->nprobe, d_bound_f, d_ex);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_shard_cut_flags(gamma_hip_index* h, int nq, uint8_t* d_flags) {
    if (!h || nq < 0 || (nq > 0 && !d_flags)) return GAMMA_HIP_EINVAL;
    if (nq == 0) return GAMMA_HIP_OK;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_shard_cut_flags");
    GH_CHECK(h, hipSetDevice(h->device));
    if (h->shard_cut_nq == nq) {
        GH_CHECK(h, hipMemcpyAsync(d_flags, h->shard_cut_chunked ? h->w_shard_cut.p : h->w_tcut.p, (size_t)nq,
                                   hipMemcpyDeviceToDevice, h->stream));
    } else {
        // no flags from the last shard search (exact ties off, or beyond the replay's range): "may have cut a tie"
        GH_CHECK(h, hipMemsetAsync(d_flags, 1, (size_t)nq, h->stream));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_merge_set_shard_flags(gamma_hip_index* h, const uint8_t* d_flags) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_merge_set_shard_flags");
    h->merge_shard_flags = d_flags;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_merge_flagged(gamma_hip_index* h, int* n_flagged, const int32_t** d_list) {
    if (!h || !n_flagged) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_merge_flagged");
    *n_flagged = 0;
    if (d_list) *d_list = nullptr;
    if (!h->merge_flags) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    int n = 0;
    GH_CHECK(h, hipMemcpyAsync(&n, h->w_tlist.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    *n_flagged = std::min(n, h->merge_nql);
    if (d_list) *d_list = h->w_tlist.as<int32_t>() + 1;
    return GAMMA_HIP_OK;
}

int gamma_hip_gather_rows(gamma_hip_index* h, const void* d_src, int row_words, const int32_t* d_list, int n, void* d_dst) {
    if (!h || row_words <= 0 || n < 0) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    if (!d_src || !d_list || !d_dst) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    gh::launch_gather_words(h->stream, d_src, d_list, n, row_words, d_dst);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_shard_export_rows(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const int32_t* d_probe_f,
                                      int64_t* max_entries) {
    if (!h || !p || !max_entries) return GAMMA_HIP_EINVAL;
    *max_entries = 0;
    if (nf <= 0) return GAMMA_HIP_OK;
    if (!d_probe_f) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_shard_export_rows");
    GH_TRY(replay_join(h));
    if (!h->ivf_init || h->ivfflat) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, h->w_qtotal.ensure(sizeof(int)));
    GH_CHECK(h, hipMemsetAsync(h->w_qtotal.p, 0, sizeof(int), h->stream));
    GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ver_ev[h->cur_ver], 0));
    gh::launch_shard_export_rows(h->stream, d_probe_f, nf, p->nprobe, h->d_list_len, h->d_list_mask, h->nlist, h->w_qtotal.as<int>());
    int mx = 0;
    GH_CHECK(h, hipMemcpyAsync(&mx, h->w_qtotal.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    *max_entries = mx;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_shard_export(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                 const float* d_cdis_f, const int32_t* d_probe_f, int64_t stride, float* d_vals, int64_t* d_ids,
                                 int32_t* d_off) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_shard_export");
    GH_TRY(replay_join(h));
    GH_TRY(ivfpq_check(h, p, nf, 1));
    if (nf == 0) return GAMMA_HIP_OK;
    if (!d_xf || !d_cdis_f || !d_probe_f || !d_vals || !d_ids || !d_off) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (p->nprobe > gh::tie_replay_max_probes()) return fail(h, GAMMA_HIP_EINVAL, "nprobe beyond the replay's range");
    GH_CHECK(h, hipSetDevice(h->device));
    const int P = p->nprobe, R = std::max(p->recall_num, 1);
    if (stride < 1) return fail(h, GAMMA_HIP_EINVAL, "stride");
    gamma_hip_search_params pp = *p;   // the scan behind an export flags nothing: its top-R goes to scratch
    pp.exact_ties = -1;
    p = &pp;
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    // the plain scan (every distance of the owned probed lists in the slab, scan order); its top-R goes to scratch
    const bool saved_bound = h->scan_bound;
    h->scan_bound = false;
    const int chunk = query_chunk(h, nf, P);
    int rc = GAMMA_HIP_OK;
    for (int f0 = 0; f0 < nf && rc == GAMMA_HIP_OK; f0 += chunk) {
        const int nc = std::min(chunk, nf - f0);
        rc = h->w_m_dis.ensure((size_t)nc * R * sizeof(float)) == hipSuccess &&
                     h->w_m_ids.ensure((size_t)nc * R * sizeof(int64_t)) == hipSuccess
                 ? GAMMA_HIP_OK
                 : fail(h, GAMMA_HIP_ENOMEM, "export scratch");
        if (rc == GAMMA_HIP_OK)
            rc = ivfpq_stage_a(h, p, fc.at(f0), nc, d_xf + (size_t)f0 * h->d, R, d_cdis_f + (size_t)f0 * P,
                               d_probe_f + (size_t)f0 * P, /*shard=*/true, h->w_m_dis.as<float>(), h->w_m_ids.as<int64_t>());
        if (rc == GAMMA_HIP_OK)
            gh::launch_shard_export(h->stream, d_probe_f + (size_t)f0 * P, nc, P, h->d_list_len, h->d_list_off, h->d_list_mask,
                                    h->nlist, h->d_ids, h->w_dist.as<float>(), h->tie.q_stride, stride,
                                    d_vals + (size_t)f0 * stride, d_ids + (size_t)f0 * stride, d_off + (size_t)f0 * (P + 1));
    }
    h->scan_bound = saved_bound;
    if (rc != GAMMA_HIP_OK) return rc;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

static int merge_replay_impl(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf, const float* d_x_slice,
                             int64_t stride, const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all, const float* d_ex_all,
                             int k, const int32_t* d_list, float* d_distances, int64_t* d_labels);
int gamma_hip_ivfpq_merge_replay(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf, const float* d_x_slice,
                                 int64_t stride, const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all, int k,
                                 const int32_t* d_list, float* d_distances, int64_t* d_labels) {
    return merge_replay_impl(h, p, nshards, nf, d_x_slice, stride, d_vals_all, d_ids_all, d_off_all, nullptr, k, d_list, d_distances, d_labels);
}
int gamma_hip_ivfpq_merge_replay_exact(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf, const float* d_x_slice,
                                       int64_t stride, const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all,
                                       const float* d_ex_all, int k, const int32_t* d_list, float* d_distances, int64_t* d_labels) {
    if (!d_ex_all) return GAMMA_HIP_EINVAL;
    return merge_replay_impl(h, p, nshards, nf, d_x_slice, stride, d_vals_all, d_ids_all, d_off_all, d_ex_all, k, d_list, d_distances, d_labels);
}
static int merge_replay_impl(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf, const float* d_x_slice,
                             int64_t stride, const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all, const float* d_ex_all,
                             int k, const int32_t* d_list, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_NO_PQ4(h, "gamma_hip_ivfpq_merge_replay(_exact)");
    if (!raw_store_served(h, false, false) && p && p->has_rank && !d_ex_all) return raw_store_refuse(h, "gamma_hip_ivfpq_merge_replay without travelled distances");
    GH_TRY(ivfpq_check(h, p, nf, k));
    if (nf == 0 || k <= 0) return GAMMA_HIP_OK;
    if (!d_x_slice || !d_vals_all || !d_ids_all || !d_off_all || !d_list || !d_distances || !d_labels)
        return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (!h->merge_flags) return fail(h, GAMMA_HIP_EINVAL, "no merge with tie flags before the replay");
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    const int P = p->nprobe, R = std::max(p->recall_num, k);
    if (R > gh::tie_replay_max_k() || P > gh::tie_replay_max_probes()) return fail(h, GAMMA_HIP_EINVAL, "beyond the replay's range");
    if (p->has_rank && !d_ex_all && (!h->raw_f32() || h->raw_d != h->d || h->raw_sparse))
        return fail(h, GAMMA_HIP_EINVAL, "has_rank needs the raw store (or the exact distances exported with the streams)");
    hipStream_t s = h->stream;
    const int64_t mstride = ((int64_t)nshards * stride + 3) & ~(int64_t)3;   // a row assembled from every shard's export
    GH_CHECK(h, h->w_mr_vals.ensure((size_t)nf * mstride * sizeof(float)));
    GH_CHECK(h, h->w_mr_ids.ensure((size_t)nf * mstride * sizeof(int64_t)));
    GH_CHECK(h, h->w_mr_meta.ensure((size_t)nf * (P + 1) * sizeof(int32_t) + (size_t)nf * P * sizeof(int64_t) + 64));
    int64_t* m_base = h->w_mr_meta.as<int64_t>();
    int* count = reinterpret_cast<int*>(m_base + (size_t)nf * P);
    int32_t* m_off = count + 16;
    GH_CHECK(h, hipMemcpyAsync(count, &nf, sizeof(int), hipMemcpyHostToDevice, s));
    gh::launch_merge_streams(s, nshards, nf, P, stride, mstride, d_vals_all, d_ids_all, d_off_all, h->w_mr_vals.as<float>(),
                             h->w_mr_ids.as<int64_t>(), m_off, m_base, l2 ? INFINITY : -INFINITY);
    gh::TieReplayArgs a;
    if (d_ex_all && p->has_rank) {
        // the exported exact distances, assembled probe by probe exactly like the ADC values (same positions); the ids of this
        // second pass go to scratch.  A member of the recall_num-heap whose distance no shard exported is COUNTED and fails the call.
        GH_CHECK(h, h->w_fslab.ensure((size_t)nf * mstride * sizeof(float)));
        GH_CHECK(h, h->w_m_ids.ensure((size_t)nf * mstride * sizeof(int64_t)));
        GH_CHECK(h, h->w_lm_cnt.ensure(64));
        GH_CHECK(h, hipMemsetAsync(h->w_lm_cnt.p, 0, sizeof(int), s));
        gh::launch_merge_streams(s, nshards, nf, P, stride, mstride, d_ex_all, d_ids_all, d_off_all, h->w_fslab.as<float>(),
                                 h->w_m_ids.as<int64_t>(), m_off, m_base, __builtin_nanf(""));
        a.ex_slab = h->w_fslab.as<float>();
        a.ex_missing = h->w_lm_cnt.as<int>();
    }
    a.list = d_list;
    a.count = count;
    a.nq = nf;
    a.slab = h->w_mr_vals.as<float>();
    a.q_stride = mstride;
    a.pair_off = m_off;
    a.pair_base = m_base;
    a.ids = h->w_mr_ids.as<int64_t>();
    a.P = P;
    a.G = P;
    a.ready = nullptr;
    a.surv = nullptr;
    a.gcnt = nullptr;
    a.nsl = 0;
    a.slice_cap = 0;
    a.x = d_x_slice;
    a.d = h->d;
    a.rows = gh::RowsRef{h->raw_f32()};
    a.nraw = h->nraw;
    a.R = R;
    a.k = k;
    a.has_rank = p->has_rank ? 1 : 0;
    a.min_score = p->min_score;
    a.max_score = p->max_score;
    a.neutral = neutral_of(l2);
    a.cand_dis = h->w_cand_dis.as<float>();     // the merged tables of the slice (gamma_hip_ivfpq_merge_rerank)
    a.cand_ids = h->w_cand_ids.as<int64_t>();
    a.distances = d_distances;
    a.labels = d_labels;
    a.compact_rows = 1;
    gh::launch_tie_replay(s, l2, a);
    GH_CHECK(h, hipGetLastError());
    if (a.ex_missing) {
        int missing = 0;
        GH_CHECK(h, hipMemcpyAsync(&missing, a.ex_missing, sizeof(int), hipMemcpyDeviceToHost, s));
        GH_CHECK(h, hipStreamSynchronize(s));
        if (missing) return fail(h, GAMMA_HIP_EDEVICE, "tie replay: a member of the recall_num-heap arrived without its exact distance");
    }
    return GAMMA_HIP_OK;
}

}  // extern "C"
