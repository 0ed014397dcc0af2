// gamma_hip_search_ivfflat.cpp -- the IVFFLAT search of libgamma_hip.so: the small-batch chain, the chunked driver
// (pair-per-workgroup or list-major scan, top-k, tie replay) and its two entry points of the C ABI (include/gamma_hip.h).
// The coarse quantizer, list compaction and the exact scanners' helpers are gamma_hip_search.cpp's (gamma_hip_search.h).
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

namespace ghi {

// ---- IVFFLAT (index/impl/gamma_index_ivfflat.cc:392-567) ------------------------------------------------------
// coarse quantizer (the IVFPQ one) -> slab offsets -> exact distance of every entry of the probed lists
// (k_ivfflat_scan) -> top-k of the slab in (distance, scan position) order -> ids.  The reference's k-heap keeps
// the same k entries (up to its order inside exact ties).
// IVFFLAT, small batches: the chain of ivfpq_small without tables and re-rank -- exact coarse distances | top-nprobe +
// slab offsets | exact distances of the probed lists' rows, one workgroup per pair | top-k + ids + score window
int ivfflat_small(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, const gh::RowsRef& rows, int nq, const float* d_x,
                  int k, float* d_distances, int64_t* d_labels) {
    const int P = p->nprobe, d = h->d, nlist = h->nlist;
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    hipStream_t s = h->stream;
    const int ver = h->cur_ver;
    GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
    GH_CHECK(h, h->w_mat.ensure((size_t)nq * nlist * sizeof(float)));
    GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nq * P * sizeof(float)));
    GH_CHECK(h, h->w_probe.ensure((size_t)nq * P * sizeof(int)));
    GH_CHECK(h, h->w_pair_off.ensure((size_t)nq * (P + 1) * sizeof(int)));
    GH_CHECK(h, h->w_pair_base.ensure((size_t)nq * P * sizeof(int64_t)));
    GH_CHECK(h, h->w_qtotal.ensure((size_t)nq * sizeof(int)));
    GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq * k * sizeof(int)));
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq * k * sizeof(float)));
    GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq * k * sizeof(int64_t)));
    const int64_t q_stride = slab_q_stride(h, P);
    GH_CHECK(h, h->w_dist.ensure((size_t)nq * q_stride * sizeof(float)));
    if (p->coarse_mode == 1) {
        gh::launch_l2_gemmform(s, d_x, nq, d, h->d_cc, nlist, nullptr, h->d_cc_norms, h->w_mat.as<float>(), nlist, true);
    } else if (!gh::launch_small_coarse_ip(s, d_x, nq, d, h->d_cc, nlist, h->w_mat.as<float>(), 0, nullptr, nullptr)) {
        gh::launch_pairwise(s, true, d_x, nq, d, h->d_cc, nlist, h->w_mat.as<float>(), nlist);   // exact, more than 16 queries
    }
    gh::launch_small_coarse_select(s, h->w_mat.as<float>(), nlist, nq, P, h->w_coarse_dis.as<float>(), h->w_probe.as<int>(),
                                   h->d_list_len, h->d_list_mask, h->d_list_off, h->w_pair_off.as<int>(),
                                   h->w_qtotal.as<int>(), h->w_pair_base.as<int64_t>(), nullptr, nullptr, 0, nullptr, nullptr,
                                   nullptr, 0, tie_on(p) ? 1 : 0, h->d_tie_stats);
    const int need_filter = (fc.any_clause || (h->d_bitmap && h->bitmap_any)) ? 1 : 0;
    gh::launch_ivfflat_scan(s, l2, d_x, nq, d, P, h->w_pair_off.as<int>(), h->w_pair_base.as<int64_t>(), h->d_ids, rows,
                            h->nraw, q_stride, h->w_dist.as<float>(), fc.d_tab, need_filter, p->min_score, p->max_score);
    const int smax = small_presel_slices(h, P, nq);   // long candidate rows: two-level selection, as in ivfpq_small
    if (smax > 0) {
        GH_CHECK(h, h->w_selv.ensure((size_t)nq * smax * k * sizeof(float)));
        GH_CHECK(h, h->w_selp.ensure(((size_t)nq * smax * k + (size_t)nq * smax) * sizeof(int)));   // + a cut flag per slice
    }
    const float neutral = neutral_of(l2);
    // exact ties: a query with equal distances at the k cut or among its k results is replayed through the scanner's
    // heap (heap_pop + heap_push per accepted entry, heap_reorder: gamma_index_ivfflat.h:52-75) inside the tail kernel
    gh::TieReplayArgs tr;
    const bool ties = tie_on(p) && k <= gh::tie_small_max_k();   // (the caller's gate: k <= 1024)
    if (ties) flat_tie_args(h, &tr, l2, nq, q_stride, P, k, d_x, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), d_distances,
                            d_labels);
    gh::launch_small_tail(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nq, k, P, h->w_probe.as<int>(),
                          h->w_pair_off.as<int>(), h->d_list_off, h->d_ids, h->w_cand_dis.as<float>(),
                          h->w_cand_pos.as<int>(), h->w_cand_ids.as<int64_t>(), 0, d_x, d, h->raw_f32(), h->nraw, k, p->min_score,
                          p->max_score, neutral, d_distances, d_labels, smax, smax ? h->w_selv.as<float>() : nullptr,
                          smax ? h->w_selp.as<int>() : nullptr, 0, ties ? &tr : nullptr, h->d_tie_stats);
    GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
    h->rd_set[ver] = true;
    h->last_nq = nq;
    h->last_P = P;
    h->last_R = k;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int ivfflat_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int k,
                                 float* d_distances, int64_t* d_labels) {
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    // (a narrow store is served only after gamma_hip_set_ivfflat_narrow_rows: the refusal is what every caller had before;
    //  an sq8 store only after gamma_hip_set_ivfflat_sq8_rows, whatever the other switches say)
    if (!raw_store_served(h, h->ivfflat_narrow_rows, h->ivfflat_sq8_rows)) return raw_store_refuse(h, "IVFFLAT search");
    GH_TRY(check_params(h, p, nq, k));
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    if (!h->ivf_init || !h->ivfflat || h->binivf) return fail(h, GAMMA_HIP_EINVAL, "ivfflat not initialised");
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "ivfflat not trained");
    if (p->nprobe <= 0 || p->nprobe > h->nlist) return fail(h, GAMMA_HIP_EINVAL, "nprobe out of range");
    if (!h->has_raw_rows() || h->raw_d != h->d) return fail(h, GAMMA_HIP_EINVAL, "ivfflat needs the raw store");
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    // the store's rows as the scan takes them: pointer + element type (fp32 rows: the launches they always were)
    const gh::RowsRef rows = raw_rows_ref(h);
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    const float neutral = neutral_of(l2);
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt, nullptr, (int64_t)nq * p->nprobe * (h->ntotal / std::max(1, h->nlist))));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    if (pp.coarse_mode < 0) pp.coarse_mode = nq < 20 ? 0 : 1;   // faiss:utils/distances.cpp:303,346, whole call
    if (pp.coarse_mode == 1 && blas_form_not_restated(nq, h->nlist, h->d)) h->blas_unrestated++;
    const int P = pp.nprobe, nlist = h->nlist;
    hipStream_t s = h->stream;
    {   // small batches, as long as the pair-per-workgroup scan is the one that would run anyway (below 2 nlist pairs)
        static const bool off = getenv("GAMMA_HIP_NO_SMALL_PATH") != nullptr;
        if (!off && h->small_path && nq <= 512 && P <= 128 && k <= 1024 && !h->profile &&
            !fc.d_qf && !h->d_list_mask && nlist <= 16384 && (int64_t)nq * P < 2 * (int64_t)nlist &&
            (int64_t)P * std::max(1, h->max_list_len) <= (1 << 22)) {
            h->fl_small.fetch_add(1, std::memory_order_relaxed);
            return ivfflat_small(h, &pp, fc, rows, nq, d_x, k, d_distances, d_labels);
        }
    }
    ListCompaction restore(h);
    GH_TRY(compact_lists_for_call(h, &fc, (int64_t)nq * P * (h->ntotal / std::max(1, nlist)), true, &restore));
    const int chunk = scan_chunk(h, nq, P);
    const int need_filter = (!h->prefiltered && (fc.any_clause || (h->d_bitmap && h->bitmap_any))) ? 1 : 0;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nc = std::min(chunk, nq - q0);
        const float* xq = d_x + (size_t)q0 * h->d;
        const int ver = h->cur_ver;
        GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
        GH_CHECK(h, h->w_pair_off.ensure((size_t)nc * (P + 1) * sizeof(int)));
        GH_CHECK(h, h->w_pair_base.ensure((size_t)nc * P * sizeof(int64_t)));
        GH_CHECK(h, h->w_qtotal.ensure((size_t)nc * sizeof(int)));
        GH_CHECK(h, h->w_cand_pos.ensure((size_t)nc * k * sizeof(int)));
        GH_CHECK(h, h->w_cand_dis.ensure((size_t)nc * k * sizeof(float)));
        GH_CHECK(h, h->w_cand_ids.ensure((size_t)nc * k * sizeof(int64_t)));
        GH_TRY(ivfpq_coarse(h, &pp, nc, xq));
        gh::launch_pair_offsets(s, h->w_probe.as<int>(), nc, P, h->d_list_len, h->d_list_mask, nlist,
                                h->w_pair_off.as<int>(), h->w_qtotal.as<int>(), nullptr, h->d_list_off,
                                h->w_pair_base.as<int64_t>());
        const int64_t q_stride = slab_q_stride(h, P);
        GH_CHECK(h, h->w_dist.ensure((size_t)nc * q_stride * sizeof(float)));
        {
            StageScope t(h, GAMMA_HIP_STAGE_SCAN);
            // enough (query, probe) pairs that lists are shared: list-major (ivfflat.hip), a list's rows are read once
            // for all the queries probing it (d in {16, 32, 64, 96, 128}) or once per tile of them (the row-sliced kernel: every
            // other d % 16 == 0 up to 4096); else one workgroup per pair
            static const bool no_lm = getenv("GAMMA_HIP_NO_IVFFLAT_LM") != nullptr;
            int lm_kind = 0, lm_slab = 0, lm_qtile = 0;
            gh::ivfflat_lm_shape(h->d, &lm_kind, &lm_slab, &lm_qtile);
            if (!no_lm && lm_kind != 0 && (int64_t)nc * P >= 2 * (int64_t)nlist && !h->d_list_mask) {
                (lm_kind == 1 ? h->fl_lm : h->fl_lms).fetch_add(1, std::memory_order_relaxed);
                GH_CHECK(h, h->w_lm_units.ensure(gh::ivfflat_lm_scratch_bytes(nc, P, nlist)));
                gh::launch_ivfflat_lm(s, l2, xq, nc, h->d, P, h->w_probe.as<int>(), h->w_pair_off.as<int>(), h->d_list_off,
                                      h->d_list_len, nlist, h->d_ids, rows, h->nraw, q_stride, h->w_dist.as<float>(),
                                      fc.d_tab, need_filter, p->min_score, p->max_score, h->w_lm_units.p);
            } else {
                h->fl_pair.fetch_add(1, std::memory_order_relaxed);
                gh::launch_ivfflat_scan(s, l2, xq, nc, h->d, P, h->w_pair_off.as<int>(), h->w_pair_base.as<int64_t>(),
                                        h->d_ids, rows, h->nraw, q_stride, h->w_dist.as<float>(), fc.d_tab, need_filter,
                                        p->min_score, p->max_score);
            }
        }
        {
            StageScope t(h, GAMMA_HIP_STAGE_SELECT);
            gh::launch_select_topk(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), 0,
                                   (int)std::min<int64_t>(q_stride, 1 << 30), nc, k, h->w_cand_dis.as<float>(),
                                   h->w_cand_pos.as<int>());
            gh::launch_map_candidates(s, h->w_cand_pos.as<int>(), nc, k, P, h->w_probe.as<int>(), h->w_pair_off.as<int>(),
                                      h->d_list_off, h->d_ids, h->w_cand_ids.as<int64_t>());
            const bool ties = tie_on(p);
            gh::TieFlags tf;
            if (ties) {
                // equal distances at the k cut or among the k selected: the scanner's heap decides (ties.hip)
                GH_CHECK(h, h->w_tcut.ensure((size_t)nc));
                GH_CHECK(h, h->w_tlist.ensure(((size_t)nc + 1) * sizeof(int)));
                GH_CHECK(h, hipMemsetAsync(h->w_tlist.p, 0, sizeof(int), s));
                GH_CHECK(h, hipMemsetAsync(h->w_tcut.p, 0, (size_t)nc, s));
                gh::launch_flag_cut_ties(s, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nc, k, h->w_cand_dis.as<float>(),
                                         h->w_cand_pos.as<int>(), h->w_tcut.as<uint8_t>(), 0, 1);
                tf.cut = h->w_tcut.as<uint8_t>();
                tf.count = h->w_tlist.as<int>();
                tf.list = h->w_tlist.as<int>() + 1;
                tf.stats = h->d_tie_stats;
            }
            gh::launch_finalize_norank(s, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), nc, k, k, p->min_score,
                                       p->max_score, neutral, d_distances + (size_t)q0 * k, d_labels + (size_t)q0 * k,
                                       ties ? &tf : nullptr);
            if (ties) {
                gh::TieReplayArgs tr;
                flat_tie_args(h, &tr, l2, nc, q_stride, P, k, xq, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(),
                              d_distances + (size_t)q0 * k, d_labels + (size_t)q0 * k);
                tr.list = tf.list;
                tr.count = tf.count;
                gh::launch_tie_replay(s, l2, tr);
            }
        }
        GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
        h->rd_set[ver] = true;
        h->last_nq = nc;
    }
    h->last_P = P;
    h->last_R = k;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

}  // namespace ghi

using namespace ghi;

extern "C" {

int gamma_hip_ivfflat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                    int k, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    return ivfflat_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
}

int gamma_hip_ivfflat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                             float* distances, int64_t* labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(check_params(h, p, nq, k));
    if (!h->ivf_init || !h->ivfflat || h->binivf) return fail(h, GAMMA_HIP_EINVAL, "ivfflat not initialised");
    if (nq > 0 && k > 0 && (!x || !distances || !labels)) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    return host_search(h, nq, h->d, x, k, distances, labels, [&](const float* dx, float* dd, int64_t* dl) {
        return ivfflat_search_device_locked(h, p, nq, dx, k, dd, dl);
    }, true, &lk);
}

}  // extern "C"
