// gamma_hip_search_ivfflat_shard.cpp -- the IVFFLAT search over list shards, entry points of the C ABI (include/gamma_hip.h):
// a shard's coarse quantizer, its preassigned search over the lists it holds and owns (rows from a dense or a sparse store:
// fp32, or float16 / uint8 / int8 after gamma_hip_set_ivfflat_narrow_rows), the merge of the shards' top-k tables with the tie flags, the exact distances a shard exports for the flagged
// queries and the replay of the assembled streams through the IVFFLAT scanner's heap.  The kernels are the single-handle
// search's (ivfflat.hip, rerank.hip: their sparse variants where the rows live with their lists) and the list shards' of the
// IVFPQ path (select.hip k_merge_shards, ties.hip k_flag_merge_cut / k_shard_export / k_merge_streams / k_tie_replay).
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

namespace ghi {
namespace {

// what every entry below asks of the handle; `what` names the entry in the refusal of a narrow store.  A float16 / uint8 / int8
// store is served where the single-handle search serves it (gamma_hip_set_ivfflat_narrow_rows); an sq8 store never is.
int ivfflat_shard_check(H* h, const gamma_hip_search_params* p, int nq, int k, const char* what, bool need_rows) {
    GH_TRY(check_params(h, p, nq, k));
    if (!h->ivf_init || !h->ivfflat || h->binivf) return fail(h, GAMMA_HIP_EINVAL, "ivfflat not initialised");
    if (need_rows && !raw_store_served(h, h->ivfflat_narrow_rows, false)) return raw_store_refuse(h, what);
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "ivfflat not trained");
    if (p->nprobe <= 0 || p->nprobe > h->nlist) return fail(h, GAMMA_HIP_EINVAL, "nprobe out of range");
    if (need_rows && (!h->has_raw_rows() || h->raw_d != h->d)) return fail(h, GAMMA_HIP_EINVAL, "ivfflat needs the raw store");
    return GAMMA_HIP_OK;
}

// One chunk's scan: pair offsets over the lists this handle's mask owns, then the exact distances of their entries into the
// slab (h->w_dist, rows of q_stride).  List-major when enough pairs share lists -- under a mask too: the kernels get a
// list-length table in which an unowned list is empty -- else one workgroup per pair.  A sparse store goes through the sparse
// variant of the same three kernels.
int ivfflat_shard_scan(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nc, const float* xq, const int* probe,
                       int64_t q_stride) {
    const int P = p->nprobe, nlist = h->nlist;
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    hipStream_t s = h->stream;
    GH_CHECK(h, h->w_pair_off.ensure((size_t)nc * (P + 1) * sizeof(int)));
    GH_CHECK(h, h->w_pair_base.ensure((size_t)nc * P * sizeof(int64_t)));
    GH_CHECK(h, h->w_qtotal.ensure((size_t)nc * sizeof(int)));
    GH_CHECK(h, h->w_dist.ensure((size_t)nc * q_stride * sizeof(float)));
    gh::launch_pair_offsets(s, probe, nc, P, h->d_list_len, h->d_list_mask, nlist, h->w_pair_off.as<int>(), h->w_qtotal.as<int>(),
                            nullptr, h->d_list_off, h->w_pair_base.as<int64_t>());
    const int need_filter = (fc.any_clause || (h->d_bitmap && h->bitmap_any)) ? 1 : 0;
    // the store's rows as the scans take them: pointer + element type (fp32 rows: the launches they always were)
    const gh::RowsRef rows = raw_rows_ref(h);
    StageScope t(h, GAMMA_HIP_STAGE_SCAN);
    if (h->raw_sparse && !h->d_raw_slot) {   // a sparse store that never took a row: every entry is a filtered entry
        const int64_t n = (int64_t)nc * q_stride;
        for (int64_t o = 0; o < n; o += 1 << 30)
            gh::launch_fill_f32(s, h->w_dist.as<float>() + o, (int)std::min<int64_t>(n - o, 1 << 30), l2 ? INFINITY : -INFINITY);
        return GAMMA_HIP_OK;
    }
    static const bool no_lm = getenv("GAMMA_HIP_NO_IVFFLAT_LM") != nullptr;
    int lm_kind = 0, lm_slab = 0, lm_qtile = 0;
    gh::ivfflat_lm_shape(h->d, &lm_kind, &lm_slab, &lm_qtile);
    if (!no_lm && lm_kind != 0 && (int64_t)nc * P >= 2 * (int64_t)nlist) {
        (lm_kind == 1 ? h->fl_lm : h->fl_lms).fetch_add(1, std::memory_order_relaxed);
        const size_t sb = (gh::ivfflat_lm_scratch_bytes(nc, P, nlist) + 15) & ~(size_t)15;
        GH_CHECK(h, h->w_lm_units.ensure(sb + (size_t)nlist * sizeof(int)));
        const int* len = h->d_list_len;
        if (h->d_list_mask) {
            int* mlen = reinterpret_cast<int*>(static_cast<char*>(h->w_lm_units.p) + sb);
            gh::launch_masked_list_len(s, h->d_list_len, h->d_list_mask, nlist, mlen);
            len = mlen;
        }
        if (h->raw_sparse)
            gh::launch_ivfflat_lm_sparse(s, l2, xq, nc, h->d, P, probe, h->w_pair_off.as<int>(), h->d_list_off, len, nlist, h->d_ids,
                                         rows, h->nraw, h->d_raw_slot, h->raw_slot_cap(), q_stride, h->w_dist.as<float>(), fc.d_tab,
                                         need_filter, p->min_score, p->max_score, h->w_lm_units.p);
        else
            gh::launch_ivfflat_lm(s, l2, xq, nc, h->d, P, probe, h->w_pair_off.as<int>(), h->d_list_off, len, nlist, h->d_ids,
                                  rows, h->nraw, q_stride, h->w_dist.as<float>(), fc.d_tab, need_filter, p->min_score,
                                  p->max_score, h->w_lm_units.p);
    } else {
        h->fl_pair.fetch_add(1, std::memory_order_relaxed);
        if (h->raw_sparse)
            gh::launch_ivfflat_scan_sparse(s, l2, xq, nc, h->d, P, h->w_pair_off.as<int>(), h->w_pair_base.as<int64_t>(), h->d_ids,
                                           rows, h->nraw, h->d_raw_slot, h->raw_slot_cap(), q_stride, h->w_dist.as<float>(),
                                           fc.d_tab, need_filter, p->min_score, p->max_score);
        else
            gh::launch_ivfflat_scan(s, l2, xq, nc, h->d, P, h->w_pair_off.as<int>(), h->w_pair_base.as<int64_t>(), h->d_ids, rows,
                                    h->nraw, q_stride, h->w_dist.as<float>(), fc.d_tab, need_filter, p->min_score, p->max_score);
    }
    return GAMMA_HIP_OK;
}

}  // namespace
}  // namespace ghi

using namespace ghi;

extern "C" {

int gamma_hip_ivfflat_coarse_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                    float* d_coarse_dis, int32_t* d_probe) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    GH_TRY(ivfflat_shard_check(h, p, nq, 1, "gamma_hip_ivfflat_coarse_device", false));
    if (nq == 0) return GAMMA_HIP_OK;
    if (!d_x || !d_coarse_dis || !d_probe) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    GH_CHECK(h, hipSetDevice(h->device));
    const int P = p->nprobe;
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, P <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    // the caller resolves coarse_mode -1 on the size of the whole batch; a slice that arrives unresolved decides by itself
    if (pp.coarse_mode < 0) pp.coarse_mode = nq < 20 ? 0 : 1;
    if (pp.coarse_mode == 1 && blas_form_not_restated(nq, h->nlist, h->d)) h->blas_unrestated++;
    const int chunk = coarse_chunk(h, nq);
    for (int q0 = 0; q0 < nq; q0 += chunk)
        GH_TRY(ivfpq_coarse(h, &pp, std::min(chunk, nq - q0), d_x + (size_t)q0 * h->d, d_coarse_dis + (size_t)q0 * P,
                            d_probe + (size_t)q0 * P));
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_search_shard(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x,
                                   const float* d_coarse_dis, const int32_t* d_probe, int k, float* d_dis, int64_t* d_ids) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    h->shard_cut_nq = 0;
    h->shard_cut_chunked = false;
    GH_TRY(ivfflat_shard_check(h, p, nq, k, "gamma_hip_ivfflat_search_shard", true));
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    (void)d_coarse_dis;   // (the IVFFLAT scan takes nothing from the coarse distances; the argument keeps the IVFPQ entry's shape)
    if (!d_x || !d_probe || !d_dis || !d_ids) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    const float neutral = neutral_of(l2);
    const int P = p->nprobe;
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt, nullptr, (int64_t)nq * P * (h->ntotal / std::max(1, h->nlist))));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    hipStream_t s = h->stream;
    const bool ties = tie_on(p);
    const int chunk = scan_chunk(h, nq, P);
    const int64_t q_stride = slab_q_stride(h, P);
    if (ties) GH_CHECK(h, h->w_shard_cut.ensure(std::max<size_t>((size_t)nq, 16)));
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nc = std::min(chunk, nq - q0);
        const float* xq = d_x + (size_t)q0 * h->d;
        const int* probe = d_probe + (size_t)q0 * P;
        float* out_d = d_dis + (size_t)q0 * k;
        int64_t* out_i = d_ids + (size_t)q0 * k;
        const int ver = h->cur_ver;
        GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
        GH_CHECK(h, h->w_cand_pos.ensure((size_t)nc * k * sizeof(int)));
        GH_CHECK(h, h->w_cand_dis.ensure((size_t)nc * k * sizeof(float)));
        GH_CHECK(h, h->w_cand_ids.ensure((size_t)nc * k * sizeof(int64_t)));
        GH_TRY(ivfflat_shard_scan(h, p, fc, nc, xq, probe, q_stride));
        {
            StageScope t(h, GAMMA_HIP_STAGE_SELECT);
            gh::launch_select_topk(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), 0,
                                   (int)std::min<int64_t>(q_stride, 1 << 30), nc, k, h->w_cand_dis.as<float>(),
                                   h->w_cand_pos.as<int>());
            gh::launch_map_candidates(s, h->w_cand_pos.as<int>(), nc, k, P, probe, h->w_pair_off.as<int>(), h->d_list_off, h->d_ids,
                                      h->w_cand_ids.as<int64_t>());
            gh::TieFlags tf;
            if (ties) {
                // the shard's own result honours its local ties (flag + replay, as the single-handle search); what the merge
                // needs is narrower -- did the k cut go through a group of equal distances? -- and is kept per query of the
                // WHOLE call, whatever the chunking (gamma_hip_ivfpq_shard_cut_flags reads it)
                GH_CHECK(h, h->w_tcut.ensure((size_t)nc));
                GH_CHECK(h, h->w_tlist.ensure(((size_t)nc + 1) * sizeof(int)));
                GH_CHECK(h, hipMemsetAsync(h->w_tlist.p, 0, sizeof(int), s));
                GH_CHECK(h, hipMemsetAsync(h->w_tcut.p, 0, (size_t)nc, s));
                GH_CHECK(h, hipMemsetAsync(h->w_shard_cut.as<uint8_t>() + q0, 0, (size_t)nc, s));
                gh::launch_flag_cut_ties(s, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nc, k, h->w_cand_dis.as<float>(),
                                         h->w_cand_pos.as<int>(), h->w_tcut.as<uint8_t>(), 0, 1);
                gh::launch_flag_cut_ties(s, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nc, k, h->w_cand_dis.as<float>(),
                                         h->w_cand_pos.as<int>(), h->w_shard_cut.as<uint8_t>() + q0, 0, 0);
                tf.cut = h->w_tcut.as<uint8_t>();
                tf.count = h->w_tlist.as<int>();
                tf.list = h->w_tlist.as<int>() + 1;
                tf.stats = h->d_tie_stats;
            }
            gh::launch_finalize_norank(s, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), nc, k, k, p->min_score, p->max_score,
                                       neutral, out_d, out_i, ties ? &tf : nullptr);
            if (ties) {
                gh::TieReplayArgs tr;
                flat_tie_args(h, &tr, l2, nc, q_stride, P, k, xq, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), out_d, out_i);
                tr.list = tf.list;
                tr.count = tf.count;
                gh::launch_tie_replay(s, l2, tr);
            }
        }
        GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
        h->rd_set[ver] = true;
        h->last_nq = nc;
    }
    if (ties) {
        h->shard_cut_nq = nq;
        h->shard_cut_chunked = true;   // (always gathered in w_shard_cut: w_tcut holds the wider local flags)
    }
    h->last_P = P;
    h->last_R = k;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_shard_export_rows(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const int32_t* d_probe_f,
                                        int64_t* max_entries) {
    if (!h || !p || !max_entries) return GAMMA_HIP_EINVAL;
    *max_entries = 0;
    if (nf <= 0) return GAMMA_HIP_OK;
    if (!d_probe_f) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    if (!h->ivf_init || !h->ivfflat || h->binivf) return fail(h, GAMMA_HIP_EINVAL, "ivfflat not initialised");
    if (p->nprobe <= 0 || p->nprobe > h->nlist) return fail(h, GAMMA_HIP_EINVAL, "nprobe out of range");
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

int gamma_hip_ivfflat_shard_export(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf,
                                   const int32_t* d_probe_f, int64_t stride, float* d_vals, int64_t* d_ids, int32_t* d_off) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    GH_TRY(ivfflat_shard_check(h, p, nf, 1, "gamma_hip_ivfflat_shard_export", true));
    if (nf == 0) return GAMMA_HIP_OK;
    if (!d_xf || !d_probe_f || !d_vals || !d_ids || !d_off) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (p->nprobe > gh::tie_replay_max_probes()) return fail(h, GAMMA_HIP_EINVAL, "nprobe beyond the replay's range");
    if (stride < 1) return fail(h, GAMMA_HIP_EINVAL, "stride");
    GH_CHECK(h, hipSetDevice(h->device));
    const int P = p->nprobe;
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    hipStream_t s = h->stream;
    const int chunk = scan_chunk(h, nf, P);
    const int64_t q_stride = slab_q_stride(h, P);
    for (int f0 = 0; f0 < nf; f0 += chunk) {
        const int nc = std::min(chunk, nf - f0);
        const int ver = h->cur_ver;
        GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
        GH_TRY(ivfflat_shard_scan(h, p, fc, nc, d_xf + (size_t)f0 * h->d, d_probe_f + (size_t)f0 * P, q_stride));
        gh::launch_shard_export(s, d_probe_f + (size_t)f0 * P, nc, P, h->d_list_len, h->d_list_off, h->d_list_mask, h->nlist, h->d_ids,
                                h->w_dist.as<float>(), q_stride, stride, d_vals + (size_t)f0 * stride, d_ids + (size_t)f0 * stride,
                                d_off + (size_t)f0 * (P + 1));
        GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
        h->rd_set[ver] = true;
    }
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_merge(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq, int k, const float* d_all_dis,
                            const int64_t* d_all_ids, int q0, int nq_local, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    const uint8_t* shard_flags = h->merge_shard_flags;
    h->merge_shard_flags = nullptr;   // one merge, with ties or without
    h->merge_flags = false;
    GH_TRY(ivfflat_shard_check(h, p, nq, k, "gamma_hip_ivfflat_merge", false));
    if (nshards <= 0 || q0 < 0 || nq_local < 0 || q0 + nq_local > nq) return fail(h, GAMMA_HIP_EINVAL, "bad shard/query range");
    if (k <= 0 || nq_local == 0) return GAMMA_HIP_OK;
    if (!d_all_dis || !d_all_ids || !d_distances || !d_labels) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if ((int64_t)nshards * k > (int64_t)1 << 24) return fail(h, GAMMA_HIP_EINVAL, "too many candidates");
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    hipStream_t s = h->stream;
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq_local * k * sizeof(float)));
    GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq_local * k * sizeof(int64_t)));
    StageScope t(h, GAMMA_HIP_STAGE_SELECT);
    if (!gh::launch_merge_shards(s, l2, d_all_dis, d_all_ids, nshards, nq, k, q0, nq_local, h->w_cand_dis.as<float>(),
                                 h->w_cand_ids.as<int64_t>())) {
        // general shapes: transpose to [nq][W * k], select, translate positions to ids
        GH_CHECK(h, h->w_m_dis.ensure((size_t)nq * nshards * k * sizeof(float)));
        GH_CHECK(h, h->w_m_ids.ensure((size_t)nq * nshards * k * sizeof(int64_t)));
        GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq_local * k * sizeof(int)));
        gh::launch_gather_shards(s, d_all_dis, d_all_ids, nshards, nq, k, h->w_m_dis.as<float>(), h->w_m_ids.as<int64_t>(),
                                 l2 ? INFINITY : -INFINITY);
        const int64_t stride = (int64_t)nshards * k;
        gh::launch_select_topk(s, l2, h->w_m_dis.as<float>() + (size_t)q0 * stride, stride, nullptr, (int)stride, (int)stride,
                               nq_local, k, h->w_cand_dis.as<float>(), h->w_cand_pos.as<int>());
        gh::launch_take_ids(s, h->w_cand_pos.as<int>(), h->w_m_ids.as<int64_t>() + (size_t)q0 * stride, stride, nq_local, k,
                            h->w_cand_ids.as<int64_t>());
    }
    // Exact ties: a query is listed when (a) two of its k merged results are equal (k_finalize_norank), (b) the merged cut
    // passes through a group of equal distances -- more entries equal to the k-th value in the shards' tables than the
    // merged table took (k_flag_merge_cut) -- or (c) a shard whose own cut went through a tie ends at the merged k-th value:
    // it may have dropped members of that group.  (a) + (b) are "two equal distances among the merged first k + 1".
    const bool ties = tie_on(p);
    gh::TieFlags tf;
    if (ties) {
        GH_CHECK(h, h->w_tcut.ensure((size_t)nq_local));
        GH_CHECK(h, h->w_tlist.ensure(((size_t)nq_local + 1) * sizeof(int)));
        GH_CHECK(h, hipMemsetAsync(h->w_tlist.p, 0, sizeof(int), s));
        gh::launch_flag_merge_cut(s, d_all_dis, nshards, nq, k, q0, nq_local, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(),
                                  h->w_tcut.as<uint8_t>(), shard_flags);
        tf.cut = h->w_tcut.as<uint8_t>();
        tf.count = h->w_tlist.as<int>();
        tf.list = h->w_tlist.as<int>() + 1;
        tf.stats = h->d_tie_stats;
    }
    gh::launch_finalize_norank(s, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), nq_local, k, k, p->min_score, p->max_score,
                               neutral_of(l2), d_distances, d_labels, ties ? &tf : nullptr);
    h->merge_flags = ties;
    h->merge_nql = nq_local;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_merge_replay(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nf, const float* d_x_slice,
                                   int64_t stride, const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all, int k,
                                   const int32_t* d_list, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(ivfflat_shard_check(h, p, nf, k, "gamma_hip_ivfflat_merge_replay", false));
    if (nf == 0 || k <= 0) return GAMMA_HIP_OK;
    if (!d_x_slice || !d_vals_all || !d_ids_all || !d_off_all || !d_list || !d_distances || !d_labels)
        return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (nshards <= 0 || stride < 1) return fail(h, GAMMA_HIP_EINVAL, "bad shard count / stride");
    if (!h->merge_flags) return fail(h, GAMMA_HIP_EINVAL, "no merge with tie flags before the replay");
    if (nf > h->merge_nql) return fail(h, GAMMA_HIP_EINVAL, "more flagged queries than the merge's slice holds");
    const int P = p->nprobe;
    if (k > gh::tie_replay_max_k() || P > gh::tie_replay_max_probes()) return fail(h, GAMMA_HIP_EINVAL, "beyond the replay's range");
    GH_CHECK(h, hipSetDevice(h->device));
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
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
    // the IVFFLAT scanner's heap over the assembled stream: `if (dis < top) { heap_pop; heap_push }`, then heap_reorder
    // (gamma_index_ivfflat.h:52-75); the k-heap IS the result, window and filters are in the stream (sentinels)
    gh::TieReplayArgs a;
    flat_tie_args(h, &a, l2, nf, mstride, P, k, d_x_slice, h->w_cand_dis.as<float>(), h->w_cand_ids.as<int64_t>(), d_distances,
                  d_labels);
    a.list = d_list;
    a.count = count;
    a.slab = h->w_mr_vals.as<float>();
    a.pair_off = m_off;
    a.pair_base = m_base;
    a.ids = h->w_mr_ids.as<int64_t>();
    a.compact_rows = 1;
    gh::launch_tie_replay(s, l2, a);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

}  // extern "C"
