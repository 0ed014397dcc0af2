// gamma_hip_binivf.cpp -- the binary IVF model's entry points (index/impl/gamma_index_binary_ivf.{h,cc}): the coarse
// quantizer's search (IndexBinaryFlat), Add (assign + AddKeys), Search (search_knn_hamming_heap).  Init / set_trained
// live with the other models' in gamma_hip_store.cpp, training in gamma_hip_train.cpp, the kernels in binivf.hip.
#include "binivf.h"
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

using namespace ghi;

namespace {

// the row stride (bytes) of the queries staged through host_search, whose rows are whole floats
inline int bin_row_words(int cs) { return (cs + 3) / 4; }

int bin_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int64_t xs, int k,
                             float* d_distances, int64_t* d_labels) {
    if (!p) return fail(h, GAMMA_HIP_EINVAL, "null params");
    if (nq < 0) return fail(h, GAMMA_HIP_EINVAL, "nq < 0");
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "binivf not trained");
    if (k > gh::kBinMaxK) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binivf: k > 4096 (the scan's heap lives in LDS)");
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    // GammaIndexBinaryIVF::Search (:290-299): the request's nprobe if it lies in (0, nlist], else the model's 20
    const int P = (p->nprobe > 0 && p->nprobe <= h->nlist) ? p->nprobe : 20;
    if (P > gh::kBinMaxProbe) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binivf: nprobe > 4096");
    if (h->arena_cap >= ((int64_t)1 << 31)) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binivf: more than 2^31 list entries");
    GH_CHECK(h, hipSetDevice(h->device));
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt, nullptr, 0));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    const int need_filter = (fc.any_clause || (h->d_bitmap && h->bitmap_any)) ? 1 : 0;
    hipStream_t s = h->stream;
    const int ver = h->cur_ver;
    GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
    GH_CHECK(h, h->w_probe.ensure((size_t)nq * P * sizeof(int)));
    {
        StageScope t(h, GAMMA_HIP_STAGE_COARSE);
        gh::launch_bin_coarse(s, d_x, nq, xs, h->d_bin_cc, h->nlist, h->code_size, P, h->w_probe.as<int>(), nullptr);
    }
    // one wave per query (k_bin_scan), or the query's scan spread over the device (binivf_spread.hip): the same answer.
    // The chain's workspaces are sized from the longest list of the version this call reads (max_list_len is set where
    // the version is published), so nothing comes back from the device before the launches.
    static const bool no_spread = getenv("GAMMA_HIP_NO_BIN_SPREAD") != nullptr;
    const int mode = no_spread ? 0 : h->bin_scan_mode;
    bool spread = mode == 1 || (mode == -1 && nq <= gh::kBinSpreadAutoMaxNq);
    int maxch = 0;
    int64_t stride = 0;
    size_t hist_b = 0, meta_b = 0, cand_b = 0;
    if (spread) {
        gh::bin_spread_bounds(P, h->nlist, h->max_list_len, &maxch, &stride);
        hist_b = (size_t)nq * maxch * ((size_t)h->code_size * 8 + 1) * sizeof(uint32_t);
        meta_b = gh::bin_spread_meta_bytes(nq, maxch);
        cand_b = (size_t)nq * (size_t)stride * sizeof(uint2);
        if (nq > gh::kBinSpreadMaxNq || maxch > 65535 * 32 || hist_b + meta_b + cand_b > h->dist_budget_bytes / 2) {
            spread = false;   // never wrong, only slower
            if (h->profile) h->bin_sp_fallback += nq;
        }
    }
    if (spread) {
        GH_CHECK(h, h->w_bs_hist.ensure(hist_b));
        GH_CHECK(h, h->w_bs_meta.ensure(meta_b));
        GH_CHECK(h, h->w_bs_cand.ensure(cand_b));
        const int stages[3] = {GAMMA_HIP_STAGE_TABLES, GAMMA_HIP_STAGE_SCAN, GAMMA_HIP_STAGE_SELECT};
        for (int st = 0; st < 3; st++) {   // chunk table + histograms + bounds | collect | replay
            StageScope t(h, stages[st]);
            gh::launch_bin_spread(s, d_x, nq, xs, h->code_size, h->w_probe.as<int>(), P, h->d_list_off, h->d_list_len,
                                  h->d_codes, h->d_ids, fc.d_tab, need_filter, p->min_score, p->max_score, k, maxch, stride,
                                  h->w_bs_hist.as<uint32_t>(), h->w_bs_meta.p, h->w_bs_cand.as<uint2>(), d_distances,
                                  d_labels, h->profile ? h->d_bin_stats : nullptr,
                                  h->profile ? h->d_bin_stats + 2 : nullptr, st + 1);
        }
    } else {
        StageScope t(h, GAMMA_HIP_STAGE_SCAN);
        gh::launch_bin_scan(s, d_x, nq, xs, h->code_size, h->w_probe.as<int>(), P, h->d_list_off, h->d_list_len, h->d_codes,
                            h->d_ids, fc.d_tab, need_filter, p->min_score, p->max_score, k, d_distances, d_labels,
                            h->profile ? h->d_bin_stats : nullptr);   // counted only while profiling
    }
    GH_CHECK(h, hipGetLastError());
    GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
    h->rd_set[ver] = true;
    return GAMMA_HIP_OK;
}

}  // namespace

extern "C" {

int gamma_hip_binivf_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int k,
                                   float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    return bin_search_device_locked(h, p, nq, d_x, h->code_size, k, d_distances, d_labels);
}

int gamma_hip_binivf_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* x, int k,
                            float* distances, int64_t* labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    if (nq > 0 && k > 0 && (!x || !distances || !labels)) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (nq <= 0 || k <= 0 || k > gh::kBinMaxK) return bin_search_device_locked(h, p, nq, nullptr, 0, k, nullptr, nullptr);
    // rows padded to whole words, so that the shared staging path (pinned buffers, results stored in place) carries them
    const int cs = h->code_size, rw = bin_row_words(cs);
    std::vector<float> rows((size_t)nq * rw, 0.f);
    for (int i = 0; i < nq; i++) memcpy(reinterpret_cast<char*>(rows.data() + (size_t)i * rw), x + (size_t)i * cs, cs);
    return host_search(h, nq, rw, rows.data(), k, distances, labels, [&](const float* dx, float* dd, int64_t* dl) {
        return bin_search_device_locked(h, p, nq, reinterpret_cast<const uint8_t*>(dx), (int64_t)rw * 4, k, dd, dl);
    }, true, &lk);
}

// quantizer->search (IndexBinaryFlat::search, faiss:IndexBinaryFlat.cpp:33-59): the k nearest centroid codes of every
// code, best first; labels -1 / distances INT32_MAX padded (k > nlist).  k = 1 is quantizer->assign.
int gamma_hip_binivf_assign(gamma_hip_index* h, int64_t n, const uint8_t* codes, int k, int32_t* distances, int64_t* labels) {
    if (!h || n < 0 || k <= 0 || (n > 0 && (!codes || !labels))) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "binivf not trained");
    if (k > gh::kBinMaxProbe) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binivf_assign: k > 4096");
    if (n == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(replay_join(h));
    hipStream_t s = h->stream;
    const int cs = h->code_size;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)1 << 26) / ((int64_t)k * 8 + cs)));
    std::vector<int> lab((size_t)std::min(n, chunk) * k);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int nc = (int)std::min(chunk, n - i0);
        GH_CHECK(h, h->w_x.ensure((size_t)nc * cs));
        GH_CHECK(h, h->w_probe.ensure((size_t)nc * k * sizeof(int)));
        GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nc * k * sizeof(int)));
        GH_CHECK(h, hipMemcpyAsync(h->w_x.p, codes + i0 * cs, (size_t)nc * cs, hipMemcpyHostToDevice, s));
        gh::launch_bin_coarse(s, h->w_x.as<uint8_t>(), nc, cs, h->d_bin_cc, h->nlist, cs, k, h->w_probe.as<int>(),
                              h->w_coarse_dis.as<int>());
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipMemcpyAsync(lab.data(), h->w_probe.p, (size_t)nc * k * sizeof(int), hipMemcpyDeviceToHost, s));
        if (distances)
            GH_CHECK(h, hipMemcpyAsync(distances + i0 * k, h->w_coarse_dis.p, (size_t)nc * k * sizeof(int),
                                       hipMemcpyDeviceToHost, s));
        GH_CHECK(h, hipStreamSynchronize(s));
        for (int64_t i = 0; i < (int64_t)nc * k; i++) labels[i0 * k + i] = lab[i];
    }
    return GAMMA_HIP_OK;
}

// GammaIndexBinaryIVF::Add (:148-206): quantizer->assign of the batch on the device (the writer stream), then AddKeys of
// every list's entries in vid order, vids first_vid, first_vid + 1, ..
int gamma_hip_binivf_add(gamma_hip_index* h, int64_t n, const uint8_t* codes, int64_t first_vid) {
    if (!h || n < 0 || (n > 0 && !codes) || first_vid < 0) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    std::vector<int> lno((size_t)n);
    int cs = 0, nlist = 0;
    {
        WriteLock lk(h);
        if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
        if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "binivf not trained");   // FAISS_THROW_IF_NOT(is_trained)
        GH_CHECK(h, hipSetDevice(h->device));
        cs = h->code_size;
        nlist = h->nlist;
        const int64_t chunk = std::min<int64_t>(n, (int64_t)1 << 20);
        GH_CHECK(h, h->we_codes.ensure((size_t)chunk * cs));
        GH_CHECK(h, h->we_assign.ensure((size_t)chunk * sizeof(int)));
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int nc = (int)std::min(chunk, n - i0);
            GH_CHECK(h, hipMemcpyAsync(h->we_codes.p, codes + i0 * cs, (size_t)nc * cs, hipMemcpyHostToDevice, h->wstream));
            gh::launch_bin_coarse(h->wstream, h->we_codes.as<uint8_t>(), nc, cs, h->d_bin_cc, nlist, cs, 1,
                                  h->we_assign.as<int>(), nullptr);
            GH_CHECK(h, hipGetLastError());
            GH_CHECK(h, hipMemcpyAsync(lno.data() + i0, h->we_assign.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost,
                                       h->wstream));
            GH_CHECK(h, hipStreamSynchronize(h->wstream));
        }
    }
    // new_keys / new_codes: std::map by list, each list's entries in vid order
    std::vector<int64_t> order;
    order.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++)
        if (lno[i] >= 0 && lno[i] < nlist) order.push_back(i);   // list_no < 0: ignored (:175-178)
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return lno[a] < lno[b]; });
    std::vector<int32_t> lists, counts;
    std::vector<int64_t> vids(order.size());
    std::vector<uint8_t> gcodes(order.size() * (size_t)cs);
    // vids are numbered over the entries that are added (the ignored ones take none)
    std::vector<int64_t> vid_of((size_t)n, -1);
    {
        int64_t v = first_vid;
        for (int64_t i = 0; i < n; i++)
            if (lno[i] >= 0 && lno[i] < nlist) vid_of[i] = v++;
    }
    for (size_t i = 0; i < order.size(); i++) {
        const int64_t src = order[i];
        vids[i] = vid_of[src];
        memcpy(gcodes.data() + i * cs, codes + (size_t)src * cs, cs);
        if (lists.empty() || lists.back() != lno[src]) {
            lists.push_back(lno[src]);
            counts.push_back(0);
        }
        counts.back()++;
    }
    if (lists.empty()) return GAMMA_HIP_OK;
    return gamma_hip_ivfpq_add_keys_batch(h, (int)lists.size(), lists.data(), counts.data(), vids.data(), gcodes.data());
}

// {queries searched, heap admissions of their scans} of the searches made while profiling was on, since the last reset
int gamma_hip_binivf_stats(gamma_hip_index* h, int64_t* out2, int reset) {
    if (!h || !out2) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    unsigned long long v[2] = {0, 0};
    GH_CHECK(h, hipMemcpyAsync(v, h->d_bin_stats, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    out2[0] = (int64_t)v[0];
    out2[1] = (int64_t)v[1];
    if (reset) {
        GH_CHECK(h, hipMemsetAsync(h->d_bin_stats, 0, sizeof(v), h->stream));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
    }
    return GAMMA_HIP_OK;
}

// which scan answers a search (both give scan_codes' answer, gamma_index_binary_ivf.cc:333-448): 0 k_bin_scan, one wave
// per query; 1 the spread chain whenever its workspace fits; -1 the chain for calls of up to auto_max_nq queries
int gamma_hip_binivf_set_scan_mode(gamma_hip_index* h, int mode) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    if (mode < -1 || mode > 1) return fail(h, GAMMA_HIP_EINVAL, "binivf scan mode: -1, 0 or 1");
    h->bin_scan_mode = mode;
    return GAMMA_HIP_OK;
}

int gamma_hip_binivf_scan_mode(const gamma_hip_index* h) {
    if (!h || !h->ivf_init || !h->binivf) return GAMMA_HIP_EINVAL;
    return h->bin_scan_mode;
}

int gamma_hip_binivf_scan_shape(int* chunk_rows, int* auto_max_nq) {
    if (chunk_rows) *chunk_rows = gh::kBinSpreadChunk;
    if (auto_max_nq) *auto_max_nq = gh::kBinSpreadAutoMaxNq;
    return GAMMA_HIP_OK;
}

// {queries the spread chain answered, their chunks, their candidates, queries that fell back to k_bin_scan for lack of
// workspace} of the searches made while profiling was on, since the last reset
int gamma_hip_binivf_scan_stats(gamma_hip_index* h, int64_t* out4, int reset) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    unsigned long long v[3] = {0, 0, 0};
    GH_CHECK(h, hipMemcpyAsync(v, h->d_bin_stats + 2, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) out4[i] = (int64_t)v[i];
    out4[3] = h->bin_sp_fallback;
    if (reset) {
        GH_CHECK(h, hipMemsetAsync(h->d_bin_stats + 2, 0, sizeof(v), h->stream));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        h->bin_sp_fallback = 0;
    }
    return GAMMA_HIP_OK;
}

}  // extern "C"
