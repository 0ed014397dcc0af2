// gamma_hip.cpp -- libgamma_hip.so, C ABI of include/gamma_hip.h: the handle's life cycle, the per-handle switches,
// memory accounting and stage profiling.  The writers (realtime lists, raw store, columns, bitmap) are in
// gamma_hip_store.cpp, the search pipelines and their entry points in gamma_hip_search.cpp and its three siblings
// (gamma_hip_search_ivfflat.cpp, _flat.cpp, _shard.cpp), the handle itself in
// gamma_hip_internal.h.  No CPU fallback anywhere: an entry point runs the HIP kernels or returns an error.
#include "gamma_hip_internal.h"

using namespace ghi;

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* gamma_hip_strerror(int code) {
    switch (code) {
        case GAMMA_HIP_OK: return "ok";
        case GAMMA_HIP_EINVAL: return "invalid argument";
        case GAMMA_HIP_ENOTTRAINED: return "index not trained";
        case GAMMA_HIP_EDEVICE: return "HIP runtime error";
        case GAMMA_HIP_ENOMEM: return "out of memory";
        case GAMMA_HIP_EFULL: return "inverted list full";
        case GAMMA_HIP_EUNSUPPORTED: return "exact ties requested beyond the replay's range";
        default: return "unknown error";
    }
}

int gamma_hip_create(int device, gamma_hip_index** out) {
    if (!out) return GAMMA_HIP_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GAMMA_HIP_EDEVICE;
    if (device < 0 || device >= ndev) return GAMMA_HIP_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return GAMMA_HIP_EDEVICE;
    H* h = new (std::nothrow) H();
    if (!h) return GAMMA_HIP_ENOMEM;
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->wstream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->side2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_rfork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_rdone, hipEventDisableTiming) != hipSuccess) {
        delete h;
        return GAMMA_HIP_EDEVICE;
    }
    for (int v = 0; v < H::NVER; v++)
        if (hipEventCreateWithFlags(&h->ver_ev[v], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->rd_ev[v], hipEventDisableTiming) != hipSuccess) {
            delete h;
            return GAMMA_HIP_EDEVICE;
        }
    if (hipMalloc((void**)&h->d_scan_codes, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(h->d_scan_codes, 0, sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&h->d_tie_stats, 3 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(h->d_tie_stats, 0, 3 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&h->bound_fb.d_stat, 5 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(h->bound_fb.d_stat, 0, 5 * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc((void**)&h->bound_fb.pin_stat, 4 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        (void)hipStreamDestroy(h->stream);
        delete h;
        return GAMMA_HIP_EDEVICE;
    }
    memset(h->bound_fb.pin_stat, 0, 4 * sizeof(unsigned long long));
    // workspace budget of the chunked buffers: an eighth of the device memory, 1..32 GiB (36 GB -> 32 GiB
    // on a 288 GB MI355X); gamma_hip_set_workspace_budget overrides
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0)
        h->dist_budget_bytes = std::min<size_t>((size_t)32 << 30, std::max<size_t>((size_t)1 << 30, total_b / 8));
    *out = h;
    return GAMMA_HIP_OK;
}

int gamma_hip_destroy(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_OK;
    {
        std::unique_lock<std::mutex> lk(h->comb_mu);
        h->comb_stop = true;
        h->comb_wcv.notify_all();
    }
    if (h->comb_thread.joinable()) h->comb_thread.join();
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->wstream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    h->call_slots.release();
    for (auto& sl : h->hslot) {
        if (sl.pin) (void)hipHostFree(sl.pin);
        if (sl.ev_up) (void)hipEventDestroy(sl.ev_up);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (h->up_stream) (void)hipStreamDestroy(h->up_stream);
    for (hipEvent_t& e : h->ev_bank)
        if (e) (void)hipEventDestroy(e);
    if (h->ev_rfork) (void)hipEventDestroy(h->ev_rfork);
    if (h->ev_rdone) (void)hipEventDestroy(h->ev_rdone);
    for (int v = 0; v < H::NVER; v++) {
        if (h->ver_ev[v]) (void)hipEventDestroy(h->ver_ev[v]);
        if (h->rd_ev[v]) (void)hipEventDestroy(h->rd_ev[v]);
        if (h->d_ver_off[v]) (void)hipFree(h->d_ver_off[v]);
        if (h->d_ver_len[v]) (void)hipFree(h->d_ver_len[v]);
        if (h->pin_ver[v]) (void)hipHostFree(h->pin_ver[v]);
    }
    for (auto& e : h->events) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    // the one-shot allocations of the model and the counters (never grown, never moved)
    void* ptrs[] = {h->d_list_rank, h->d_sq8_tab, h->d_cc, h->d_cc_norms, h->d_pqc, h->d_T2, h->d_list_mask, h->d_scan_codes,
                    h->d_tie_stats, h->d_t2max, h->bound_fb.d_stat, h->d_bin_cc, h->d_bin_stats, h->d_bf_stats, h->d_cc_img,
                    h->d_cbf_stat, h->d_opq, h->rf.par, h->rf.d_stat};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
    for (void* pp : h->comb_pin)
        if (pp) (void)hipHostFree(pp);
    if (h->dir_pin) (void)hipHostFree(h->dir_pin);
    if (h->bound_fb.copy_ev) (void)hipEventDestroy(h->bound_fb.copy_ev);
    if (h->bound_fb.pin_stat) (void)hipHostFree(h->bound_fb.pin_stat);
    if (h->cbf_copy_ev) (void)hipEventDestroy(h->cbf_copy_ev);
    if (h->pin_cbf_stat) (void)hipHostFree(h->pin_cbf_stat);
    if (h->rf.copy_ev) (void)hipEventDestroy(h->rf.copy_ev);
    if (h->rf.built) (void)hipEventDestroy(h->rf.built);
    if (h->rf.pin_stat) (void)hipHostFree(h->rf.pin_stat);
    (void)hipStreamDestroy(h->stream);
    (void)hipStreamDestroy(h->wstream);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->side2) (void)hipStreamDestroy(h->side2);
    // Everything above is destroyed by hand because the runtime hands it out as a bare handle or pointer: streams, events,
    // pinned host memory, the one-shot allocations.  Device memory that grows has an owner -- the workspaces (DevBuf), the
    // raw store, the columns, the bitmap, the tables (DevArray), the arena's sets and the retired address ranges (ArenaSets)
    // -- and the owners free themselves here, with the handle's device still current (hipSetDevice above) and its streams
    // drained.
    delete h;
    return GAMMA_HIP_OK;
}

const char* gamma_hip_last_error(gamma_hip_index* h) { return h ? h->err.c_str() : "null handle"; }
void* gamma_hip_stream(gamma_hip_index* h) { return h ? (void*)h->stream : nullptr; }

int gamma_hip_synchronize(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    if (h->side) GH_CHECK(h, hipStreamSynchronize(h->side));
    if (h->side2) GH_CHECK(h, hipStreamSynchronize(h->side2));
    h->replay_pending = false;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_deferred_replay(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!on && h->replay_pending) {
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_rdone, 0));
        h->replay_pending = false;
    }
    h->defer_replay = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_join(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (h->replay_pending) {
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_rdone, 0));
        h->replay_pending = false;
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_dim(gamma_hip_index* h) { return (h && h->ivf_init) ? h->d : 0; }
int gamma_hip_ivfpq_nlist(gamma_hip_index* h) { return (h && h->ivf_init) ? h->nlist : 0; }
int gamma_hip_ivfpq_code_size(gamma_hip_index* h) { return (h && h->ivf_init) ? h->code_size : 0; }

int gamma_hip_set_exact_ties(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->exact_ties = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_coarse_fused(gamma_hip_index* h, int on, int list_cap) {
    if (!h || list_cap < 1 || list_cap > gh::kCoarseCap) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->coarse_fused = on == 0 ? 0 : (on == 2 ? 2 : 1);
    h->coarse_cap = list_cap;
    h->cbf_off_calls = 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_coarse_filter_stats(gamma_hip_index* h, int64_t* out4) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    unsigned long long v[2] = {0, 0};
    if (h->d_cbf_stat) {
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        GH_CHECK(h, hipMemcpy(v, h->d_cbf_stat, sizeof(v), hipMemcpyDeviceToHost));
    }
    out4[0] = (int64_t)v[0];
    out4[1] = (int64_t)v[1];
    out4[2] = h->cbf_backoffs;
    out4[3] = h->cbf_off_calls;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_rerank_filter(gamma_hip_index* h, int mode) {
    if (!h || mode < 0 || mode > 2) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->rf.mode = mode;
    h->rf.off_calls = 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_rerank_filter_stats(gamma_hip_index* h, int64_t* out5) {
    if (!h || !out5) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    std::vector<unsigned long long> v(gh::kRerankFilterStatLines * 16, 0);
    if (h->rf.d_stat) {
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        GH_CHECK(h, hipMemcpy(v.data(), h->rf.d_stat, gh::rerank_filter_stat_bytes(), hipMemcpyDeviceToHost));
    }
    out5[0] = (int64_t)h->rf.cand;
    out5[1] = 0;
    for (int i = 0; i < gh::kRerankFilterStatLines; i++) out5[1] += (int64_t)v[16 * i];
    out5[2] = h->rf.calls;
    out5[3] = h->rf.backoffs;
    out5[4] = h->rf.on ? h->nraw : 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_rerank_filter_form(gamma_hip_index* h, int form) {
    if (!h || form < 0 || form > 2) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->rf.form = form;
    return GAMMA_HIP_OK;
}

int gamma_hip_rerank_filter_form(gamma_hip_index* h, int64_t* out4) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    out4[0] = h->rf.form;
    out4[1] = h->rf.last_form;
    out4[2] = h->rf.wave_calls;
    out4[3] = gh::kRerankWaveAutoMinNq;
    return GAMMA_HIP_OK;
}

int gamma_hip_flat_filter_shape(int d, int* d_pad, float* margin) { return gh::flat_filter_shape(d, d_pad, margin); }

int gamma_hip_flat_filter_stats(gamma_hip_index* h, int64_t* out3, int reset) {
    if (!h || !out3) return GAMMA_HIP_EINVAL;
    out3[0] = reset ? h->ff_passes.exchange(0) : h->ff_passes.load();
    out3[1] = reset ? h->ff_pairs.exchange(0) : h->ff_pairs.load();
    out3[2] = reset ? h->ff_redone.exchange(0) : h->ff_redone.load();
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile) {
    if (!kind || !slab || !qtile) return GAMMA_HIP_EINVAL;
    gh::ivfflat_lm_shape(d, kind, slab, qtile);
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_scan_stats(gamma_hip_index* h, int64_t* out4, int reset) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    out4[0] = reset ? h->fl_small.exchange(0) : h->fl_small.load();
    out4[1] = reset ? h->fl_pair.exchange(0) : h->fl_pair.load();
    out4[2] = reset ? h->fl_lm.exchange(0) : h->fl_lm.load();
    out4[3] = reset ? h->fl_lms.exchange(0) : h->fl_lms.load();
    return GAMMA_HIP_OK;
}

int gamma_hip_set_small_path(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->small_path = on != 0;
    h->small_presel = on >= 2 ? on : 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_flat_narrow_rows(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->flat_narrow_rows = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_ivfflat_narrow_rows(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->ivfflat_narrow_rows = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_sparse_narrow_rows(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->sparse_narrow_rows = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_flat_sq8_rows(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->flat_sq8_rows = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_set_ivfflat_sq8_rows(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->ivfflat_sq8_rows = on != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_tie_stats(gamma_hip_index* h, int64_t* out3, int reset) {
    if (!h || !out3) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    // (everything on the handle's own streams: a null-stream hipMemset is asynchronous and NOT ordered against the
    //  non-blocking search stream -- a reset could land after the next search's first increments)
    if (h->side) GH_CHECK(h, hipStreamSynchronize(h->side));
    if (h->side2) GH_CHECK(h, hipStreamSynchronize(h->side2));
    unsigned long long v[3];
    GH_CHECK(h, hipMemcpyAsync(v, h->d_tie_stats, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    if (reset) GH_CHECK(h, hipMemsetAsync(h->d_tie_stats, 0, sizeof(v), h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) out3[i] = (int64_t)v[i];
    return GAMMA_HIP_OK;
}

int gamma_hip_ties_not_honoured(gamma_hip_index* h, int64_t* out_calls, int reset) {
    if (!h || !out_calls) return GAMMA_HIP_EINVAL;
    *out_calls = reset ? h->ties_unhonoured.exchange(0) : h->ties_unhonoured.load();
    return GAMMA_HIP_OK;
}

int gamma_hip_blas_form_not_restated(gamma_hip_index* h, int64_t* out_calls, int reset) {
    if (!h || !out_calls) return GAMMA_HIP_EINVAL;
    *out_calls = reset ? h->blas_unrestated.exchange(0) : h->blas_unrestated.load();
    return GAMMA_HIP_OK;
}

int gamma_hip_set_scan_bound_feedback(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->bound_fb.set_on(on != 0);
    return GAMMA_HIP_OK;
}

int gamma_hip_scan_bound_stats(gamma_hip_index* h, int64_t* out4) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    GH_CHECK(h, hipMemcpy(v, h->bound_fb.d_stat, sizeof(v), hipMemcpyDeviceToHost));
    const int slot = h->bound_fb.slot();   // the counts of the current kind of call
    out4[0] = (int64_t)v[2 * slot];
    out4[1] = (int64_t)v[2 * slot + 1];
    out4[2] = h->bound_fb.backoffs;
    out4[3] = (int64_t)v[4];
    return GAMMA_HIP_OK;
}

int gamma_hip_set_workspace_budget(gamma_hip_index* h, int64_t bytes) {
    if (!h || bytes <= 0) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->dist_budget_bytes = (size_t)bytes;
    return GAMMA_HIP_OK;
}

/* ---- accounting ----------------------------------------------------------------------------- */
int64_t gamma_hip_total_mem_bytes(gamma_hip_index* h) {
    if (!h) return -1;
    std::lock_guard<std::mutex> g(h->mu);
    int64_t b = 0;
    b += h->raw_cap() * h->raw_d * (int64_t)h->raw_esz() + h->raw_slot_cap() * (int64_t)sizeof(int32_t);
    if (h->d_sq8_tab) b += (int64_t)h->raw_d * 4 * (int64_t)sizeof(float);   // sq8 store: the decode and the encode table
    b += (int64_t)(h->rf.rows.cap + h->rf.aux.cap);   // the re-rank filter's image, once a call has built it: d + 8 bytes per row
    b += (int64_t)h->d_bitmap.cap;
    for (auto& kv : h->fields) b += (int64_t)kv.second.d.cap;
    for (auto& kv : h->terms) b += (int64_t)(kv.second.d_off.cap + kv.second.d_tok.cap);
    b += (int64_t)h->d_bf_codes.cap;   // the binary flat store
    if (h->ivf_init) {
        b += (int64_t)h->nlist * h->d * 4 + (int64_t)h->nlist * 4 + (int64_t)h->M * 256 * h->dsub * 4;
        if (h->d_T2) b += h->ivfflat ? 256 : (int64_t)h->nlist * h->M * 256 * 4;
        b += h->arena_cap * (h->code_size + (int64_t)sizeof(int64_t));
        if (h->d_sums) b += h->arena_cap * (int64_t)sizeof(float) + (int64_t)h->nlist * 4;
        b += (int64_t)h->nlist * 12;
        b += (int64_t)h->cc_img_bytes;
        // the shadow arena of calls that run over lists compacted under their filter (kept between calls)
        b += (int64_t)(h->w_cmp_codes.cap + h->w_cmp_ids.cap + h->w_cmp_len.cap);
    }
    return b;
}

int gamma_hip_profile_enable(gamma_hip_index* h, int on) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->profile = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return GAMMA_HIP_OK;
}

int gamma_hip_profile_reset(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(drain_events(h));
    for (int i = 0; i < GAMMA_HIP_NUM_STAGES; i++) {
        h->stage_ms[i] = 0;
        h->stage_n[i] = 0;
    }
    h->scan_pairs = 0;
    GH_CHECK(h, hipMemsetAsync(h->d_scan_codes, 0, sizeof(unsigned long long), h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    return GAMMA_HIP_OK;
}

int gamma_hip_profile_get(gamma_hip_index* h, int stage, double* total_ms, int64_t* launches) {
    if (!h || stage < 0 || stage >= GAMMA_HIP_NUM_STAGES) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(drain_events(h));
    if (total_ms) *total_ms = h->stage_ms[stage];
    if (launches) *launches = h->stage_n[stage];
    return GAMMA_HIP_OK;
}

int gamma_hip_profile_scan_bytes(gamma_hip_index* h, int64_t* bytes, int64_t* pairs) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    unsigned long long codes = 0;
    GH_CHECK(h, hipMemcpy(&codes, h->d_scan_codes, sizeof(codes), hipMemcpyDeviceToHost));
    if (bytes) *bytes = (int64_t)codes * h->code_size;
    if (pairs) *pairs = h->scan_pairs;
    return GAMMA_HIP_OK;
}

}  // extern "C"