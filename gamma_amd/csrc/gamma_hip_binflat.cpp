// gamma_hip_binflat.cpp -- exact Hamming (binary flat) search: the store of every code in vid order and its entry points.
// The answer is faiss:IndexBinaryFlat.cpp / utils/hamming.cpp:230-265 over all stored codes as
// GammaIVFBinaryScannerL2::scan_codes (gamma_index_binary_ivf.cc:333-448) gives it for ONE list that holds every code in
// vid order; the kernels and the argument they rest on are in binflat.hip.
#include "binflat.h"
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"

using namespace ghi;

namespace {

inline int bin_row_words(int cs) { return (cs + 3) / 4; }

// the store holds cap rows afterwards.  Growth frees the old array, which a search in flight may read: it waits for them
// (DevArray::grow, the raw store's rule -- the first allocation waits too, though it frees nothing); the rows move on the
// writer stream.  Searches may start again afterwards.
int binflat_reserve(H* h, WriteLock& lk, int64_t cap) {
    if (cap <= h->bf_cap()) return GAMMA_HIP_OK;
    const int64_t want = std::max<int64_t>(cap, std::max<int64_t>(1024, h->bf_cap() + h->bf_cap() / 2));
    if (want >= ((int64_t)1 << 31)) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binflat: 2^31 rows or more");
    const int rc = grow_array(h, "binflat", h->d_bf_codes, (size_t)cap * h->bf_cs, (size_t)want * h->bf_cs, (size_t)h->bf_count * h->bf_cs);
    lk.shared();
    return rc;
}

int binflat_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int64_t xs, int k,
                                 float* d_distances, int64_t* d_labels) {
    if (!p) return fail(h, GAMMA_HIP_EINVAL, "null params");
    if (nq < 0) return fail(h, GAMMA_HIP_EINVAL, "nq < 0");
    if (!h->bf_init) return fail(h, GAMMA_HIP_EINVAL, "binflat not initialised");
    if (k > gh::kBinMaxK) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binflat: k > 4096 (the replay's heap lives in LDS)");
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    gh::FilterDesc filt;
    GH_TRY(build_filter(h, p, &filt, nullptr, 0));
    FiltCtx fc;
    GH_TRY(filt_ctx_single(h, filt, &fc));
    const int need_filter = (fc.any_clause || (h->d_bitmap && h->bitmap_any)) ? 1 : 0;
    hipStream_t s = h->stream;
    const int cs = h->bf_cs;
    const int64_t n = h->bf_count;   // published after its rows are in place (gamma_hip_binflat_append)
    const uint8_t* codes = h->d_bf_codes;
    if (n == 0) {   // nothing to scan: heap_heapify + heap_reorder of empty heaps
        StageScope t(h, GAMMA_HIP_STAGE_SELECT);
        gh::launch_binflat_replay(s, nullptr, nullptr, nullptr, nq, k, d_distances, d_labels, h->d_bf_stats);
        GH_CHECK(h, hipGetLastError());
        return GAMMA_HIP_OK;
    }
    const int64_t nch = (n + gh::kBinFlatChunk - 1) / gh::kBinFlatChunk;
    const int nb = cs * 8 + 1;
    // per query: its chunk histograms, then {bound, offset} per chunk, total and segment base
    const size_t hist_q = (size_t)nch * nb * sizeof(uint32_t);
    const size_t half = std::max<size_t>(h->dist_budget_bytes / 2, 1);
    const int qo = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)nq, (size_t)32768), half / hist_q));
    // (handle-owned: the upload of the segment bases may still be under way when a device-pointer call returns)
    std::vector<uint32_t>& tot = h->bf_tot_h;
    std::vector<int64_t>& base = h->bf_base_h;
    for (int q0 = 0; q0 < nq; q0 += qo) {
        const int nqs = std::min(qo, nq - q0);
        const uint8_t* xq = d_x + (int64_t)q0 * xs;
        GH_CHECK(h, h->w_bf_hist.ensure((size_t)nqs * hist_q));
        const size_t meta_off = ((size_t)nqs * nch * sizeof(int) + 15) & ~(size_t)15;
        const size_t tot_off = 2 * meta_off, base_off = tot_off + (((size_t)nqs * sizeof(uint32_t) + 15) & ~(size_t)15);
        GH_CHECK(h, h->w_bf_meta.ensure(base_off + (size_t)nqs * sizeof(int64_t)));
        char* meta = h->w_bf_meta.as<char>();
        int* d_bound = reinterpret_cast<int*>(meta);
        uint32_t* d_off = reinterpret_cast<uint32_t*>(meta + meta_off);
        uint32_t* d_tot = reinterpret_cast<uint32_t*>(meta + tot_off);
        int64_t* d_base = reinterpret_cast<int64_t*>(meta + base_off);
        {
            StageScope t(h, GAMMA_HIP_STAGE_COARSE);
            gh::launch_binflat_hist(s, xq, nqs, xs, codes, n, cs, fc.d_tab, need_filter, p->min_score, p->max_score,
                                    h->w_bf_hist.as<uint32_t>());
            gh::launch_binflat_bounds(s, h->w_bf_hist.as<uint32_t>(), nqs, n, cs, k, d_bound, d_off, d_tot);
        }
        GH_CHECK(h, hipGetLastError());
        // the candidate counts are data dependent (rows ordered from far to near make most rows candidates): the totals
        // come back, and the queries run in sub-batches whose candidates fit the workspace budget
        if (tot.size() < (size_t)nqs) {   // grows in the first round only (nqs <= qo), before anything reads it
            tot.resize((size_t)nqs);
            base.resize((size_t)nqs);
        }
        GH_CHECK(h, hipMemcpyAsync(tot.data(), d_tot, (size_t)nqs * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GH_CHECK(h, hipStreamSynchronize(s));
        const size_t cap_cand = std::max<size_t>(half / sizeof(uint2), 1);
        std::vector<int> cuts{0};   // sub-batch boundaries
        size_t acc = 0, most = 0;
        for (int q = 0; q < nqs; q++) {
            if (acc > 0 && acc + tot[q] > cap_cand) {
                cuts.push_back(q);
                acc = 0;
            }
            base[q] = (int64_t)acc;
            acc += tot[q];
            most = std::max(most, acc);
        }
        cuts.push_back(nqs);
        GH_CHECK(h, hipMemcpyAsync(d_base, base.data(), (size_t)nqs * sizeof(int64_t), hipMemcpyHostToDevice, s));
        GH_CHECK(h, h->w_bf_cand.ensure(most * sizeof(uint2)));
        for (size_t b = 0; b + 1 < cuts.size(); b++) {
            const int qa = cuts[b], nqb = cuts[b + 1] - qa;
            {
                StageScope t(h, GAMMA_HIP_STAGE_SCAN);
                gh::launch_binflat_collect(s, xq + (int64_t)qa * xs, nqb, xs, codes, n, cs, fc.d_tab, need_filter,
                                           p->min_score, p->max_score, d_bound + (int64_t)qa * nch, d_off + (int64_t)qa * nch,
                                           d_tot + qa, d_base + qa, h->w_bf_cand.as<uint2>());
            }
            {
                StageScope t(h, GAMMA_HIP_STAGE_SELECT);
                gh::launch_binflat_replay(s, h->w_bf_cand.as<uint2>(), d_base + qa, d_tot + qa, nqb, k,
                                          d_distances + (int64_t)(q0 + qa) * k, d_labels + (int64_t)(q0 + qa) * k,
                                          h->d_bf_stats);
            }
            GH_CHECK(h, hipGetLastError());
            h->bf_subbatches++;
        }
        // (the next round overwrites base only behind its own hipStreamSynchronize)
    }
    return GAMMA_HIP_OK;
}

}  // namespace

extern "C" {

int gamma_hip_binflat_chunk_rows(void) { return gh::kBinFlatChunk; }

int gamma_hip_binflat_init(gamma_hip_index* h, int nbits) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (nbits <= 0 || nbits % 8 != 0 || nbits / 8 > gh::kBinMaxCodeSize)
        return fail(h, GAMMA_HIP_EINVAL, "bad nbits (nbits % 8 == 0, at most 2048 bits)");
    // a handle of a float model (lists or raw rows of floats) has no binary codes
    if ((h->ivf_init && !h->binivf) || h->raw_d != 0)
        return fail(h, GAMMA_HIP_EINVAL, "binflat: the handle serves a float model");
    if (h->binivf && h->code_size != nbits / 8) return fail(h, GAMMA_HIP_EINVAL, "binflat: nbits differs from the binivf model's");
    if (h->bf_init) return h->bf_cs == nbits / 8 ? GAMMA_HIP_OK : fail(h, GAMMA_HIP_EINVAL, "binflat: initialised with another nbits");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipMalloc((void**)&h->d_bf_stats, 3 * sizeof(unsigned long long)));
    GH_CHECK(h, hipMemset(h->d_bf_stats, 0, 3 * sizeof(unsigned long long)));
    h->bf_cs = nbits / 8;
    h->bf_init = true;
    return GAMMA_HIP_OK;
}

int gamma_hip_binflat_append(gamma_hip_index* h, int64_t n, const uint8_t* codes) {
    if (!h || n < 0 || (n > 0 && !codes)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->bf_init) return fail(h, GAMMA_HIP_EINVAL, "binflat not initialised");
    if (n == 0) return GAMMA_HIP_OK;
    if (h->bf_count + n >= ((int64_t)1 << 31)) return fail(h, GAMMA_HIP_EUNSUPPORTED, "binflat: 2^31 rows or more");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(binflat_reserve(h, lk, h->bf_count + n));
    // the rows first, on the writer stream; the count a search reads is published behind them
    GH_CHECK(h, hipMemcpyAsync(h->d_bf_codes + (size_t)h->bf_count * h->bf_cs, codes, (size_t)n * h->bf_cs,
                               hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->bf_count += n;
    return GAMMA_HIP_OK;
}

int64_t gamma_hip_binflat_count(gamma_hip_index* h) {
    if (!h) return -1;
    std::lock_guard<std::mutex> g(h->mu);
    return h->bf_init ? h->bf_count : -1;
}

int gamma_hip_binflat_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* d_x, int k,
                                    float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    return binflat_search_device_locked(h, p, nq, d_x, h->bf_cs, k, d_distances, d_labels);
}

int gamma_hip_binflat_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const uint8_t* x, int k,
                             float* distances, int64_t* labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->bf_init) return fail(h, GAMMA_HIP_EINVAL, "binflat not initialised");
    if (nq > 0 && k > 0 && (!x || !distances || !labels)) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    if (nq <= 0 || k <= 0 || k > gh::kBinMaxK) return binflat_search_device_locked(h, p, nq, nullptr, 0, k, nullptr, nullptr);
    // rows padded to whole words: the shared staging path (pinned buffers, results stored in place) carries floats
    const int cs = h->bf_cs, rw = bin_row_words(cs);
    std::vector<float> rows((size_t)nq * rw, 0.f);
    for (int i = 0; i < nq; i++) memcpy(reinterpret_cast<char*>(rows.data() + (size_t)i * rw), x + (size_t)i * cs, cs);
    return host_search(h, nq, rw, rows.data(), k, distances, labels, [&](const float* dx, float* dd, int64_t* dl) {
        return binflat_search_device_locked(h, p, nq, reinterpret_cast<const uint8_t*>(dx), (int64_t)rw * 4, k, dd, dl);
    }, true, &lk);
}

// {queries searched, candidates collected, heap admissions of the replays, query sub-batches} since the last reset
int gamma_hip_binflat_stats(gamma_hip_index* h, int64_t* out4, int reset) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->bf_init) return fail(h, GAMMA_HIP_EINVAL, "binflat not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    unsigned long long v[3] = {0, 0, 0};
    GH_CHECK(h, hipMemcpyAsync(v, h->d_bf_stats, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) out4[i] = (int64_t)v[i];
    out4[3] = h->bf_subbatches;
    if (reset) {
        GH_CHECK(h, hipMemsetAsync(h->d_bf_stats, 0, sizeof(v), h->stream));
        GH_CHECK(h, hipStreamSynchronize(h->stream));
        h->bf_subbatches = 0;
    }
    return GAMMA_HIP_OK;
}

}  // extern "C"
