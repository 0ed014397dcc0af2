// gamma_hip_store.cpp -- the writers of libgamma_hip.so: the realtime inverted-list arena (growth law, repack,
// versioned (offset, length) tables), training state, Add / Update / Delete / compaction, device-side encoding, the raw
// vector store, scalar columns and the delete bitmap.  C ABI: include/gamma_hip.h.
#include "binivf.h"
#include "gamma_hip_internal.h"
#include "opq.h"
#include "pq4.h"

namespace ghi {

// ---- arena ---------------------------------------------------------------------------
// (every array of this file that grows does so through DevArray::grow, dev_mem.h; the growth laws are here)
static const size_t kArenaChunk = (size_t)8 << 20;   // mapped in chunks of at least 8 MB
// the readers' pointers and the capacity are the current set's
static void arena_adopt(H* h) { h->arena.adopt(&h->d_codes, &h->d_ids, &h->d_sums, &h->arena_cap); }

int arena_reserve(H* h, int64_t need_entries) {
    const int64_t need = h->arena_used + need_entries;
    if (need <= h->arena_cap) return GAMMA_HIP_OK;
    DevColumns& cur = h->arena.cur;
    if (!h->d_codes && h->arena_cap == 0) {
        // the first reservation of an index: mapped ranges when the runtime offers them AND the first chunks map (a failure
        // leaves the reallocating arena, nothing behind)
        cur.shape((size_t)h->code_size, sizeof(int64_t), h->keep_sums ? sizeof(float) : 0);
        if (!getenv("GAMMA_HIP_NO_ARENA_VMM") && cur.start_mapped(h->device, kArenaChunk, need)) {
            arena_adopt(h);
            return GAMMA_HIP_OK;
        }
    }
    // mapped: more physical memory behind the arrays in place -- nothing moves, the searches in flight go on.  Otherwise the
    // arrays move, under the exclusive lock.
    int64_t ncap = std::max<int64_t>(h->arena_cap * 2, need);
    ncap += ncap / 8;
    const bool moves = !cur.mapped();
    const char* what = "";
    const hipError_t e = cur.grow(need, ncap, h->arena_used, h->wstream, writer_exclusive(h), &what);
    arena_adopt(h);   // (also after a failure: a column that did move is read through its new pointer)
    if (moves && e == hipSuccess) h->arena_regrows++;   // as DevArray::regrows: the moves that happened
    return e == hipSuccess ? GAMMA_HIP_OK : grow_fail(h, "arena growth", e, what);
}

// sums of arena entries [pos, pos + n) of list l, behind the copy of their codes on the writer stream
static int sums_range(H* h, int l, int64_t pos, int n) {
    if (!h->d_sums || !h->trained || n <= 0) return GAMMA_HIP_OK;
    gh::launch_code_sums_one(h->wstream, h->d_T2, h->d_codes, h->code_size, l, pos, n, h->d_sums);
    return GAMMA_HIP_OK;
}
// every list at its current extent (after a repack, a compaction, a new table): the device tables of the current
// version must be the host mirror's (publish_meta before)
static int sums_all_lists(H* h) {
    if (!h->d_sums || !h->trained) return GAMMA_HIP_OK;
    gh::launch_code_sums_lists(h->wstream, h->d_T2, h->d_codes, h->code_size, h->d_list_off, h->d_list_len, h->nlist,
                               std::max(1, h->max_list_len), h->d_sums);
    return GAMMA_HIP_OK;
}

// The reference frees a bucket's old memory after a grow / compact swap (delayed by 1 s,
// realtime_mem_data.cc:457-466).  Here grown and compacted extents are abandoned inside the arena
// (arena_waste); once they are more than half of what is in use -- and worth at least a megabyte of codes --
// every list moves into a fresh, tight arena: one kernel, offsets re-published in stream order.
// Safe by construction (round 5): the version of the list tables that points at the new extents is published only after
// the target has been READ BACK through its new mapping and found equal to the source -- per-list checksums of ids + codes
// (k_list_checksum) taken at the source before the move and at the target in a launch of its own, behind a translation
// fence (the stale-translation failure seen on this runtime lets a kernel read back what it wrote itself; a later launch
// over fresh translations is what a search would see).  A mismatch keeps the old version (nothing has been freed), retires
// the target's address ranges, counts (gamma_hip_ivfpq_repack_verify_stats, logged by the plugins) and repeats the move
// into ordinary hipMalloc'd arrays -- the handle's arena then stays outside virtual memory management.  The fence after
// every unmap stays as belt and braces.
static int repack_checksums(H* h, const uint8_t* codes, const int64_t* ids, const int64_t* d_off, std::vector<unsigned long long>* out) {
    GH_CHECK(h, h->we_chk.ensure((size_t)h->nlist * sizeof(unsigned long long)));
    gh::launch_list_checksum(h->wstream, codes, ids, d_off, h->d_list_len, h->nlist, h->code_size, std::max(1, h->max_list_len),
                             h->we_chk.as<unsigned long long>());
    out->resize(h->nlist);
    GH_CHECK(h, hipMemcpyAsync(out->data(), h->we_chk.p, (size_t)h->nlist * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

// one attempt: GAMMA_HIP_OK = moved, verified, committed; kRepackMismatch = the target did not read back as written (old
// version intact, target given back / retired); anything else = error (old version intact)
static const int kRepackMismatch = 1;
static int arena_repack_once(H* h, bool vmm, const std::vector<int64_t>& noff, int64_t total, int64_t ncap,
                             const std::vector<unsigned long long>& src_sum) {
    // The handle keeps TWO column sets and the repack moves the lists from the set in use into the other one -- physical chunks
    // mapped into its ranges for the occasion, or plain allocations -- gives the old set's memory back and swaps the roles.
    DevColumns& alt = h->arena.alt;
    struct TargetGuard {   // an error below gives the target set's memory back
        H* h;
        bool armed = true;
        ~TargetGuard() {
            if (armed) h->arena.alt.clear(&h->arena.retired);
        }
    } guard{h};
    alt.shape((size_t)h->code_size, sizeof(int64_t), h->keep_sums ? sizeof(float) : 0);
    const char* what = "";
    const hipError_t te = vmm ? alt.map_target(h->device, kArenaChunk, ncap, &h->arena.retired, &what)
                              : alt.alloc_target(ncap, h->wstream, writer_exclusive(h), &h->arena.retired, &what);
    if (te != hipSuccess) return grow_fail(h, "arena repack", te, what);
    uint8_t* nc = alt.col[0].as<uint8_t>();
    int64_t* ni = alt.col[1].as<int64_t>();
    GH_CHECK(h, h->we_stage.ensure((size_t)h->nlist * sizeof(int64_t)));
    GH_CHECK(h, hipMemcpyAsync(h->we_stage.p, noff.data(), (size_t)h->nlist * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
    gh::launch_repack_lists(h->wstream, h->d_codes, h->d_ids, nc, ni, h->d_list_off, h->we_stage.as<int64_t>(),
                            h->d_list_len, h->nlist, h->code_size, h->max_list_len);
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    static const bool no_verify = getenv("GAMMA_HIP_NO_REPACK_VERIFY") != nullptr;
    if (!no_verify) {
        if (vmm) (void)vm_unmap_fence();   // translations the move may have cached are gone before the read-back
        // fault injection for the tests (GAMMA_HIP_FAULT_REPACK=<n>: the first n read-backs see a zeroed entry)
        static std::atomic<int> fault_left{getenv("GAMMA_HIP_FAULT_REPACK") ? atoi(getenv("GAMMA_HIP_FAULT_REPACK")) : 0};
        if (total > 0 && fault_left.load() > 0 && fault_left.fetch_sub(1) > 0) {
            int l0 = 0;
            while (l0 < h->nlist - 1 && h->h_list_len[l0] == 0) l0++;
            GH_CHECK(h, hipMemsetAsync(ni + noff[l0], 0, sizeof(int64_t), h->wstream));
            GH_CHECK(h, hipMemsetAsync(nc + noff[l0] * h->code_size, 0xa5, (size_t)h->code_size, h->wstream));
        }
        std::vector<unsigned long long> dst_sum;
        GH_TRY(repack_checksums(h, nc, ni, h->we_stage.as<int64_t>(), &dst_sum));
        h->repack_verified++;
        if (dst_sum != src_sum) {
            h->repack_verify_failures++;
            alt.taint();   // the guard unmaps a mapped target (with its fence); its addresses are never mapped again
            return kRepackMismatch;
        }
    }
    // the target set is the arena from here; the old set's memory goes back (a set that leaves virtual memory management
    // after a failed read-back keeps its ranges reserved, unmapped)
    guard.armed = false;
    h->arena.swap_sets();
    h->arena.alt.clear(&h->arena.retired);
    arena_adopt(h);
    h->arena_used = total;
    h->arena_waste = 0;
    h->h_list_off = noff;
    h->n_repacks++;
    GH_TRY(publish_meta(h));
    return sums_all_lists(h);   // the sums follow their codes: recomputed at the new offsets (the caller drains the stream)
}

int arena_repack(H* h) {
    int64_t total = 0;
    std::vector<int64_t> noff(h->nlist);
    for (int l = 0; l < h->nlist; l++) {
        noff[l] = total;
        total += h->h_list_cap[l];
    }
    const int64_t ncap = total + total / 8 + 1024;
    if (h->wl) GH_CHECK(h, h->wl->exclusive());   // every list moves and the old arrays are freed
    GH_TRY(publish_meta(h));                      // the device tables the kernels below read = the host mirror
    std::vector<unsigned long long> src_sum;
    GH_TRY(repack_checksums(h, h->d_codes, h->d_ids, h->d_list_off, &src_sum));
    int rc = arena_repack_once(h, h->arena_vmm(), noff, total, ncap, src_sum);
    if (rc == kRepackMismatch && h->arena_vmm()) rc = arena_repack_once(h, false, noff, total, ncap, src_sum);
    if (rc == kRepackMismatch)
        return fail(h, GAMMA_HIP_EDEVICE, "arena repack: the moved lists did not read back as written (the previous arena stays in use)");
    return rc;
}
int arena_repack_if_need(H* h) {
    const int64_t min_waste = std::max<int64_t>(h->repack_min_entries, 1);
    if (h->arena_waste < min_waste || h->arena_waste * 2 < h->arena_used) return GAMMA_HIP_OK;
    return arena_repack(h);
}

// RealTimeMemData::ExtendBucketIfNeed + RTInvertBucketData::ExtendBucketMem
// (realtime_mem_data.cc:383-421,152-188): same growth law, region moved inside the arena.
int list_ensure(H* h, int l, int add) {
    const int len = h->h_list_len[l], cap = h->h_list_cap[l];
    if ((int64_t)len + add <= cap) return GAMMA_HIP_OK;
    if ((int64_t)cap * 2 >= h->bucket_max) return fail(h, GAMMA_HIP_EFULL, "exceed the max bucket keys");
    const int least = len + add;
    // the growth step is worked out on a copy of the list's extend counter and committed only once the arena holds
    // the new extent (a failed reservation leaves the list as it was)
    uint8_t et = h->h_extend_time[l];
    double coef = extend_coefficient(++et);
    int ext = (int)(cap * coef);
    while (ext < least) {
        coef = extend_coefficient(++et);
        ext = (int)(ext * coef);
    }
    GH_TRY(arena_reserve(h, ext));
    h->h_extend_time[l] = et;
    const int64_t noff = h->arena_used;
    if (len > 0) {
        GH_CHECK(h, hipMemcpyAsync(h->d_codes + noff * h->code_size,
                                   h->d_codes + h->h_list_off[l] * h->code_size,
                                   (size_t)len * h->code_size, hipMemcpyDeviceToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(h->d_ids + noff, h->d_ids + h->h_list_off[l],
                                   (size_t)len * sizeof(int64_t), hipMemcpyDeviceToDevice, h->wstream));
        if (h->d_sums)
            GH_CHECK(h, hipMemcpyAsync(h->d_sums + noff, h->d_sums + h->h_list_off[l], (size_t)len * sizeof(float),
                                       hipMemcpyDeviceToDevice, h->wstream));
    }
    h->arena_waste += cap;
    h->arena_used += ext;
    h->h_list_off[l] = noff;   // the old extent stays intact: searches in flight read it through their version
    h->h_list_cap[l] = ext;
    return GAMMA_HIP_OK;
}

int add_keys_locked(H* h, int l, int n, const int64_t* vids, const uint8_t* codes) {
    if (l < 0 || l >= h->nlist || n < 0) return fail(h, GAMMA_HIP_EINVAL, "bad list_no");
    if (n == 0) return GAMMA_HIP_OK;
    GH_TRY(list_ensure(h, l, n));
    const int64_t pos = h->h_list_off[l] + h->h_list_len[l];
    GH_CHECK(h, hipMemcpyAsync(h->d_ids + pos, vids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice,
                               h->wstream));
    GH_CHECK(h, hipMemcpyAsync(h->d_codes + pos * h->code_size, codes, (size_t)n * h->code_size,
                               hipMemcpyHostToDevice, h->wstream));
    GH_TRY(sums_range(h, l, pos, n));
    for (int i = 0; i < n; i++) {
        const int64_t v = vids[i];
        if (v < 0) {   // superseded slot restored from a dump (ReadInvertedLists, gamma_index_io.cc:186-189)
            h->h_deleted[l]++;
            h->n_moved++;
            continue;
        }
        if ((size_t)v >= h->vid_pos.size()) h->vid_pos.resize(std::max<size_t>(h->vid_pos.size() * 2, v + 1), -1);
        h->vid_pos[v] = ((int64_t)l << 32) | (int64_t)(h->h_list_len[l] + i);
        if (h->doc_deleted(v)) h->h_deleted[l]++;  // realtime_mem_data.cc:293-296
    }
    h->h_list_len[l] += n;  // publish after the copies (realtime_mem_data.cc:299-300)
    h->ntotal += n;
    GH_TRY(publish_meta(h));
    // the host buffers may be reused by the caller as soon as we return
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return arena_repack_if_need(h);
}
// Spatial order of the coarse centroids by recursive principal-axis bisection: split the set at
// the median of its projection on the dominant direction (a few power iterations), recurse.
// Neighbouring ranks = neighbouring centroids.  Used only to order queries for cache locality.
void centroid_order_rec(const float* cc, int d, std::vector<int>& idx, int lo, int hi, std::vector<float>& proj,
                        std::vector<double>& mean, std::vector<double>& dir, std::vector<double>& tmp) {
    const int n = hi - lo;
    if (n <= 2) return;
    for (int t = 0; t < d; t++) mean[t] = 0;
    for (int i = lo; i < hi; i++) {
        const float* c = cc + (size_t)idx[i] * d;
        for (int t = 0; t < d; t++) mean[t] += c[t];
    }
    for (int t = 0; t < d; t++) mean[t] /= n;
    // start from the direction to the point farthest from the mean (never orthogonal to the data)
    double best = -1;
    int far = lo;
    for (int i = lo; i < hi; i++) {
        const float* c = cc + (size_t)idx[i] * d;
        double s = 0;
        for (int t = 0; t < d; t++) s += (c[t] - mean[t]) * (c[t] - mean[t]);
        if (s > best) { best = s; far = i; }
    }
    for (int t = 0; t < d; t++) dir[t] = cc[(size_t)idx[far] * d + t] - mean[t];
    for (int it = 0; it < 6; it++) {
        for (int t = 0; t < d; t++) tmp[t] = 0;
        for (int i = lo; i < hi; i++) {
            const float* c = cc + (size_t)idx[i] * d;
            double pr = 0;
            for (int t = 0; t < d; t++) pr += (c[t] - mean[t]) * dir[t];
            for (int t = 0; t < d; t++) tmp[t] += pr * (c[t] - mean[t]);
        }
        double nrm = 0;
        for (int t = 0; t < d; t++) nrm += tmp[t] * tmp[t];
        if (nrm <= 0) break;
        nrm = std::sqrt(nrm);
        for (int t = 0; t < d; t++) dir[t] = tmp[t] / nrm;
    }
    for (int i = lo; i < hi; i++) {
        const float* c = cc + (size_t)idx[i] * d;
        double pr = 0;
        for (int t = 0; t < d; t++) pr += (c[t] - mean[t]) * dir[t];
        proj[idx[i]] = (float)pr;
    }
    const int mid = lo + n / 2;
    std::nth_element(idx.begin() + lo, idx.begin() + mid, idx.begin() + hi,
                     [&](int a, int b) { return proj[a] < proj[b] || (proj[a] == proj[b] && a < b); });
    centroid_order_rec(cc, d, idx, lo, mid, proj, mean, dir, tmp);
    centroid_order_rec(cc, d, idx, mid, hi, proj, mean, dir, tmp);
}

std::vector<int> centroid_rank(const float* cc, int nlist, int d) {
    std::vector<int> idx(nlist), rank(nlist);
    for (int i = 0; i < nlist; i++) idx[i] = i;
    std::vector<float> proj(nlist);
    std::vector<double> mean(d), dir(d), tmp(d);
    centroid_order_rec(cc, d, idx, 0, nlist, proj, mean, dir, tmp);
    for (int i = 0; i < nlist; i++) rank[idx[i]] = i;
    return rank;
}

// ---- the re-rank filter's image of a dense fp32 store (rerank_filter.hip; the handle's rf) ------------------------------------
// its arrays hold `need` rows: a geometric reallocation that carries the image of the rows present (DevArray::grow)
int rerank_image_reserve(H* h, int64_t need) {
    const size_t d = (size_t)h->raw_d, ax = 2 * sizeof(float);
    const int64_t cap = h->rf.cap_rows(h->raw_d);
    if (need <= cap) return GAMMA_HIP_OK;
    const int64_t ncap = std::max<int64_t>(std::max<int64_t>(need, cap + cap / 2), 1024);
    const size_t keep = h->rf.on ? (size_t)h->nraw : 0;   // (a new image: nothing to carry)
    GH_TRY(grow_array(h, "re-rank image", h->rf.rows, (size_t)need * d, (size_t)ncap * d, keep * d));
    return grow_array(h, "re-rank image", h->rf.aux, (size_t)need * ax, (size_t)ncap * ax, keep * ax);
}

}  // namespace ghi

using namespace ghi;

extern "C" {


int gamma_hip_field_append(gamma_hip_index* h, int field_id, int dtype, int64_t n, const void* values) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (dtype < GAMMA_HIP_FIELD_INT || dtype > GAMMA_HIP_FIELD_DOUBLE || n < 0 || (n > 0 && !values))
        return fail(h, GAMMA_HIP_EINVAL, "bad column append");
    GH_CHECK(h, hipSetDevice(h->device));
    auto& c = h->fields[field_id];
    if (c.n == 0 && c.d.cap == 0) c.dtype = dtype;
    if (c.dtype != dtype) return fail(h, GAMMA_HIP_EINVAL, "column dtype mismatch");
    const size_t es = field_elem_size(dtype);
    const int64_t ncap = std::max<int64_t>(c.n + n, std::max<int64_t>(1 << 16, (int64_t)(c.d.cap / es) * 2));
    GH_TRY(grow_array(h, "column", c.d, (size_t)(c.n + n) * es, (size_t)ncap * es, (size_t)c.n * es));
    if (n) {
        GH_CHECK(h, hipMemcpyAsync(c.d + (size_t)c.n * es, values, (size_t)n * es, hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
    }
    c.n += n;
    return GAMMA_HIP_OK;
}

int gamma_hip_field_update(gamma_hip_index* h, int field_id, int64_t docid, const void* value) {
    if (!h || !value) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    auto it = h->fields.find(field_id);
    if (it == h->fields.end() || docid < 0 || docid >= it->second.n) return fail(h, GAMMA_HIP_EINVAL, "bad column update");
    GH_CHECK(h, hipSetDevice(h->device));
    const size_t es = field_elem_size(it->second.dtype);
    GH_CHECK(h, hipMemcpyAsync(it->second.d + (size_t)docid * es, value, es, hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

int gamma_hip_vid2docid_append(gamma_hip_index* h, int64_t n, const int32_t* docids) {
    if (!h || n < 0 || (n > 0 && !docids)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    const int64_t have = (int64_t)h->h_v2d.size();
    const int64_t ncap = std::max<int64_t>(have + n, std::max<int64_t>(1 << 16, (int64_t)(h->d_v2d.cap / sizeof(int32_t)) * 2));
    GH_TRY(grow_array(h, "vid2docid", h->d_v2d, (size_t)(have + n) * sizeof(int32_t), (size_t)ncap * sizeof(int32_t), (size_t)have * sizeof(int32_t)));
    if (n) {
        GH_CHECK(h, hipMemcpyAsync(h->d_v2d + have, docids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        h->h_v2d.insert(h->h_v2d.end(), docids, docids + n);   // published last: searches enqueued before see the shorter map
    }
    return GAMMA_HIP_OK;
}

int64_t gamma_hip_vid2docid_count(gamma_hip_index* h) {
    if (!h) return -1;
    std::lock_guard<std::mutex> g(h->mu);
    return (int64_t)h->h_v2d.size();
}

int64_t gamma_hip_field_count(gamma_hip_index* h, int field_id) {
    if (!h) return -1;
    std::lock_guard<std::mutex> g(h->mu);
    auto it = h->fields.find(field_id);
    return it == h->fields.end() ? 0 : it->second.n;
}

// A STRING column on the device: doc i = items tok[start .. start + len), its row word = start << 16 | len.  One 8-byte
// word per doc (not CSR offsets) so that a doc's items can be REWRITTEN: the new items go in place when they fit, else
// to the end of the item array, and the row word -- a single aligned store -- switches the doc over.
static int term_reserve(gamma_hip_index* h, gamma_hip_index::TermColumn& c, int64_t add_docs, int64_t add_tok) {
    const int64_t cap_docs = (int64_t)(c.d_off.cap / sizeof(int64_t)), cap_tok = (int64_t)(c.d_tok.cap / sizeof(int32_t));
    if (c.ndocs + add_docs <= cap_docs && c.ntok + add_tok <= cap_tok && c.d_off) return GAMMA_HIP_OK;
    // both arrays move whenever either is short (so each is asked for its new capacity, not for what it needs)
    const size_t nd = (size_t)std::max<int64_t>(c.ndocs + add_docs, std::max<int64_t>(1 << 16, cap_docs * 2)) * sizeof(int64_t);
    const size_t nt = (size_t)std::max<int64_t>(c.ntok + add_tok, std::max<int64_t>(1 << 16, cap_tok * 2)) * sizeof(int32_t);
    GH_TRY(grow_array(h, "term column", c.d_off, nd, nd, (size_t)c.ndocs * sizeof(int64_t)));
    return grow_array(h, "term column", c.d_tok, nt, nt, (size_t)c.ntok * sizeof(int32_t));
}

int gamma_hip_term_append(gamma_hip_index* h, int field_id, int64_t n_docs, const int32_t* counts,
                          const int32_t* items) {
    if (!h || n_docs < 0 || (n_docs > 0 && !counts)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    auto& c = h->terms[field_id];
    int64_t add_tok = 0;
    for (int64_t i = 0; i < n_docs; i++) {
        if (counts[i] < 0 || counts[i] > 65535) return fail(h, GAMMA_HIP_EINVAL, "item count out of range");
        add_tok += counts[i];
    }
    if (add_tok > 0 && !items) return fail(h, GAMMA_HIP_EINVAL, "null items");
    GH_TRY(term_reserve(h, c, n_docs, add_tok));
    if (n_docs > 0) {
        std::vector<int64_t> rows(n_docs);
        int64_t run = c.ntok;
        for (int64_t i = 0; i < n_docs; i++) {
            rows[i] = (run << 16) | (int64_t)counts[i];
            run += counts[i];
        }
        if (add_tok) GH_CHECK(h, hipMemcpyAsync(c.d_tok + c.ntok, items, (size_t)add_tok * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(c.d_off + c.ndocs, rows.data(), (size_t)n_docs * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        c.h_rows.insert(c.h_rows.end(), rows.begin(), rows.end());
        c.ntok += add_tok;
        c.ndocs += n_docs;   // published last: a search enqueued before sees the shorter column
    }
    return GAMMA_HIP_OK;
}

// a doc's items rewritten (the doc's STRING field was updated in the table)
int gamma_hip_term_update(gamma_hip_index* h, int field_id, int64_t docid, int32_t count, const int32_t* items) {
    if (!h || count < 0 || count > 65535 || (count > 0 && !items)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    auto it = h->terms.find(field_id);
    if (it == h->terms.end() || docid < 0 || docid >= it->second.ndocs) return fail(h, GAMMA_HIP_EINVAL, "term update: unknown field / doc");
    auto& c = it->second;
    const int64_t old = c.h_rows[docid];
    int64_t start = old >> 16;
    if (count > (int32_t)(old & 0xffff)) {   // does not fit in place: the new items go to the end of the item array
        GH_TRY(term_reserve(h, c, 0, count));
        start = c.ntok;
        c.ntok += count;
    }
    const int64_t row = (start << 16) | (int64_t)count;
    if (count) GH_CHECK(h, hipMemcpyAsync(c.d_tok + start, items, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipMemcpyAsync(c.d_off + docid, &row, sizeof(row), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    c.h_rows[docid] = row;
    return GAMMA_HIP_OK;
}

int64_t gamma_hip_term_count(gamma_hip_index* h, int field_id) {
    if (!h) return -1;
    std::lock_guard<std::mutex> g(h->mu);
    auto it = h->terms.find(field_id);
    return it == h->terms.end() ? 0 : it->second.ndocs;
}

// what a narrow store answers to the entry points of the sparse fp32 store (gamma_hip_raw_put, _drop)
static const char* narrow_store_name(const H* h) {
    switch (h->raw_et) {
        case gh::ROW_F16: return "the raw store holds float16 rows (gamma_hip_raw_init_f16)";
        case gh::ROW_SQ8: return "the raw store holds scalar-quantised sq8 rows (gamma_hip_raw_init_sq8)";
        default: return "the raw store holds 8-bit rows (gamma_hip_raw_init_i8)";
    }
}

// et: gh::RowType (0 fp32, 1 float16, 2 uint8, 3 int8, 4 sq8: gamma_hip_raw_elem_type)
static int raw_init_as(gamma_hip_index* h, int d, int et) {
    if (!h || d <= 0) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_d != 0 && h->raw_d != d) return fail(h, GAMMA_HIP_EINVAL, "raw store dimension mismatch");
    if (h->raw_d != 0 && h->raw_elem_type() != et) return fail(h, GAMMA_HIP_EINVAL, "the raw store's element type is fixed at its first init");
    h->raw_et = et;
    if (h->raw_d == 0 && !getenv("GAMMA_HIP_NO_RAW_VMM")) {
        // reserve the address range the store may ever need (the device's memory): physical chunks are mapped into it
        // as rows arrive (raw_reserve).  Any failure -- here or of the FIRST chunk -- leaves the reallocating store.
        GH_CHECK(h, hipSetDevice(h->device));
        (void)h->raw.reserve(h->device, (size_t)64 << 20);   // chunks of whole 64 MB
    }
    h->raw_d = d;
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_init(gamma_hip_index* h, int d) { return raw_init_as(h, d, 0); }
int gamma_hip_raw_init_f16(gamma_hip_index* h, int d) { return raw_init_as(h, d, 1); }
int gamma_hip_raw_init_i8(gamma_hip_index* h, int d, int is_signed) { return raw_init_as(h, d, is_signed ? 3 : 2); }
int gamma_hip_raw_init_sq8(gamma_hip_index* h, int d) { return raw_init_as(h, d, 4); }
int gamma_hip_raw_elem_type(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    return h->raw_elem_type();
}
int gamma_hip_raw_elem_bytes(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    return h->raw_d > 0 ? (int)h->raw_esz() : 0;
}

// the store holds `need` rows afterwards: chunks mapped behind the rows in place, or a geometric reallocation (a mapped
// store whose first chunk fails gives its range back and reallocates from then on: DevArray::grow)
static int raw_reserve(H* h, int64_t need) {
    const size_t row = (size_t)h->raw_d * h->raw_esz();
    const int64_t cap = h->raw_cap();
    const int64_t ncap = std::max<int64_t>(std::max<int64_t>(need, cap + cap / 2), 1024);
    GH_TRY(grow_array(h, "raw store", h->raw, (size_t)need * row, (size_t)ncap * row, (size_t)h->nraw * row));
    return h->rf.on ? rerank_image_reserve(h, need) : GAMMA_HIP_OK;   // the image grows with its store
}

// ---- the re-rank filter's image of a dense fp32 store (rerank_filter.hip; the handle's rf; its growth: rerank_image_reserve) ----
// what a dense writer does behind its row copies, on the writer stream: the image rows of store rows first, first + 1, ..
// (d_vids == nullptr) or d_vids[i] (device memory), so that an image row is in place whenever its row is
static int raw_image_rows_in(H* h, int64_t first, const int64_t* d_vids, int64_t n, int64_t nrows) {
    if (!h->rf.on) return GAMMA_HIP_OK;
    GH_CHECK(h, hipStreamWaitEvent(h->wstream, h->rf.built, 0));   // the parameters come from the search stream
    gh::launch_rerank_image_rows(h->wstream, h->raw_f32(), d_vids, first, n, h->raw_d, h->rf.par, h->rf.rows.as<uint8_t>(),
                                 h->rf.aux.as<float>(), std::min(nrows, h->rf.cap_rows(h->raw_d)));
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

// ---- float16 store: what the writers do instead of their copy --------------------------------------------------------
// A finite fp32 value that rounds to an infinite half (|x| >= 65520: the midpoint of 65504 and 2^16 rounds to even = up) is an
// error of the caller's, found before anything of the store changes.  NaN and +-inf pass: they are stored as they convert.
static inline float half_bits_to_float(uint16_t b) {
    const uint32_t sign = (uint32_t)(b & 0x8000u) << 16, e = (b >> 10) & 0x1fu, m = b & 0x3ffu;
    uint32_t u;
    if (e == 0x1fu) u = sign | 0x7f800000u | (m << 13);                       // inf, NaN (payload kept)
    else if (e != 0) u = sign | ((e + 112u) << 23) | (m << 13);               // normal
    else if (m == 0) u = sign;                                                // zero
    else {                                                                    // subnormal half = m * 2^-24: a normal float
        int s = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; s++; }
        u = sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

static int half_values_check(H* h, int64_t count, const float* v) {
    for (int64_t i = 0; i < count; i++) {
        const float a = fabsf(v[i]);
        if (a >= 65520.f && a != INFINITY)
            return fail(h, GAMMA_HIP_EINVAL, "raw store (float16): a finite value is outside binary16's range (|x| >= 65520); nothing was written");
    }
    return GAMMA_HIP_OK;
}

// ---- byte store (gamma_hip_raw_init_i8): lossless or refused ----------------------------------------------------------
// A value is storable when it is finite, integral and inside the element type's range: exactly when float(T(x)) == x (-0.0
// compares equal to 0 and is stored as 0).  The comparisons are false for NaN; +-inf and the fractions fail them or the trunc.
int gamma_hip_raw_i8_check(const float* x, int64_t n, int is_signed, int64_t* first_bad) {
    if (n < 0 || (n > 0 && !x)) return GAMMA_HIP_EINVAL;
    const float lo = is_signed ? -128.f : 0.f, hi = is_signed ? 127.f : 255.f;
    for (int64_t i = 0; i < n; i++) {
        const float v = x[i];
        if (!(v >= lo && v <= hi && v == truncf(v))) {
            if (first_bad) *first_bad = i;
            return GAMMA_HIP_EINVAL;
        }
    }
    return GAMMA_HIP_OK;
}

// the writers' check in front of their reservation: base = the position of v[0] in the caller's array (for the message)
static int byte_values_check(H* h, int64_t count, const float* v, int64_t base = 0) {
    int64_t bad = -1;
    if (gamma_hip_raw_i8_check(v, count, h->raw_et == gh::ROW_I8, &bad) == GAMMA_HIP_OK) return GAMMA_HIP_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "raw store (%s, gamma_hip_raw_init_i8): value %g at position %lld (row %lld, element %lld) is not exactly storable; nothing was written",
             h->raw_et == gh::ROW_I8 ? "int8" : "uint8", (double)v[bad], (long long)(base + bad), (long long)((base + bad) / h->raw_d),
             (long long)((base + bad) % h->raw_d));
    return fail(h, GAMMA_HIP_EINVAL, msg);
}
// ---- scalar-quantised store (gamma_hip_raw_init_sq8): lossy, float data ------------------------------------------------
// the acceptance predicate: every value is finite (-0.0 and values far outside the ranges are: the encoder clips)
int gamma_hip_raw_sq8_check(const float* x, int64_t n, int64_t* first_bad) {
    if (n < 0 || (n > 0 && !x)) return GAMMA_HIP_EINVAL;
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(x[i])) {
            if (first_bad) *first_bad = i;
            return GAMMA_HIP_EINVAL;
        }
    return GAMMA_HIP_OK;
}

// step = span / 255 and inv = 255 / span of every dimension, one fp32 operation each (this file is built with
// -ffp-contract=off and the three operations cannot fuse anyway); span == 0 or an infinite inv: a constant dimension
int gamma_hip_raw_sq8_params(int d, const float* vmin, const float* vmax, float* step_out, float* inv_out) {
    if (d <= 0 || !vmin || !vmax) return GAMMA_HIP_EINVAL;
    for (int j = 0; j < d; j++) {
        if (!std::isfinite(vmin[j]) || !std::isfinite(vmax[j]) || vmin[j] > vmax[j]) return GAMMA_HIP_EINVAL;
        const float span = vmax[j] - vmin[j];
        if (!std::isfinite(span)) return GAMMA_HIP_EINVAL;
    }
    for (int j = 0; j < d; j++) {
        const float span = vmax[j] - vmin[j];
        float step = span / 255.0f;
        float inv = 255.0f / span;
        if (span == 0.0f || !std::isfinite(inv)) step = inv = 0.0f;
        if (step_out) step_out[j] = step;
        if (inv_out) inv_out[j] = inv;
    }
    return GAMMA_HIP_OK;
}

// the ranges and both tables of an empty sq8 store (caller holds the write lock)
static int sq8_set_ranges_locked(H* h, const float* vmin, const float* vmax) {
    if (h->raw_et != gh::ROW_SQ8) return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_set_ranges: the raw store is not an sq8 store (gamma_hip_raw_init_sq8)");
    if (h->nraw > 0) return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_set_ranges: the sq8 raw store holds rows; the ranges change only while it is empty (after gamma_hip_raw_clear)");
    // (members of a group are compared once, when their stores take the sparse form: the ranges are fixed from then on)
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_set_ranges: the sq8 raw store has taken its sparse form (gamma_hip_raw_put); the ranges change only before that (after gamma_hip_raw_clear)");
    const int d = h->raw_d;
    std::vector<float> step(d), inv(d);
    if (gamma_hip_raw_sq8_params(d, vmin, vmax, step.data(), inv.data()) != GAMMA_HIP_OK)
        return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_set_ranges: every range needs finite bounds, vmin <= vmax and a finite span");
    std::vector<float> tab((size_t)d * 4);
    for (int j = 0; j < d; j++) {
        tab[2 * j] = step[j];
        tab[2 * j + 1] = vmin[j];
        tab[2 * d + 2 * j] = inv[j];
        tab[2 * d + 2 * j + 1] = vmin[j];
    }
    GH_CHECK(h, hipSetDevice(h->device));
    if (!h->d_sq8_tab) GH_CHECK(h, hipMalloc((void**)&h->d_sq8_tab, tab.size() * sizeof(float)));
    // (the store is empty: no search in flight decodes a row)
    GH_CHECK(h, hipMemcpyAsync(h->d_sq8_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->sq8_vmin.assign(vmin, vmin + d);
    h->sq8_vmax.assign(vmax, vmax + d);
    h->sq8_step.swap(step);
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_sq8_set_ranges(gamma_hip_index* h, const float* vmin, const float* vmax) {
    if (!h || !vmin || !vmax) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    return sq8_set_ranges_locked(h, vmin, vmax);
}

int gamma_hip_raw_sq8_get_ranges(gamma_hip_index* h, float* vmin, float* vmax) {
    if (!h || !vmin || !vmax) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->raw_et != gh::ROW_SQ8 || h->sq8_vmin.empty()) {
        h->err = "gamma_hip_raw_sq8_get_ranges: no ranges (an sq8 store after gamma_hip_raw_sq8_set_ranges / _train has them)";
        return GAMMA_HIP_EINVAL;
    }
    memcpy(vmin, h->sq8_vmin.data(), h->sq8_vmin.size() * sizeof(float));
    memcpy(vmax, h->sq8_vmax.data(), h->sq8_vmax.size() * sizeof(float));
    return GAMMA_HIP_OK;
}

static int sq8_values_check(H* h, int64_t count, const float* v, int64_t base = 0);

// per-dimension minimum and maximum of n host rows: staged through the writer's staging buffer in 64 MB pieces, every piece
// folded into the running result by k_sq8_minmax on the writer stream
int gamma_hip_raw_sq8_train(gamma_hip_index* h, int64_t n, const float* x) {
    if (!h || n <= 0 || !x) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_et != gh::ROW_SQ8) return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_train: the raw store is not an sq8 store (gamma_hip_raw_init_sq8)");
    if (h->nraw > 0) return fail(h, GAMMA_HIP_EINVAL, "gamma_hip_raw_sq8_train: the sq8 raw store holds rows; the ranges change only while it is empty (after gamma_hip_raw_clear)");
    const int d = h->raw_d;
    GH_TRY(sq8_values_check(h, n * d, x));
    GH_CHECK(h, hipSetDevice(h->device));
    const int64_t piece = std::max<int64_t>(1, ((int64_t)16 << 20) / d);
    GH_CHECK(h, h->we_stage.ensure((size_t)std::min(piece, n) * d * sizeof(float)));
    GH_CHECK(h, h->we_chk.ensure((size_t)d * 2 * sizeof(float)));   // d minima, d maxima
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t m = std::min(piece, n - i0);
        GH_CHECK(h, hipMemcpyAsync(h->we_stage.p, x + i0 * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
        gh::launch_sq8_minmax(h->wstream, h->we_stage.as<float>(), m, d, h->we_chk.as<float>(), /*first=*/i0 == 0);
    }
    GH_CHECK(h, hipGetLastError());
    std::vector<float> mm((size_t)d * 2);
    GH_CHECK(h, hipMemcpyAsync(mm.data(), h->we_chk.p, mm.size() * sizeof(float), hipMemcpyDeviceToHost, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    for (float& v : mm) v += 0.0f;   // -0.0 -> +0.0: which zero a minimum of both returns depends on the order
    return sq8_set_ranges_locked(h, mm.data(), mm.data() + d);
}

// the writers' check in front of their reservation: ranges first, then the values (base: see byte_values_check)
static int sq8_values_check(H* h, int64_t count, const float* v, int64_t base) {
    int64_t bad = -1;
    if (gamma_hip_raw_sq8_check(v, count, &bad) == GAMMA_HIP_OK) return GAMMA_HIP_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "raw store (sq8, gamma_hip_raw_init_sq8): value %g at position %lld (row %lld, element %lld) is not finite; nothing was written",
             (double)v[bad], (long long)(base + bad), (long long)((base + bad) / h->raw_d), (long long)((base + bad) % h->raw_d));
    return fail(h, GAMMA_HIP_EINVAL, msg);
}
static int sq8_need_ranges(H* h) {
    if (!h->sq8_vmin.empty()) return GAMMA_HIP_OK;
    return fail(h, GAMMA_HIP_EINVAL, "raw store (sq8, gamma_hip_raw_init_sq8): no ranges yet (gamma_hip_raw_sq8_set_ranges / _train come before the first row); nothing was written");
}

// the check of a writer's values for the store's element type (fp32 rows take everything); base: see byte_values_check
static int raw_narrow_check(H* h, int64_t count, const float* v, int64_t base = 0) {
    switch (h->raw_et) {
        case gh::ROW_F16: return half_values_check(h, count, v);
        case gh::ROW_U8:
        case gh::ROW_I8: return byte_values_check(h, count, v, base);
        case gh::ROW_SQ8: GH_TRY(sq8_need_ranges(h)); return sq8_values_check(h, count, v, base);
        default: return GAMMA_HIP_OK;
    }
}

// n caller rows -> rows first, first + 1, .. (vids == nullptr) or rows vids[i] (those outside [0, nrows) are skipped) of a narrow
// store: staged as fp32 through the writer's staging buffer in pieces, converted by the store's kernel (launch_raw_rows_narrow) on
// the writer stream.  The caller has checked the values, reserved the rows and waits for the stream.
static int raw_narrow_rows_in(H* h, int64_t first, const int64_t* vids, int64_t n, const float* vecs, int64_t nrows) {
    const int d = h->raw_d;
    const int64_t piece = std::max<int64_t>(1, ((int64_t)16 << 20) / d);   // 64 MB of fp32 per piece
    GH_CHECK(h, h->we_stage.ensure((size_t)std::min(piece, n) * d * sizeof(float)));
    if (vids) {
        GH_CHECK(h, h->we_chk.ensure((size_t)n * sizeof(int64_t)));
        GH_CHECK(h, hipMemcpyAsync(h->we_chk.p, vids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
    }
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t m = std::min(piece, n - i0);
        GH_CHECK(h, hipMemcpyAsync(h->we_stage.p, vecs + i0 * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
        gh::launch_raw_rows_narrow(h->wstream, h->we_stage.as<float>(), vids ? h->we_chk.as<int64_t>() + i0 : nullptr, first + i0, m, d,
                                   h->raw.p, h->raw_et, h->raw_et == gh::ROW_SQ8 ? h->d_sq8_tab + 2 * (size_t)d : nullptr, nrows);
    }
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

// n caller rows into rows first, first + 1, .. of the store, on the writer stream: fp32 rows are copied into place, the rows of a
// narrow store converted on the way (nrows: the rows it may write).  The caller's part is raw_narrow_rows_in's.
static int raw_rows_in(H* h, int64_t first, int64_t n, const float* vecs, int64_t nrows) {
    if (h->raw_narrow()) return raw_narrow_rows_in(h, first, nullptr, n, vecs, nrows);
    GH_CHECK(h, hipMemcpyAsync(h->raw_f32() + first * h->raw_d, vecs, (size_t)n * h->raw_d * sizeof(float), hipMemcpyHostToDevice,
                               h->wstream));
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_append(gamma_hip_index* h, int64_t n, const float* vecs) {
    if (!h || n < 0 || (n > 0 && !vecs)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    if (n == 0) return GAMMA_HIP_OK;
    GH_TRY(raw_narrow_check(h, n * h->raw_d, vecs));
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(raw_reserve(h, h->nraw + n));
    GH_TRY(raw_rows_in(h, h->nraw, n, vecs, h->raw_cap()));
    GH_TRY(raw_image_rows_in(h, h->nraw, nullptr, n, h->raw_cap()));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->nraw += n;
    return GAMMA_HIP_OK;
}

// the device's vid -> row table reaches vector id `hi`: a larger array and the whole mirror when it does not (rare: the
// table grows by half; readers are drained first), nothing otherwise -- single entries go through k_raw_slot_scatter
static int raw_slot_reserve(H* h, int64_t hi) {
    if (hi < h->raw_slot_cap()) return GAMMA_HIP_OK;
    const int64_t ncap = std::max<int64_t>(hi + 1 + (hi + 1) / 2, 1 << 16);
    // nothing is carried over on the device: the new table is -1 throughout, then the host mirror goes up -- so a table that
    // fell behind its mirror (a raw_put or raw_drop that failed half way) is whole again after a growth
    GH_TRY(grow_array(h, "raw slot table", h->d_raw_slot, (size_t)(hi + 1) * sizeof(int32_t), (size_t)ncap * sizeof(int32_t), 0, 0xff));
    if (!h->h_raw_slot.empty())
        GH_CHECK(h, hipMemcpyAsync(h->d_raw_slot, h->h_raw_slot.data(), h->h_raw_slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

// Rows of a sparse store.  A vector the store holds keeps its row (rewritten in place), a new one takes a freed row before
// the store grows.  What a search in flight may read is never written under it: new rows at the end of the store are
// reachable by no search yet (the caller lists a vector after its row is in place, and this call returns with the writer
// stream drained); a rewrite in place and the reuse of a freed row wait for the searches in flight first (exclusive()) --
// a freed row belonged to a vector this handle no longer lists, which only a search enqueued before it left can still reach.
// On the writer stream the rows go before the table entries that point at them.
int gamma_hip_raw_put(gamma_hip_index* h, int64_t n, const int64_t* vids, const float* vecs) {
    if (!h || n < 0 || (n > 0 && (!vids || !vecs))) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    // (rows sharded with their lists are fp32 unless gamma_hip_set_sparse_narrow_rows says otherwise)
    if (h->raw_narrow() && !h->sparse_narrow_rows) return fail(h, GAMMA_HIP_EUNSUPPORTED, narrow_store_name(h));
    if (!h->raw_sparse && h->nraw > 0) return fail(h, GAMMA_HIP_EINVAL, "raw_put on a store that holds rows by vector id");
    if (n == 0) {   // the first call turns the empty store into the sparse form, rows or not (a shard that owns no vector yet)
        if (!h->raw_sparse) {
            GH_CHECK(h, hipSetDevice(h->device));
            GH_TRY(raw_reserve(h, 1));
            h->raw_sparse = true;
        }
        return GAMMA_HIP_OK;
    }
    int64_t hi = -1;
    for (int64_t i = 0; i < n; i++) {
        if (vids[i] < 0 || vids[i] >= ((int64_t)1 << 31)) return fail(h, GAMMA_HIP_EINVAL, "raw_put: vector id out of range");
        hi = std::max(hi, vids[i]);
    }
    // a narrow store: the whole batch is storable, or the call fails here with nothing changed (an sq8 store: ranges first)
    GH_TRY(raw_narrow_check(h, n * h->raw_d, vecs));
    // the row of every entry; nothing of the handle changes before the device memory is there
    std::vector<int32_t> pairs((size_t)n * 2);
    std::unordered_map<int64_t, int64_t> seen;   // vid -> its latest entry of this batch (the last one named wins)
    seen.reserve((size_t)n * 2);
    const int64_t nfree = (int64_t)h->raw_free.size();
    int64_t used_free = 0, grow = 0, fresh = 0;
    bool touches_old = false, in_order = true;
    for (int64_t i = 0; i < n; i++) {
        const int64_t v = vids[i];
        int32_t row;
        auto it = seen.find(v);
        if (it != seen.end()) {
            row = pairs[2 * it->second + 1];
            pairs[2 * it->second] = pairs[2 * it->second + 1] = -1;
            it->second = i;
            in_order = false;
        } else {
            const int32_t held = (size_t)v < h->h_raw_slot.size() ? h->h_raw_slot[v] : -1;
            if (held >= 0) {
                row = held;
                touches_old = true;
            } else {
                fresh++;
                if (used_free < nfree) {
                    row = h->raw_free[nfree - 1 - used_free++];
                    touches_old = true;
                } else {
                    if (h->nraw + grow >= ((int64_t)1 << 31) - 1) return fail(h, GAMMA_HIP_EFULL, "raw_put: more than 2^31 rows");
                    row = (int32_t)(h->nraw + grow++);
                }
            }
            seen.emplace(v, i);
        }
        pairs[2 * i] = (int32_t)v;
        pairs[2 * i + 1] = row;
    }
    in_order = in_order && !touches_old;   // rows nraw, nraw + 1, ..: the batch is the tail of the store as it stands
    GH_CHECK(h, hipSetDevice(h->device));
    if (touches_old) GH_CHECK(h, lk.exclusive());
    GH_TRY(raw_reserve(h, h->nraw + grow));
    GH_TRY(raw_slot_reserve(h, hi));
    GH_CHECK(h, h->we_chk.ensure((size_t)n * 2 * sizeof(int32_t)));
    if (!in_order && !h->raw_narrow()) GH_CHECK(h, h->we_stage.ensure((size_t)n * h->raw_d * sizeof(float)));
    h->raw_sparse = true;
    std::vector<int64_t> rows;   // (a narrow store's target rows: read by the copy below until the stream is drained)
    if (h->raw_narrow()) {
        // converted on the device by the store's writer, into the batch's rows (a superseded entry's is -1: skipped).  The
        // writer's row list goes through the buffer the pairs take behind it, in stream order.
        rows.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) rows[i] = pairs[2 * i + 1];
        GH_TRY(raw_narrow_rows_in(h, 0, rows.data(), n, vecs, h->raw_cap()));
    }
    GH_CHECK(h, hipMemcpyAsync(h->we_chk.p, pairs.data(), (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
    if (h->raw_narrow()) {   // (in place already)
    } else if (in_order) {
        GH_TRY(raw_rows_in(h, h->nraw, n, vecs, h->raw_cap()));
    } else {
        GH_CHECK(h, hipMemcpyAsync(h->we_stage.p, vecs, (size_t)n * h->raw_d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
        gh::launch_raw_rows_scatter(h->wstream, h->we_stage.as<float>(), h->we_chk.as<int32_t>(), n, h->raw_d, h->raw_f32(), h->raw_cap());
    }
    gh::launch_raw_slot_scatter(h->wstream, h->we_chk.as<int32_t>(), n, h->d_raw_slot, h->raw_slot_cap());
    GH_CHECK(h, hipGetLastError());
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    if ((int64_t)h->h_raw_slot.size() <= hi) h->h_raw_slot.resize((size_t)hi + 1, -1);
    for (int64_t i = 0; i < n; i++)
        if (pairs[2 * i] >= 0) h->h_raw_slot[pairs[2 * i]] = pairs[2 * i + 1];
    h->raw_free.resize((size_t)(nfree - used_free));
    h->nraw += grow;
    h->raw_live += fresh;
    lk.shared();
    return GAMMA_HIP_OK;
}

// the store forgets rows: their table entries go to -1 (one 4-byte store each: a search beside it reads the old row, intact,
// or none), the rows to the free list
int gamma_hip_raw_drop(gamma_hip_index* h, int64_t n, const int64_t* vids) {
    if (!h || n < 0 || (n > 0 && !vids)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_narrow() && !h->sparse_narrow_rows) return fail(h, GAMMA_HIP_EUNSUPPORTED, narrow_store_name(h));
    if (!h->raw_sparse) {
        if (h->nraw > 0) return fail(h, GAMMA_HIP_EINVAL, "raw_drop on a store that holds rows by vector id");
        return GAMMA_HIP_OK;   // empty: nothing to forget
    }
    std::vector<int32_t> pairs;
    for (int64_t i = 0; i < n; i++) {
        const int64_t v = vids[i];
        if (v < 0 || (size_t)v >= h->h_raw_slot.size() || h->h_raw_slot[v] < 0) continue;
        pairs.push_back((int32_t)v);
        pairs.push_back(-1);
        h->raw_free.push_back(h->h_raw_slot[v]);
        h->h_raw_slot[v] = -1;
        h->raw_live--;
    }
    if (pairs.empty()) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, h->we_chk.ensure(pairs.size() * sizeof(int32_t)));
    GH_CHECK(h, hipMemcpyAsync(h->we_chk.p, pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->wstream));
    gh::launch_raw_slot_scatter(h->wstream, h->we_chk.as<int32_t>(), (int64_t)pairs.size() / 2, h->d_raw_slot, h->raw_slot_cap());
    GH_CHECK(h, hipGetLastError());
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

// back to the state after gamma_hip_raw_init: no rows, no table, neither dense nor sparse yet
int gamma_hip_raw_clear(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, lk.exclusive());   // the rows are given back: no search may be reading them
    // (a mapped store keeps its address range unless the unmap went without its fence; the handle has ONE list of ranges
    //  that may not be mapped again, freed with it -- the arena's sets keep it, the raw store's ranges go there too)
    h->raw.clear(&h->arena.retired);
    h->d_raw_slot.clear(&h->arena.retired);
    h->rf.rows.clear(&h->arena.retired);   // the image goes with its rows; the next call that qualifies builds a new one
    h->rf.aux.clear(&h->arena.retired);
    h->rf.on = false;
    std::vector<int32_t>().swap(h->h_raw_slot);
    std::vector<int32_t>().swap(h->raw_free);
    h->nraw = h->raw_live = 0;
    h->raw_sparse = false;
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_sparse_stats(gamma_hip_index* h, int64_t* out3) {
    if (!h || !out3) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    out3[0] = h->raw_sparse ? h->raw_live : 0;
    out3[1] = h->raw_sparse ? h->nraw : 0;
    out3[2] = (int64_t)h->raw_free.size();
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_write(gamma_hip_index* h, int64_t first_vid, int64_t n, const float* vecs) {
    if (!h || n < 0 || first_vid < 0 || (n > 0 && !vecs)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    if (first_vid > h->nraw) return fail(h, GAMMA_HIP_EINVAL, "raw write would leave a gap");
    if (n == 0) return GAMMA_HIP_OK;
    GH_TRY(raw_narrow_check(h, n * h->raw_d, vecs));
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(raw_reserve(h, first_vid + n));
    GH_TRY(raw_rows_in(h, first_vid, n, vecs, h->raw_cap()));
    GH_TRY(raw_image_rows_in(h, first_vid, nullptr, n, h->raw_cap()));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->nraw = std::max(h->nraw, first_vid + n);
    return GAMMA_HIP_OK;
}

int gamma_hip_raw_update(gamma_hip_index* h, int64_t vid, const float* vec) {
    if (!h || !vec) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    if (vid < 0 || vid >= h->nraw) return fail(h, GAMMA_HIP_EINVAL, "vid out of range");
    GH_TRY(raw_narrow_check(h, h->raw_d, vec));
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(raw_rows_in(h, vid, 1, vec, h->nraw));
    GH_TRY(raw_image_rows_in(h, vid, nullptr, 1, h->nraw));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

// n rows rewritten (vids below the row count; others are skipped: the mirror has not reached them yet), one wait
int gamma_hip_raw_update_batch(gamma_hip_index* h, int64_t n, const int64_t* vids, const float* vecs) {
    if (!h || n < 0 || (n > 0 && (!vids || !vecs))) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    WriteLock lk(h);
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    if (h->raw_narrow()) {
        GH_TRY(raw_narrow_check(h, 0, vecs));   // (an sq8 store without ranges refuses, whether or not a row is in range)
        for (int64_t i = 0; i < n; i++)
            if (vids[i] >= 0 && vids[i] < h->nraw) GH_TRY(raw_narrow_check(h, h->raw_d, vecs + i * h->raw_d, i * h->raw_d));
        // one kernel writes all rows: of a vid named twice the last entry wins, as with the fp32 store's ordered copies
        std::vector<int64_t> v(vids, vids + n);
        std::unordered_map<int64_t, int64_t> last;
        for (int64_t i = 0; i < n; i++) {
            auto it = last.find(v[i]);
            if (it != last.end()) v[it->second] = -1;
            last[v[i]] = i;
        }
        GH_CHECK(h, hipSetDevice(h->device));
        GH_TRY(raw_narrow_rows_in(h, 0, v.data(), n, vecs, h->nraw));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        return GAMMA_HIP_OK;
    }
    GH_CHECK(h, hipSetDevice(h->device));
    for (int64_t i = 0; i < n; i++) {
        if (vids[i] < 0 || vids[i] >= h->nraw) continue;
        GH_CHECK(h, hipMemcpyAsync(h->raw_f32() + vids[i] * h->raw_d, vecs + i * h->raw_d, (size_t)h->raw_d * sizeof(float),
                                   hipMemcpyHostToDevice, h->wstream));
    }
    if (h->rf.on) {   // (a vid named twice: both entries quantise the row as the last copy left it)
        GH_CHECK(h, h->we_chk.ensure((size_t)n * sizeof(int64_t)));
        GH_CHECK(h, hipMemcpyAsync(h->we_chk.p, vids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
        GH_TRY(raw_image_rows_in(h, 0, h->we_chk.as<int64_t>(), n, h->nraw));
    }
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

// VectorReader::Gets (vector/raw_vector.cc:99-109 -> MemoryRawVector::GetVector, vector/memory_raw_vector.cc:136-142): rows
// by vector id, read back from the device store (what compute_dis hands to the exact distance); one wait for n rows
int gamma_hip_raw_gets(gamma_hip_index* h, int64_t n, const int64_t* vids, float* out) {
    if (!h || n < 0 || (n > 0 && (!vids || !out))) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    WriteLock lk(h);   // no row is read half written
    if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "the raw store holds this shard's rows only (gamma_hip_raw_put)");
    if (h->raw_d <= 0) return fail(h, GAMMA_HIP_EINVAL, "raw store not initialised");
    for (int64_t i = 0; i < n; i++)
        if (vids[i] < 0 || vids[i] >= h->nraw) return fail(h, GAMMA_HIP_EINVAL, "vid out of range");
    GH_CHECK(h, hipSetDevice(h->device));
    // the rows come back as they are: fp32 rows straight into `out`, narrow rows into a byte buffer that is widened below
    const int d = h->raw_d;
    const size_t row = (size_t)d * h->raw_esz();
    std::vector<uint8_t> bb(h->raw_narrow() ? (size_t)n * row : 0);
    char* dst = h->raw_narrow() ? reinterpret_cast<char*>(bb.data()) : reinterpret_cast<char*>(out);
    for (int64_t i = 0; i < n; i++)
        GH_CHECK(h, hipMemcpyAsync(dst + i * row, static_cast<const char*>(h->raw.p) + vids[i] * row, row, hipMemcpyDeviceToHost,
                                   h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    const size_t ne = (size_t)n * d;
    switch (h->raw_et) {
        case gh::ROW_F16: {   // widened exactly
            const uint16_t* hb = reinterpret_cast<const uint16_t*>(bb.data());
            for (size_t i = 0; i < ne; i++) out[i] = half_bits_to_float(hb[i]);
            break;
        }
        case gh::ROW_U8:
            for (size_t i = 0; i < ne; i++) out[i] = (float)bb[i];
            break;
        case gh::ROW_I8:
            for (size_t i = 0; i < ne; i++) out[i] = (float)(int8_t)bb[i];
            break;
        case gh::ROW_SQ8:   // decoded: a multiply, then an add, each rounded in fp32
            for (int64_t i = 0; i < n; i++)
                for (int j = 0; j < d; j++) {
                    const float t = (float)bb[i * d + j] * h->sq8_step[j];
                    out[i * d + j] = h->sq8_vmin[j] + t;
                }
            break;
        default: break;   // fp32: in place already
    }
    return GAMMA_HIP_OK;
}

int64_t gamma_hip_raw_count(gamma_hip_index* h) { return h ? (h->raw_sparse ? h->raw_live : h->nraw) : -1; }

int gamma_hip_raw_stats(gamma_hip_index* h, int64_t* out4) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    out4[0] = h->nraw;
    out4[1] = h->raw_cap();
    out4[2] = h->raw.regrows;
    out4[3] = h->raw.mapped ? 1 : 0;
    return GAMMA_HIP_OK;
}

/* ---- delete bitmap ------------------------------------------------------------------- */
static int bitmap_reserve(H* h, int64_t nbits) {
    size_t bytes = (((size_t)nbits >> 3) + 1 + 3) & ~(size_t)3;
    if (bytes <= h->d_bitmap.cap) return GAMMA_HIP_OK;
    const size_t ncap = std::max(bytes, h->d_bitmap.cap * 2);
    GH_TRY(grow_array(h, "bitmap", h->d_bitmap, bytes, ncap, h->d_bitmap.cap, 0));
    h->h_bitmap.resize(ncap, 0);
    return GAMMA_HIP_OK;
}

int gamma_hip_bitmap_upload(gamma_hip_index* h, const uint8_t* bitmap, int64_t nbits) {
    if (!h || nbits < 0 || (nbits > 0 && !bitmap)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_TRY(bitmap_reserve(h, nbits));
    size_t bytes = ((size_t)nbits >> 3) + 1;  // bitmap::create, util/bitmap.cc:15-23
    GH_CHECK(h, hipMemsetAsync(h->d_bitmap, 0, h->d_bitmap.cap, h->wstream));
    GH_CHECK(h, hipMemcpyAsync(h->d_bitmap, bitmap, bytes, hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    std::fill(h->h_bitmap.begin(), h->h_bitmap.end(), 0);
    memcpy(h->h_bitmap.data(), bitmap, bytes);
    h->bitmap_bits = nbits;
    h->bitmap_any = false;
    for (size_t i = 0; i < bytes && !h->bitmap_any; i++) h->bitmap_any = bitmap[i] != 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_bitmap_set(gamma_hip_index* h, const int64_t* docids, int64_t n, int value) {
    if (!h || n < 0 || (n > 0 && !docids)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (n == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    int64_t mx = 0;
    for (int64_t i = 0; i < n; i++) mx = std::max(mx, docids[i]);
    if (mx >= h->bitmap_bits) {
        GH_TRY(bitmap_reserve(h, mx + 1));
        h->bitmap_bits = std::max<int64_t>(h->bitmap_bits, mx + 1);
    }
    GH_CHECK(h, h->we_stage.ensure((size_t)n * sizeof(int64_t)));
    GH_CHECK(h, hipMemcpyAsync(h->we_stage.p, docids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
    gh::launch_bitmap_set(h->wstream, h->d_bitmap, h->we_stage.as<int64_t>(), n, h->bitmap_bits, value);
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    for (int64_t i = 0; i < n; i++) {
        int64_t id = docids[i];
        if (id < 0) continue;
        if (value) h->bitmap_any = true;
        if (value) h->h_bitmap[id >> 3] |= (uint8_t)(1u << (id & 7));
        else h->h_bitmap[id >> 3] &= (uint8_t)~(1u << (id & 7));
    }
    return GAMMA_HIP_OK;
}

/* ---- IVFPQ / IVFFLAT models ----------------------------------------------------------- */
static int ivf_init_locked(gamma_hip_index* h, int d, int nlist, int M, int metric, int bucket_init_size,
                           int bucket_max_size, bool flat, bool binary = false);
int gamma_hip_ivfpq_init(gamma_hip_index* h, int d, int nlist, int M, int nbits, int metric,
                         int bucket_init_size, int bucket_max_size) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "already initialised");
    if (d <= 0 || nlist <= 0 || M <= 0) return fail(h, GAMMA_HIP_EINVAL, "bad d/nlist/M");
    if (nbits != 8) return fail(h, GAMMA_HIP_EINVAL, "only nbits_per_idx == 8 is supported on device");
    if (d % M != 0) return fail(h, GAMMA_HIP_EINVAL, "d must be divisible by nsubvector");
    if (d / M > 64) return fail(h, GAMMA_HIP_EINVAL, "dsub > 64 unsupported");
    if (M > 64) return fail(h, GAMMA_HIP_EINVAL, "nsubvector > 64 unsupported (LUT must fit 64 KiB LDS)");
    return ivf_init_locked(h, d, nlist, M, metric, bucket_init_size, bucket_max_size, false);
}

// faiss::precomputed_table_max_bytes (faiss:IndexIVFPQ.cpp:379): process-wide like the library's extern
static std::atomic<int64_t> g_table_max_bytes{(int64_t)1 << 31};
int gamma_hip_set_precomputed_table_max_bytes(int64_t bytes) {
    if (bytes < 0) return GAMMA_HIP_EINVAL;
    g_table_max_bytes.store(bytes);
    return GAMMA_HIP_OK;
}
int64_t gamma_hip_get_precomputed_table_max_bytes(void) { return g_table_max_bytes.load(); }
int gamma_hip_ivfpq_use_precomputed_table(gamma_hip_index* h) {
    if (!h || !h->ivf_init || h->ivfflat) return GAMMA_HIP_EINVAL;
    return h->table_mode;
}

// nbits_per_idx = 4 (gamma_index_ivfpq.cc:167-170): 16 centroids per sub-quantizer, two indices per code byte
int gamma_hip_ivfpq4_init(gamma_hip_index* h, int d, int nlist, int M, int metric, int bucket_init_size,
                          int bucket_max_size) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "already initialised");
    if (d <= 0 || nlist <= 0 || M <= 0) return fail(h, GAMMA_HIP_EINVAL, "bad d/nlist/M");
    if (d % M != 0) return fail(h, GAMMA_HIP_EINVAL, "d must be divisible by nsubvector");
    if (d / M > 64) return fail(h, GAMMA_HIP_EINVAL, "dsub > 64 unsupported");
    if (gh::pq4_code_size(M) > gh::kPq4MaxCodeSize)
        return fail(h, GAMMA_HIP_EINVAL, "4-bit codes: code_size = (4 * nsubvector + 7) / 8 > 64 unsupported");
    if ((int64_t)nlist * M * gh::kPq4Ksub * (int64_t)sizeof(float) > g_table_max_bytes.load())
        return fail(h, GAMMA_HIP_EUNSUPPORTED, "4-bit codes: the precomputed table would exceed precomputed_table_max_bytes (table mode 0 is 8-bit only)");
    h->ksub = gh::kPq4Ksub;
    const int rc = ivf_init_locked(h, d, nlist, M, metric, bucket_init_size, bucket_max_size, false);
    if (rc != GAMMA_HIP_OK) h->ksub = 256;
    return rc;
}

// binary: the binary IVF model -- no float centroids, PQ codebooks or tables (gamma_hip_binivf_init)
static int ivf_init_locked(gamma_hip_index* h, int d, int nlist, int M, int metric, int bucket_init_size,
                           int bucket_max_size, bool flat, bool binary) {
    if (metric != GAMMA_HIP_METRIC_IP && metric != GAMMA_HIP_METRIC_L2) return fail(h, GAMMA_HIP_EINVAL, "bad metric");
    GH_CHECK(h, hipSetDevice(h->device));
    h->ivfflat = flat;
    // initialize_IVFPQ_precomputed_table's rule (faiss:IndexIVFPQ.cpp:441-449): `table_size > max` keeps mode 0.  faiss
    // applies it at train / Load; the outcome depends on nlist, M and the process-wide limit only, so it is fixed here,
    // where the arena decides whether it keeps the per-code table sums (they are sums of T2 entries: none in mode 0).
    const int ksub = h->ksub;   // 256, or 16 on a 4-bit handle (gamma_hip_ivfpq4_init, which has ruled table mode 0 out)
    h->table_mode = (!flat && (int64_t)nlist * M * ksub * (int64_t)sizeof(float) > g_table_max_bytes.load()) ? 0 : 1;
    // (4-bit: no code sums -- the passes built on them, cf / c8 / q8, are 8-bit kernels)
    h->keep_sums = !flat && ksub == 256 && h->table_mode == 1 && getenv("GAMMA_HIP_NO_CODE_SUMS") == nullptr;
    h->d = d;
    h->nlist = nlist;
    h->M = M;
    h->dsub = d / M;
    h->code_size = ksub == gh::kPq4Ksub ? gh::pq4_code_size(M) : M;   // IVFFLAT: M = 1, one dummy byte per entry (the arena code keeps its shape)
    h->metric = metric;
    h->bucket_init = bucket_init_size > 0 ? bucket_init_size : 1000;
    h->bucket_max = bucket_max_size > 0 ? bucket_max_size : 1280000;
    if (!binary) {
        GH_CHECK(h, hipMalloc((void**)&h->d_cc, (size_t)nlist * d * sizeof(float)));
        GH_CHECK(h, hipMalloc((void**)&h->d_cc_norms, (size_t)nlist * sizeof(float)));
        GH_CHECK(h, hipMalloc((void**)&h->d_pqc, flat ? 256 : (size_t)M * ksub * h->dsub * sizeof(float)));
        if (flat || h->table_mode == 1)
            GH_CHECK(h, hipMalloc((void**)&h->d_T2, flat ? 256 : (size_t)nlist * M * ksub * sizeof(float)));
    }
    for (int v = 0; v < H::NVER; v++) {
        GH_CHECK(h, hipMalloc((void**)&h->d_ver_off[v], (size_t)nlist * sizeof(int64_t)));
        GH_CHECK(h, hipMalloc((void**)&h->d_ver_len[v], (size_t)nlist * sizeof(int)));
        GH_CHECK(h, hipHostMalloc(&h->pin_ver[v], (size_t)nlist * (sizeof(int64_t) + sizeof(int)), hipHostMallocDefault));
    }
    h->d_list_off = h->d_ver_off[0];
    h->d_list_len = h->d_ver_len[0];
    // RTInvertBucketData::Init (realtime_mem_data.cc:57-96): bucket_init entries per list
    h->h_list_off.resize(nlist);
    h->h_list_len.assign(nlist, 0);
    h->h_list_cap.assign(nlist, h->bucket_init);
    h->h_deleted.assign(nlist, 0);
    h->h_extend_time.assign(nlist, 0);
    for (int l = 0; l < nlist; l++) h->h_list_off[l] = (int64_t)l * h->bucket_init;
    h->arena_used = 0;
    GH_TRY(arena_reserve(h, (int64_t)nlist * h->bucket_init));
    h->arena_used = (int64_t)nlist * h->bucket_init;
    GH_TRY(publish_meta(h));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->vid_pos.assign((size_t)nlist * h->bucket_init, -1);
    h->ivf_init = true;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_init(gamma_hip_index* h, int d, int nlist, int metric, int bucket_init_size, int bucket_max_size) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "already initialised");
    if (d <= 0 || nlist <= 0) return fail(h, GAMMA_HIP_EINVAL, "bad d/nlist");
    return ivf_init_locked(h, d, nlist, 1, metric, bucket_init_size, bucket_max_size, true);
}

// The bf16 hi / lo image of the centroids for the coarse filter (coarse.hip), wherever the centroids and their norms
// are set: once per trained index.  Call with the norms launched on wstream; synchronises it.
static int build_coarse_image(H* h) {
    h->cc_img_ok = false;
    if (!gh::coarse_image_supported(h->d, h->nlist)) return GAMMA_HIP_OK;
    const size_t bytes = gh::coarse_image_bytes(h->d, h->nlist);
    if (!h->d_cc_img) {
        GH_CHECK(h, hipMalloc(&h->d_cc_img, bytes));
        h->cc_img_bytes = bytes;
    }
    if (!h->d_cbf_stat) {
        GH_CHECK(h, hipMalloc((void**)&h->d_cbf_stat, 2 * sizeof(unsigned long long)));
        GH_CHECK(h, hipMemset(h->d_cbf_stat, 0, 2 * sizeof(unsigned long long)));
        GH_CHECK(h, hipHostMalloc((void**)&h->pin_cbf_stat, 2 * sizeof(unsigned long long), hipHostMallocDefault));
        h->pin_cbf_stat[0] = h->pin_cbf_stat[1] = 0;
        GH_CHECK(h, hipEventCreateWithFlags(&h->cbf_copy_ev, hipEventDisableTiming));
    }
    gh::launch_coarse_image(h->wstream, h->d_cc, h->d_cc_norms, h->nlist, h->d, h->d_cc_img);
    GH_CHECK(h, hipGetLastError());
    std::vector<float> nn((size_t)h->nlist);
    GH_CHECK(h, hipMemcpyAsync(nn.data(), h->d_cc_norms, nn.size() * sizeof(float), hipMemcpyDeviceToHost, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    float mx = 0.f;
    bool ok = true;
    for (float v : nn) {
        if (!(v <= gh::kCoarseBfNormMax)) ok = false;   // NaN included
        else mx = std::max(mx, v);
    }
    h->cc_norm_max = mx;
    h->cc_img_ok = ok;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfflat_set_trained(gamma_hip_index* h, const float* cc) {
    if (!h || !cc) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init || !h->ivfflat || h->binivf) return fail(h, GAMMA_HIP_EINVAL, "ivfflat not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipMemcpyAsync(h->d_cc, cc, (size_t)h->nlist * h->d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
    gh::launch_row_norms(h->wstream, h->d_cc, h->nlist, h->d, h->d_cc_norms);
    GH_CHECK(h, hipGetLastError());
    GH_TRY(build_coarse_image(h));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->trained = true;
    return GAMMA_HIP_OK;
}

int gamma_hip_binivf_init(gamma_hip_index* h, int nbits, int nlist, int bucket_init_size, int bucket_max_size) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "already initialised");
    if (nbits <= 0 || nbits % 8 != 0 || nbits / 8 > gh::kBinMaxCodeSize || nlist <= 0)
        return fail(h, GAMMA_HIP_EINVAL, "bad nbits / nlist (nbits % 8 == 0, at most 2048 bits)");
    if (h->bf_init && h->bf_cs != nbits / 8) return fail(h, GAMMA_HIP_EINVAL, "nbits differs from the binary flat store's");
    // the IVFFLAT set-up with M = code_size: code_size bytes per list entry; no float centroids, PQ tables or code sums
    GH_TRY(ivf_init_locked(h, nbits, nlist, nbits / 8, GAMMA_HIP_METRIC_L2, bucket_init_size, bucket_max_size, true, true));
    h->binivf = true;
    GH_CHECK(h, hipMalloc((void**)&h->d_bin_cc, (size_t)nlist * h->code_size));
    GH_CHECK(h, hipMalloc((void**)&h->d_bin_stats, 5 * sizeof(unsigned long long)));
    GH_CHECK(h, hipMemset(h->d_bin_stats, 0, 5 * sizeof(unsigned long long)));
    return GAMMA_HIP_OK;
}

int gamma_hip_binivf_set_trained(gamma_hip_index* h, const uint8_t* centroid_codes) {
    if (!h || !centroid_codes) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init || !h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binivf not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipMemcpyAsync(h->d_bin_cc, centroid_codes, (size_t)h->nlist * h->code_size, hipMemcpyHostToDevice,
                               h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->trained = true;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_set_trained(gamma_hip_index* h, const float* cc, const float* pqc, const float* table) {
    if (!h || !cc || !pqc) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init || h->ivfflat) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    const size_t ncc = (size_t)h->nlist * h->d, npq = (size_t)h->M * h->ksub * h->dsub;
    const size_t nt = (size_t)h->nlist * h->M * h->ksub;
    GH_CHECK(h, hipMemcpyAsync(h->d_cc, cc, ncc * sizeof(float), hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipMemcpyAsync(h->d_pqc, pqc, npq * sizeof(float), hipMemcpyHostToDevice, h->wstream));
    gh::launch_row_norms(h->wstream, h->d_cc, h->nlist, h->d, h->d_cc_norms);
    GH_TRY(build_coarse_image(h));
    if (h->table_mode == 0) {
        // no table (a supplied one is not taken either: the reference would not have built it)
    } else if (table)
        GH_CHECK(h, hipMemcpyAsync(h->d_T2, table, nt * sizeof(float), hipMemcpyHostToDevice, h->wstream));
    else if (h->ksub == gh::kPq4Ksub)
        gh::launch_pq4_precompute_table(h->wstream, h->d_cc, h->nlist, h->d, h->M, h->d_pqc, h->d_T2);
    else
        gh::launch_precompute_table(h->wstream, h->d_cc, h->nlist, h->d, h->M, h->d_pqc, h->d_T2);
    {
        std::vector<int> rank = centroid_rank(cc, h->nlist, h->d);
        if (!h->d_list_rank) GH_CHECK(h, hipMalloc((void**)&h->d_list_rank, (size_t)h->nlist * sizeof(int)));
        GH_CHECK(h, hipMemcpyAsync(h->d_list_rank, rank.data(), (size_t)h->nlist * sizeof(int),
                                   hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));   // rank is a local
    }
    if (h->keep_sums) {
        if (!h->d_t2max) GH_CHECK(h, hipMalloc((void**)&h->d_t2max, (size_t)h->nlist * sizeof(float)));
        gh::launch_t2_rowmax(h->wstream, h->d_T2, h->nlist, h->M, h->d_t2max);
    }
    GH_CHECK(h, hipGetLastError());
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->t2max_all = 0.f;
    if (h->keep_sums && h->d_t2max) {   // the largest of the per-list bounds: the filter pass's margin without a look-up per list
        std::vector<float> tm((size_t)h->nlist);
        GH_CHECK(h, hipMemcpy(tm.data(), h->d_t2max, tm.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (float v : tm) h->t2max_all = std::max(h->t2max_all, v);
    }
    h->trained = true;
    if (h->ntotal > 0) {   // a new table under existing lists: their sums follow it
        GH_TRY(sums_all_lists(h));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_get_precomputed_table(gamma_hip_index* h, float* out) {
    if (!h || !out) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "not trained");
    if (h->table_mode == 0) return fail(h, GAMMA_HIP_EUNSUPPORTED, "table mode 0: no precomputed table (it would exceed precomputed_table_max_bytes)");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipMemcpyAsync(out, h->d_T2, (size_t)h->nlist * h->M * h->ksub * sizeof(float),
                               hipMemcpyDeviceToHost, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

/* ---- realtime lists ------------------------------------------------------------------- */
int gamma_hip_ivfpq_add_keys(gamma_hip_index* h, int list_no, int n, const int64_t* vids, const uint8_t* codes) {
    if (!h || (n > 0 && (!vids || !codes))) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    return add_keys_locked(h, list_no, n, vids, codes);
}

int gamma_hip_ivfpq_add_keys_batch(gamma_hip_index* h, int nlists, const int32_t* list_nos,
                                   const int32_t* counts, const int64_t* vids, const uint8_t* codes) {
    if (!h || nlists < 0 || (nlists > 0 && (!list_nos || !counts || !vids || !codes))) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    int64_t off = 0;
    // grow first so that no copy below races with an arena move; a list named twice reserves for the sum
    {
        std::map<int, int64_t> per_list;
        for (int i = 0; i < nlists; i++) {
            if (list_nos[i] < 0 || list_nos[i] >= h->nlist || counts[i] < 0) return fail(h, GAMMA_HIP_EINVAL, "bad list_no");
            per_list[list_nos[i]] += counts[i];
        }
        for (auto& kv : per_list) {
            if (kv.second > h->bucket_max) return fail(h, GAMMA_HIP_EFULL, "exceed the max bucket keys");
            GH_TRY(list_ensure(h, kv.first, (int)kv.second));
        }
    }
    std::vector<int> r_list, r_n;      // the appended ranges, for the code sums (alive until the wait below)
    std::vector<int64_t> r_pos;
    int r_max = 0;
    for (int i = 0; i < nlists; i++) {
        const int l = list_nos[i], n = counts[i];
        if (n == 0) continue;
        const int64_t pos = h->h_list_off[l] + h->h_list_len[l];
        r_list.push_back(l);
        r_n.push_back(n);
        r_pos.push_back(pos);
        r_max = std::max(r_max, n);
        GH_CHECK(h, hipMemcpyAsync(h->d_ids + pos, vids + off, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(h->d_codes + pos * h->code_size, codes + off * h->code_size,
                                   (size_t)n * h->code_size, hipMemcpyHostToDevice, h->wstream));
        for (int j = 0; j < n; j++) {
            const int64_t v = vids[off + j];
            if (v < 0) {   // superseded slot restored from a dump: same accounting as add_keys_locked, so that
                h->h_deleted[l]++;   // the scan reads the ids (n_moved) and never returns the slot
                h->n_moved++;
                continue;
            }
            if ((size_t)v >= h->vid_pos.size()) h->vid_pos.resize(std::max<size_t>(h->vid_pos.size() * 2, v + 1), -1);
            h->vid_pos[v] = ((int64_t)l << 32) | (int64_t)(h->h_list_len[l] + j);
            if (h->doc_deleted(v)) h->h_deleted[l]++;
        }
        h->h_list_len[l] += n;
        h->ntotal += n;
        if (h->h_list_len[l] > h->max_list_len) h->max_list_len = h->h_list_len[l];
        off += n;
    }
    if (h->d_sums && h->trained && !r_list.empty()) {
        const size_t nr = r_list.size(), o_n = nr * sizeof(int), o_pos = (2 * nr * sizeof(int) + 7) & ~(size_t)7;
        GH_CHECK(h, h->we_stage.ensure(o_pos + nr * sizeof(int64_t)));
        char* b = h->we_stage.as<char>();
        GH_CHECK(h, hipMemcpyAsync(b, r_list.data(), nr * sizeof(int), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(b + o_n, r_n.data(), nr * sizeof(int), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(b + o_pos, r_pos.data(), nr * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
        gh::launch_code_sums_ranges(h->wstream, h->d_T2, h->d_codes, h->code_size, reinterpret_cast<int*>(b),
                                    reinterpret_cast<int64_t*>(b + o_pos), reinterpret_cast<int*>(b + o_n), (int)nr, r_max,
                                    h->d_sums);
    }
    // publish the new lengths (and moved extents) after the copies, in stream order
    GH_TRY(publish_meta(h));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return arena_repack_if_need(h);
}

int gamma_hip_ivfpq_update(gamma_hip_index* h, int list_no, int64_t vid, const uint8_t* code) {
    if (!h || !code) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init || list_no < 0 || list_no >= h->nlist) return fail(h, GAMMA_HIP_EINVAL, "bad list_no");
    if (vid < 0 || (size_t)vid >= h->vid_pos.size()) return GAMMA_HIP_OK;  // realtime_mem_data.cc:307
    const int64_t bp = h->vid_pos[vid];
    if (bp == -1) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    const int ob = (int)(bp >> 32), op = (int)(bp & 0xffffffff);
    if (ob == list_no) {
        GH_CHECK(h, hipMemcpyAsync(h->d_codes + (h->h_list_off[ob] + op) * h->code_size, code, h->code_size,
                                   hipMemcpyHostToDevice, h->wstream));
        GH_TRY(sums_range(h, ob, h->h_list_off[ob] + op, 1));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        return GAMMA_HIP_OK;
    }
    GH_TRY(list_ensure(h, list_no, 1));   // before the old entry is given up: a full list must not lose the vector
    gh::launch_mark_moved(h->wstream, h->d_ids, h->h_list_off[ob] + op);
    h->h_deleted[ob]++;
    h->n_moved++;
    h->ntotal -= 1;  // add_keys_locked re-counts it
    return add_keys_locked(h, list_no, 1, &vid, code);
}

// n list updates with the codes already computed: what RTInvertIndex::Update (realtime_mem_data.cc:305-327) does for
// each entry in order, with ONE publish of the lists' tables and ONE wait for the device at the end.
//   ops[i] (nullptr = all 0)   0: Update -- a vid this handle does not hold is ignored (:307-311)
//                              1: the vid is held by ANOTHER shard of a list-sharded index and joins list_nos[i] here: AddKeys
//                              2: the vid leaves this shard: the first half of Update alone (gamma_hip_ivfpq_remove)
int gamma_hip_ivfpq_apply_updates(gamma_hip_index* h, int n, const int32_t* list_nos, const int64_t* vids,
                                  const uint8_t* codes, const uint8_t* ops) {
    if (!h || n < 0 || (n > 0 && (!list_nos || !vids || !codes))) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    const int cs = h->code_size;
    // room first: an upper bound of the entries every list may receive (an entry that stays in its list needs none,
    // but a vid named twice may have moved in between -- counted as a move), so that no extent moves while the copies
    // below are in flight
    {
        std::map<int, int64_t> per_list;
        for (int i = 0; i < n; i++) {
            const int op = ops ? ops[i] : 0;
            if (op == 2) continue;
            if (list_nos[i] < 0 || list_nos[i] >= h->nlist) return fail(h, GAMMA_HIP_EINVAL, "bad list_no");
            if (op == 0) {
                const int64_t v = vids[i];
                if (v < 0 || (size_t)v >= h->vid_pos.size() || h->vid_pos[v] == -1) continue;
            }
            per_list[list_nos[i]]++;
        }
        for (auto& kv : per_list) {
            if (h->h_list_len[kv.first] + kv.second > h->bucket_max) return fail(h, GAMMA_HIP_EFULL, "exceed the max bucket keys");
            GH_TRY(list_ensure(h, kv.first, (int)kv.second));
        }
    }
    bool changed = false;
    for (int i = 0; i < n; i++) {
        const int op = ops ? ops[i] : 0;
        const int64_t vid = vids[i];
        const int l = list_nos[i];
        const uint8_t* code = codes + (size_t)i * cs;
        int64_t bp = -1;
        if (vid >= 0 && (size_t)vid < h->vid_pos.size()) bp = h->vid_pos[vid];
        if (op != 1) {
            if (bp == -1) continue;   // not held here
            const int ob = (int)(bp >> 32), opos = (int)(bp & 0xffffffff);
            if (op == 0 && ob == l) {   // same list: the code is rewritten in place
                GH_CHECK(h, hipMemcpyAsync(h->d_codes + (h->h_list_off[ob] + opos) * cs, code, cs, hipMemcpyHostToDevice, h->wstream));
                GH_TRY(sums_range(h, ob, h->h_list_off[ob] + opos, 1));
                continue;
            }
            gh::launch_mark_moved(h->wstream, h->d_ids, h->h_list_off[ob] + opos);
            h->h_deleted[ob]++;
            h->n_moved++;
            h->ntotal -= 1;
            h->vid_pos[vid] = -1;
            if (op == 2) continue;
        }
        // AddKeys of one entry (add_keys_locked without its publish)
        const int64_t pos = h->h_list_off[l] + h->h_list_len[l];
        GH_CHECK(h, hipMemcpyAsync(h->d_ids + pos, vids + i, sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(h->d_codes + pos * cs, code, cs, hipMemcpyHostToDevice, h->wstream));
        GH_TRY(sums_range(h, l, pos, 1));
        if ((size_t)vid >= h->vid_pos.size()) h->vid_pos.resize(std::max<size_t>(h->vid_pos.size() * 2, vid + 1), -1);
        h->vid_pos[vid] = ((int64_t)l << 32) | (int64_t)h->h_list_len[l];
        if (h->doc_deleted(vid)) h->h_deleted[l]++;
        h->h_list_len[l] += 1;
        h->ntotal += 1;
        if (h->h_list_len[l] > h->max_list_len) h->max_list_len = h->h_list_len[l];
        changed = true;
    }
    if (changed) GH_TRY(publish_meta(h));
    GH_CHECK(h, hipGetLastError());
    GH_CHECK(h, hipStreamSynchronize(h->wstream));   // the caller's buffers are free again
    return changed ? arena_repack_if_need(h) : GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_has_vid(gamma_hip_index* h, const int64_t* vids, int n, uint8_t* out) {
    if (!h || n < 0 || (n > 0 && (!vids || !out))) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    for (int i = 0; i < n; i++)
        out[i] = vids[i] >= 0 && (size_t)vids[i] < h->vid_pos.size() && h->vid_pos[vids[i]] != -1;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_remove(gamma_hip_index* h, int64_t vid) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    if (vid < 0 || (size_t)vid >= h->vid_pos.size()) return GAMMA_HIP_OK;
    const int64_t bp = h->vid_pos[vid];
    if (bp == -1) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    const int ob = (int)(bp >> 32), op = (int)(bp & 0xffffffff);
    gh::launch_mark_moved(h->wstream, h->d_ids, h->h_list_off[ob] + op);
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    h->h_deleted[ob]++;
    h->n_moved++;
    h->ntotal -= 1;
    h->vid_pos[vid] = -1;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_delete(gamma_hip_index* h, const int64_t* vids, int n) {
    if (!h || (n > 0 && !vids)) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    for (int i = 0; i < n; i++) {
        if (vids[i] < 0 || (size_t)vids[i] >= h->vid_pos.size()) continue;
        const int64_t bp = h->vid_pos[vids[i]];
        if (bp == -1) continue;
        h->h_deleted[bp >> 32]++;
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_compact_if_need(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    std::vector<int64_t> ids;
    std::vector<uint8_t> codes;
    bool changed = false;
    for (int l = 0; l < h->nlist; l++) {
        const int len = h->h_list_len[l];
        if (!((float)h->h_deleted[l] / len >= 0.3f)) continue;  // Compactable, :373-377
        ids.resize(len);
        codes.resize((size_t)len * h->code_size);
        GH_CHECK(h, hipMemcpyAsync(ids.data(), h->d_ids + h->h_list_off[l], (size_t)len * sizeof(int64_t), hipMemcpyDeviceToHost, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(codes.data(), h->d_codes + h->h_list_off[l] * h->code_size, (size_t)len * h->code_size, hipMemcpyDeviceToHost, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        int pos = 0;
        for (int i = 0; i < len; i++) {  // CompactOne, :98-112
            const int64_t id = ids[i];
            const int64_t v = id & ~kDelMask;
            const bool deleted = h->doc_deleted(v);
            if (!(id & kDelMask) && !deleted) {
                ids[pos] = id;
                memmove(codes.data() + (size_t)pos * h->code_size, codes.data() + (size_t)i * h->code_size, h->code_size);
                h->vid_pos[id] = ((int64_t)l << 32) | pos;
                pos++;
            }
        }
        // new region of the same capacity (copy-on-write swap, :426-474)
        GH_TRY(arena_reserve(h, h->h_list_cap[l]));
        const int64_t noff = h->arena_used;
        h->arena_used += h->h_list_cap[l];
        h->arena_waste += h->h_list_cap[l];
        if (pos > 0) {
            GH_CHECK(h, hipMemcpyAsync(h->d_ids + noff, ids.data(), (size_t)pos * sizeof(int64_t), hipMemcpyHostToDevice, h->wstream));
            GH_CHECK(h, hipMemcpyAsync(h->d_codes + noff * h->code_size, codes.data(), (size_t)pos * h->code_size, hipMemcpyHostToDevice, h->wstream));
            GH_TRY(sums_range(h, l, noff, pos));
        }
        h->h_list_off[l] = noff;
        h->ntotal -= (len - pos);
        h->h_list_len[l] = pos;
        h->h_deleted[l] = 0;
        GH_CHECK(h, hipStreamSynchronize(h->wstream));   // ids / codes are locals of this loop
        changed = true;
    }
    if (changed) {
        GH_TRY(publish_meta(h));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        GH_TRY(arena_repack_if_need(h));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_arena_stats(gamma_hip_index* h, int64_t* out4) {
    if (!h || !out4) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    out4[0] = h->arena_cap;
    out4[1] = h->arena_used;
    out4[2] = h->arena_waste;
    out4[3] = h->n_repacks;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_repack_verify_stats(gamma_hip_index* h, int64_t* out2) {
    if (!h || !out2) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    out2[0] = h->repack_verified;
    out2[1] = h->repack_verify_failures;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_arena_growth(gamma_hip_index* h, int64_t* out2) {
    if (!h || !out2) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    out2[0] = h->arena_regrows;
    out2[1] = h->arena_vmm() ? 1 : 0;
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_set_repack_threshold(gamma_hip_index* h, int64_t min_waste_entries) {
    if (!h || min_waste_entries < 0) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    GH_CHECK(h, hipSetDevice(h->device));
    h->repack_min_entries = min_waste_entries;
    return arena_repack_if_need(h);
}

int64_t gamma_hip_ivfpq_list_size(gamma_hip_index* h, int l) {
    if (!h || !h->ivf_init || l < 0 || l >= h->nlist) return -1;
    return h->h_list_len[l];
}
int64_t gamma_hip_ivfpq_list_capacity(gamma_hip_index* h, int l) {
    if (!h || !h->ivf_init || l < 0 || l >= h->nlist) return -1;
    return h->h_list_cap[l];
}

int gamma_hip_ivfpq_get_list(gamma_hip_index* h, int l, int64_t* vids, uint8_t* codes) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init || l < 0 || l >= h->nlist) return fail(h, GAMMA_HIP_EINVAL, "bad list_no");
    const int len = h->h_list_len[l];
    if (len == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    if (vids) GH_CHECK(h, hipMemcpyAsync(vids, h->d_ids + h->h_list_off[l], (size_t)len * sizeof(int64_t), hipMemcpyDeviceToHost, h->wstream));
    if (codes) GH_CHECK(h, hipMemcpyAsync(codes, h->d_codes + h->h_list_off[l] * h->code_size, (size_t)len * h->code_size, hipMemcpyDeviceToHost, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_set_list_mask(gamma_hip_index* h, const uint8_t* owned) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    if (h->ksub == gh::kPq4Ksub) return fail(h, GAMMA_HIP_EUNSUPPORTED, "4-bit handle: list shards (gamma_hip_ivfpq_set_list_mask) are 8-bit only");
    if (h->d_opq) return fail(h, GAMMA_HIP_EUNSUPPORTED, "handle with an OPQ matrix: list shards (gamma_hip_ivfpq_set_list_mask) are not supported");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, lk.exclusive());
    if (!owned) {
        if (h->d_list_mask) GH_CHECK(h, hipFree(h->d_list_mask));
        h->d_list_mask = nullptr;
        h->h_list_mask.clear();
        return GAMMA_HIP_OK;
    }
    if (!h->d_list_mask) GH_CHECK(h, hipMalloc((void**)&h->d_list_mask, (size_t)h->nlist));
    h->h_list_mask.assign(owned, owned + h->nlist);
    GH_CHECK(h, hipMemcpyAsync(h->d_list_mask, owned, (size_t)h->nlist, hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

/* ---- device-side encode / add ----------------------------------------------------------- */
// exact: the arithmetic form faiss picks from the size of the WHOLE assign() call (n < 20), not of a chunk
static int encode_locked(H* h, int64_t n, const float* d_vecs, int* d_assign, uint8_t* d_codes_out, bool exact) {
    // quantizer->assign == search with k = 1 (faiss rule for the arithmetic form)
    hipStream_t s = h->wstream;   // own stream and own workspace: runs beside the searches
    const int d = h->d, nlist = h->nlist;
    GH_CHECK(h, h->we_mat.ensure((size_t)n * nlist * sizeof(float)));
    GH_CHECK(h, h->we_cdis.ensure((size_t)n * sizeof(float)));
    if (exact) {
        gh::launch_pairwise(s, true, d_vecs, (int)n, d, h->d_cc, nlist, h->we_mat.as<float>(), nlist);
    } else {
        gh::launch_l2_gemmform(s, d_vecs, (int)n, d, h->d_cc, nlist, nullptr, h->d_cc_norms,
                               h->we_mat.as<float>(), nlist, true);
    }
    gh::launch_select_topk(s, true, h->we_mat.as<float>(), nlist, nullptr, nlist, nlist, (int)n, 1,
                           h->we_cdis.as<float>(), d_assign);
    if (h->ivfflat) GH_CHECK(h, hipMemsetAsync(d_codes_out, 0, (size_t)n, s));   // the dummy byte of every entry
    else if (h->ksub == gh::kPq4Ksub) gh::launch_pq4_encode(s, d_vecs, n, d, h->M, d_assign, h->d_cc, h->d_pqc, d_codes_out);
    else gh::launch_pq_encode(s, d_vecs, n, d, h->M, d_assign, h->d_cc, h->d_pqc, d_codes_out);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

static int encode_host(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos, uint8_t* codes, bool exact);

int gamma_hip_ivfpq_encode(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos, uint8_t* codes) {
    return encode_host(h, n, vecs, list_nos, codes, n < 20);
}

// every vector assigned as a call of its own would assign it (quantizer->assign(1, ..): the exact form, what
// GammaIVFPQIndex::Update runs per vector, gamma_index_ivfpq.cc:398), in one device pass
int gamma_hip_ivfpq_encode_each(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos, uint8_t* codes) {
    return encode_host(h, n, vecs, list_nos, codes, true);
}

static int encode_host(gamma_hip_index* h, int64_t n, const float* vecs, int64_t* list_nos, uint8_t* codes, bool exact) {
    if (!h || n < 0 || (n > 0 && (!vecs || !list_nos || !codes))) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (h->binivf) return fail(h, GAMMA_HIP_EINVAL, "binary IVF handle: gamma_hip_binivf_add");
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "not trained");
    if (n == 0) return GAMMA_HIP_OK;
    if (!exact && blas_form_not_restated(n, h->nlist, h->d)) h->blas_unrestated++;
    GH_CHECK(h, hipSetDevice(h->device));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, 65536), (int64_t)(h->dist_budget_bytes / ((size_t)h->nlist * sizeof(float)))));
    std::vector<int> assign(chunk);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nc = std::min(chunk, n - i0);
        GH_CHECK(h, h->we_x.ensure((size_t)nc * h->d * sizeof(float)));
        GH_CHECK(h, h->we_assign.ensure((size_t)nc * sizeof(int)));
        GH_CHECK(h, h->we_codes.ensure((size_t)nc * h->code_size));
        GH_CHECK(h, hipMemcpyAsync(h->we_x.p, vecs + i0 * h->d, (size_t)nc * h->d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
        const float* d_vecs = h->we_x.as<float>();
        if (h->d_opq) {   // OPQ: assignment and codes are those of the rotated vectors (gamma_index_ivfpq.cc:375-512)
            GH_CHECK(h, h->we_xrot.ensure((size_t)nc * h->d * sizeof(float)));
            gh::launch_opq_apply(h->wstream, h->d_opq, h->d, d_vecs, nc, h->we_xrot.as<float>());
            GH_CHECK(h, hipGetLastError());
            d_vecs = h->we_xrot.as<float>();
        }
        GH_TRY(encode_locked(h, nc, d_vecs, h->we_assign.as<int>(), h->we_codes.as<uint8_t>(), exact));
        GH_CHECK(h, hipMemcpyAsync(assign.data(), h->we_assign.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost, h->wstream));
        GH_CHECK(h, hipMemcpyAsync(codes + i0 * h->code_size, h->we_codes.p, (size_t)nc * h->code_size, hipMemcpyDeviceToHost, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
        for (int64_t i = 0; i < nc; i++) list_nos[i0 + i] = assign[i];
    }
    return GAMMA_HIP_OK;
}

// GammaIVFPQIndex::Update for a batch (gamma_index_ivfpq.cc:375-422; the engine drains up to 20 000 updated vids per
// pass, vector/vector_manager.cc:355-380): one encode, the list updates in order, one publish
int gamma_hip_ivfpq_update_batch(gamma_hip_index* h, int n, const int64_t* vids, const float* vecs) {
    if (!h || n < 0 || (n > 0 && (!vids || !vecs))) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    int cs = 0;
    {
        std::lock_guard<std::mutex> g(h->mu);
        if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "not trained");
        cs = h->code_size;
    }
    std::vector<int64_t> lno(n);
    std::vector<uint8_t> codes((size_t)n * cs);
    GH_TRY(encode_host(h, n, vecs, lno.data(), codes.data(), true));
    std::vector<int32_t> l32(n);
    for (int i = 0; i < n; i++) l32[i] = (int32_t)lno[i];
    return gamma_hip_ivfpq_apply_updates(h, n, l32.data(), vids, codes.data(), nullptr);
}

int gamma_hip_assign(gamma_hip_index* h, int d, int64_t n, const float* x, int k, const float* centroids,
                     int32_t* assign, float* dis) {
    if (!h || d <= 0 || n < 0 || k <= 0 || (n > 0 && (!x || !centroids || !assign))) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (h->replay_pending) {
        GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_rdone, 0));
        h->replay_pending = false;
    }
    if (n == 0) return GAMMA_HIP_OK;
    if (blas_form_not_restated(n, k, d)) h->blas_unrestated++;
    GH_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // centroids + their norms live in the (otherwise unused here) partial-result buffers
    GH_CHECK(h, h->w_part_v.ensure((size_t)k * d * sizeof(float)));
    GH_CHECK(h, h->w_xn.ensure((size_t)k * sizeof(float)));
    GH_CHECK(h, hipMemcpyAsync(h->w_part_v.p, centroids, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, s));
    gh::launch_row_norms(s, h->w_part_v.as<float>(), k, d, h->w_xn.as<float>());
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(h->dist_budget_bytes / ((size_t)k * sizeof(float)))));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nc = std::min(chunk, n - i0);
        GH_CHECK(h, h->w_x.ensure((size_t)nc * d * sizeof(float)));
        GH_CHECK(h, h->w_mat.ensure((size_t)nc * k * sizeof(float)));
        GH_CHECK(h, h->w_assign.ensure((size_t)nc * sizeof(int)));
        GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nc * sizeof(float)));
        GH_CHECK(h, hipMemcpyAsync(h->w_x.p, x + i0 * d, (size_t)nc * d * sizeof(float), hipMemcpyHostToDevice, s));
        gh::launch_l2_gemmform(s, h->w_x.as<float>(), (int)nc, d, h->w_part_v.as<float>(), k, nullptr,
                               h->w_xn.as<float>(), h->w_mat.as<float>(), k, true);
        gh::launch_select_topk(s, true, h->w_mat.as<float>(), k, nullptr, k, k, (int)nc, 1,
                               h->w_coarse_dis.as<float>(), h->w_assign.as<int>());
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipMemcpyAsync(assign + i0, h->w_assign.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost, s));
        if (dis) GH_CHECK(h, hipMemcpyAsync(dis + i0, h->w_coarse_dis.p, (size_t)nc * sizeof(float), hipMemcpyDeviceToHost, s));
        GH_CHECK(h, hipStreamSynchronize(s));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_add(gamma_hip_index* h, int64_t n, const float* vecs, int64_t first_vid) {
    if (!h || n < 0 || (n > 0 && !vecs)) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    std::vector<int64_t> lno(n);
    std::vector<uint8_t> codes;
    {
        std::lock_guard<std::mutex> g(h->mu);
        if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "not trained");
        codes.resize((size_t)n * h->code_size);
    }
    GH_TRY(gamma_hip_ivfpq_encode(h, n, vecs, lno.data(), codes.data()));
    // group by list in ascending list order (std::map in gamma_index_ivfpq.cc:428-494)
    const int cs = h->code_size;
    std::vector<int64_t> order(n);
    for (int64_t i = 0; i < n; i++) {
        if (lno[i] < 0) lno[i] = (first_vid + i) % h->nlist;
        order[i] = i;
    }
    // list-sharded index: every shard is handed the same batch and keeps the vectors whose list it owns
    // (realtime inserts route to the owner of the assigned list) -- no exchange needed
    {
        std::lock_guard<std::mutex> g(h->mu);
        if (!h->h_list_mask.empty()) {
            int64_t m = 0;
            for (int64_t i = 0; i < n; i++)
                if (h->h_list_mask[lno[i]]) order[m++] = i;
            order.resize(m);
        }
    }
    const int64_t nkeep = (int64_t)order.size();
    if (nkeep == 0) return GAMMA_HIP_OK;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return lno[a] < lno[b]; });
    std::vector<int32_t> lists, counts;
    std::vector<int64_t> vids(nkeep);
    std::vector<uint8_t> gcodes((size_t)nkeep * cs);
    for (int64_t i = 0; i < nkeep; i++) {
        const int64_t src = order[i];
        vids[i] = first_vid + src;
        memcpy(gcodes.data() + (size_t)i * cs, codes.data() + (size_t)src * cs, cs);
        if (lists.empty() || lists.back() != (int32_t)lno[src]) {
            lists.push_back((int32_t)lno[src]);
            counts.push_back(0);
        }
        counts.back()++;
    }
    return gamma_hip_ivfpq_add_keys_batch(h, (int)lists.size(), lists.data(), counts.data(), vids.data(), gcodes.data());
}

}  // extern "C"

// ---- the store's answers to a caller that holds several handles (gamma_hip_internal.h; the group asks through its table) -------
namespace ghi {

int raw_rows_check(H* h, int64_t n, const float* vecs) {
    if (!h || n < 0 || (n > 0 && !vecs)) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->raw_d <= 0) return GAMMA_HIP_OK;
    return raw_narrow_check(h, n * h->raw_d, vecs);
}

bool raw_same_rows(H* a, H* b) {
    if (!a || !b) return false;
    int et, d;
    std::vector<float> lo, hi;
    {
        std::lock_guard<std::mutex> g(a->mu);
        et = a->raw_et, d = a->raw_d, lo = a->sq8_vmin, hi = a->sq8_vmax;
    }
    std::lock_guard<std::mutex> g(b->mu);
    if (b->raw_et != et || b->raw_d != d || lo.size() != b->sq8_vmin.size()) return false;
    return lo.empty() || (memcmp(lo.data(), b->sq8_vmin.data(), lo.size() * sizeof(float)) == 0 &&
                          memcmp(hi.data(), b->sq8_vmax.data(), hi.size() * sizeof(float)) == 0);
}

}  // namespace ghi
