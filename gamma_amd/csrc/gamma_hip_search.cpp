// gamma_hip_search.cpp -- what every search of libgamma_hip.so shares (validity filters, parameter checks, the exact-ties
// choice, the coarse quantizer, the exact scanners' row reference and tie-replay arguments), the IVFPQ pipeline (stages A
// and B, the small-batch chain, list compaction, the chunked driver) and the IVFPQ entry points of the C ABI
// (include/gamma_hip.h).  IVFFLAT, flat and the list-shard / merge entries are gamma_hip_search_ivfflat.cpp, _flat.cpp and
// _shard.cpp; the combining queue is gamma_hip_combine.cpp.  No CPU fallback: every entry point runs the HIP kernels or
// returns an error.
#include "gamma_hip_internal.h"
#include "gamma_hip_search.h"
#include "opq.h"

namespace ghi {


// off != nullptr: the range bitmaps go to w_filter at *off (advanced; the caller has sized w_filter for all
// the requests of a combined batch); nullptr: a call of its own, bitmaps from offset 0
// est_codes > 0: about how many list entries (rows, for the flat search) the call will test against the filter; when
// that is several times the number of documents, the field / term clauses are evaluated once per document into a
// bitmap (k_filter_bitmap) and join the request's range bitmaps -- the scan then tests a bit instead of reading column
// values (C5 shape, 10 % range filter on an int64 column: scan 9.6 -> 7.5 ms per 4096 queries)
int build_filter(H* h, const gamma_hip_search_params* p, gh::FilterDesc* f, size_t* off_io, int64_t est_codes) {
    memset(f, 0, sizeof(*f));
    f->del_bitmap = h->d_bitmap;
    f->del_bits = h->d_bitmap ? h->bitmap_bits : 0;
    f->vid2doc = h->h_v2d.empty() ? nullptr : h->d_v2d;
    f->n_vid2doc = (int64_t)h->h_v2d.size();
    f->has_range = p->has_range ? 1 : 0;
    f->n_range = p->has_range ? p->n_range : 0;
    if (f->n_range > gh::kMaxRange) return fail(h, GAMMA_HIP_EINVAL, "too many range filters");
    if (f->n_range > 0) {
        size_t tot = 0;
        for (int i = 0; i < f->n_range; i++) tot += ((size_t)p->range[i].bitmap_bytes + 15) & ~(size_t)15;
        if (!off_io) GH_CHECK(h, h->w_filter.ensure(tot));
        size_t off = off_io ? *off_io : 0;
        for (int i = 0; i < f->n_range; i++) {
            const gamma_hip_range_filter& r = p->range[i];
            uint8_t* dst = h->w_filter.as<uint8_t>() + off;
            GH_CHECK(h, hipMemcpyAsync(dst, r.bitmap, (size_t)r.bitmap_bytes, hipMemcpyHostToDevice,
                                       h->stream));
            f->range[i].bitmap = dst;
            f->range[i].min_doc = r.min_doc;
            f->range[i].max_doc = r.max_doc;
            f->range[i].min_aligned = r.min_aligned;
            f->range[i].b_not_in = r.b_not_in;
            off += ((size_t)r.bitmap_bytes + 15) & ~(size_t)15;
        }
        if (off_io) *off_io = off;
    }
    f->n_field = p->n_field;
    if (p->n_field < 0 || p->n_field > gh::kMaxField || (p->n_field > 0 && !p->field))
        return fail(h, GAMMA_HIP_EINVAL, "bad field filters");
    for (int i = 0; i < p->n_field; i++) {
        const gamma_hip_field_filter& ff = p->field[i];
        auto it = h->fields.find(ff.field_id);
        if (it == h->fields.end()) return fail(h, GAMMA_HIP_EINVAL, "field filter on an unknown column");
        gh::FieldDesc& fd = f->field[i];
        fd.col = it->second.d;
        fd.n = it->second.n;
        fd.dtype = it->second.dtype;
        fd.incl = (ff.include_lower ? 1 : 0) | (ff.include_upper ? 2 : 0);
        fd.lo_i = ff.lower_i;
        fd.hi_i = ff.upper_i;
        fd.lo_f = ff.lower_f;
        fd.hi_f = ff.upper_f;
    }
    f->n_term = p->n_term;
    if (p->n_term < 0 || p->n_term > gh::kMaxTerm || (p->n_term > 0 && !p->term))
        return fail(h, GAMMA_HIP_EINVAL, "bad term filters");
    for (int i = 0; i < p->n_term; i++) {
        const gamma_hip_term_filter& tf = p->term[i];
        auto it = h->terms.find(tf.field_id);
        if (it == h->terms.end()) return fail(h, GAMMA_HIP_EINVAL, "term filter on an unknown column");
        if (tf.n_items < 0 || tf.n_items > gh::kMaxTermItems || tf.op < 0 || tf.op > 2)
            return fail(h, GAMMA_HIP_EINVAL, "bad term filter");
        gh::TermDesc& td = f->term[i];
        td.off = it->second.d_off;
        td.tok = it->second.d_tok;
        td.n = it->second.ndocs;
        td.op = tf.op;
        td.n_items = tf.n_items;
        for (int k = 0; k < tf.n_items; k++) td.items[k] = tf.items[k];
    }
    if (!off_io && est_codes > 0 && f->n_field + f->n_term > 0 && f->n_range < gh::kMaxRange) {
        int64_t nbits = 0;   // beyond every column no clause matches (filter_dev.h), as beyond a range bitmap's max_doc
        for (int i = 0; i < f->n_field; i++) nbits = std::max<int64_t>(nbits, f->field[i].n);
        for (int i = 0; i < f->n_term; i++) nbits = std::max<int64_t>(nbits, f->term[i].n);
        const char* env = getenv("GAMMA_HIP_FILTER_BITMAP");   // 0: never, 1: always (tests), unset: by the estimate
        const bool want = env ? atoi(env) != 0 : est_codes >= 4 * nbits;
        if (want && nbits > 0 && nbits < ((int64_t)1 << 31)) {
            gh::FilterDesc g = *f;   // the clauses alone, on document ids
            g.has_range = 0;
            g.n_range = 0;
            g.del_bitmap = nullptr;
            g.del_bits = 0;
            g.vid2doc = nullptr;
            g.n_vid2doc = 0;
            GH_CHECK(h, h->w_fbits.ensure((size_t)((nbits + 63) / 64) * 8));
            gh::launch_filter_bitmap(h->stream, g, nbits, h->w_fbits.as<uint8_t>());
            gh::RangeDesc& r = f->range[f->n_range++];
            r.bitmap = h->w_fbits.as<uint8_t>();
            r.min_doc = 0;
            r.max_doc = (int32_t)(nbits - 1);
            r.min_aligned = 0;
            r.b_not_in = 0;
            f->has_range = 1;
            f->n_field = 0;
            f->n_term = 0;
        }
    }
    return GAMMA_HIP_OK;
}

int filt_ctx_single(H* h, const gh::FilterDesc& f, FiltCtx* c) {
    GH_CHECK(h, h->w_ftab.ensure(sizeof(gh::FilterDesc)));
    if (!h->ftab_valid || memcmp(&h->ftab_shadow, &f, sizeof(f)) != 0) {
        // the stream may still be reading the previous image: the copy is ordered behind it
        h->ftab_shadow = f;
        h->ftab_valid = true;
        GH_CHECK(h, hipMemcpyAsync(h->w_ftab.p, &h->ftab_shadow, sizeof(f), hipMemcpyHostToDevice, h->stream));
    }
    c->d_tab = h->w_ftab.as<gh::FilterDesc>();
    c->d_qf = nullptr;
    c->any_clause = f.has_range || f.n_field > 0 || f.n_term > 0;
    return GAMMA_HIP_OK;
}

int check_params(H* h, const gamma_hip_search_params* p, int nq, int k) {
    if (!p) return fail(h, GAMMA_HIP_EINVAL, "null params");
    if (nq < 0) return fail(h, GAMMA_HIP_EINVAL, "nq < 0");
    if (p->metric != GAMMA_HIP_METRIC_IP && p->metric != GAMMA_HIP_METRIC_L2)
        return fail(h, GAMMA_HIP_EINVAL, "bad metric");
    if (k > 4096) return fail(h, GAMMA_HIP_EINVAL, "k > 4096 unsupported");
    return GAMMA_HIP_OK;
}

// (the exact-ties choice of a request: gamma_hip_search.h)
int resolve_ties(H* h, const gamma_hip_search_params* p, gamma_hip_search_params* pp, bool in_range, const char* what) {
    *pp = *p;
    bool want = p->exact_ties != 0 ? p->exact_ties > 0 : h->exact_ties;
    if (want && !in_range) {
        if (p->exact_ties > 0) return fail(h, GAMMA_HIP_EUNSUPPORTED, what);
        h->ties_unhonoured.fetch_add(1, std::memory_order_relaxed);
        want = false;
    }
    pp->exact_ties = want ? 1 : -1;
    return GAMMA_HIP_OK;
}

// ---- the coarse quantizer (IVFPQ and IVFFLAT) ------------------------------------------
int coarse_join(H* h) {
    if (h->coarse_join_pending) {
        GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
        h->coarse_join_pending = false;
    }
    return GAMMA_HIP_OK;
}

int ivfpq_coarse(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, float* out_dis, int* out_probe, bool defer_join) {
    const int P = p->nprobe, d = h->d, nlist = h->nlist;
    hipStream_t s = h->stream;
    int mode = p->coarse_mode;
    if (mode < 0) mode = nq < 20 ? 0 : 1;  // faiss:utils/distances.cpp:303,346
    // large batches: no distance matrix (coarse.hip); with exact ties its rows with a tie near the cut are recomputed
    // and replayed through the reference's heap by the repair kernel
    const bool fused = mode == 1 && h->coarse_fused != 0 && gh::coarse_fused_supported(nq, d, nlist, P, tie_on(p));
    // the filter launch on the bf16 pipe (coarse.hip): needs the centroid image with every norm in the domain; turned off
    // for a while by the handle when the recent calls of this kind handed too many queries to the repair kernels
    bool bf16 = fused && h->coarse_fused == 1 && h->d_cc_img && h->cc_img_ok;
    if (bf16) {
        const uint64_t sig = ((uint64_t)nlist << 32) ^ ((uint64_t)P << 16) ^ (uint64_t)d ^ (1ull << 63);
        auto landed = [&]() {
            if (h->cbf_copy_pending && hipEventQuery(h->cbf_copy_ev) == hipSuccess) h->cbf_copy_pending = false;
            else if (h->cbf_copy_pending) (void)hipGetLastError();
            return !h->cbf_copy_pending;
        };
        if (sig != h->cbf_sig) {   // another kind of call: what was learnt does not carry over
            h->cbf_sig = sig;
            h->cbf_off_calls = 0;
            if (h->cbf_copy_pending) {
                (void)hipEventSynchronize(h->cbf_copy_ev);
                h->cbf_copy_pending = false;
            }
            h->cbf_seen[0] = h->pin_cbf_stat[0];
            h->cbf_seen[1] = h->pin_cbf_stat[1];
        }
        if (h->cbf_off_calls > 0) {
            if (--h->cbf_off_calls > 0) bf16 = false;   // (0: this call re-probes)
        } else if (landed()) {
            // the counters are cumulative and the pair is read only behind the copy that wrote it
            const unsigned long long u = h->pin_cbf_stat[0], n = h->pin_cbf_stat[1];
            const unsigned long long dn = n - h->cbf_seen[1], du = std::min(u - h->cbf_seen[0], dn);
            if (dn >= 2048) {
                h->cbf_seen[0] = u;
                h->cbf_seen[1] = n;
                if (8 * du > dn) {
                    h->cbf_off_calls = 256;
                    h->cbf_backoffs++;
                    bf16 = false;
                }
            }
        }
    }
    gh::CoarseFusedPlan plan;
    if (fused) {
        plan = gh::coarse_fused_plan(nq, nlist, P, h->coarse_cap, tie_on(p));
        GH_CHECK(h, h->w_mat.ensure(plan.bytes));
    } else {
        GH_CHECK(h, h->w_mat.ensure((size_t)nq * nlist * sizeof(float)));
    }
    if (!out_dis || !out_probe) {   // the workspace the scan reads
        GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nq * P * sizeof(float)));
        GH_CHECK(h, h->w_probe.ensure((size_t)nq * P * sizeof(int)));
        out_dis = h->w_coarse_dis.as<float>();
        out_probe = h->w_probe.as<int>();
    }
    StageScope t(h, GAMMA_HIP_STAGE_COARSE);
    if (fused) {
        static const bool no_side = getenv("GAMMA_HIP_NO_SIDE_STREAM") != nullptr;
        const bool side = tie_on(p) && defer_join && !no_side;
        gh::CoarseBf16 bf;
        if (bf16) {
            const size_t ny_pad = ((size_t)nlist + 63) / 64 * 64;
            bf.img = h->d_cc_img;
            bf.hc = reinterpret_cast<const float*>(static_cast<const char*>(h->d_cc_img) + ny_pad * d * 4);
            bf.yn_max = h->cc_norm_max;
            bf.stat = h->d_cbf_stat;
        }
        gh::launch_coarse_fused(s, plan, h->w_mat.p, d_x, nq, d, h->d_cc, nlist, h->d_cc_norms, P, out_dis, out_probe,
                                tie_on(p), h->d_tie_stats, side ? h->side : nullptr, h->ev_fork, h->ev_join,
                                bf16 ? &bf : nullptr);
        h->coarse_join_pending = side;
        if (bf16) {
            h->cbf_calls++;
            if (!h->cbf_copy_pending) {   // one copy in flight at a time: the pinned pair belongs to one state of the counters
                GH_CHECK(h, hipMemcpyAsync(h->pin_cbf_stat, h->d_cbf_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
                GH_CHECK(h, hipEventRecord(h->cbf_copy_ev, s));
                h->cbf_copy_pending = true;
            }
        }
        static const bool dbg = getenv("GAMMA_HIP_COARSE_DBG") != nullptr;
        if (dbg) {   // how many queries the strip lists could not hold (they went through the repair kernel)
            int n_ovf = 0;
            GH_CHECK(h, hipStreamSynchronize(s));
            GH_CHECK(h, hipMemcpy(&n_ovf, static_cast<char*>(h->w_mat.p) + plan.off_ovf, sizeof(int), hipMemcpyDeviceToHost));
            fprintf(stderr, "coarse fused: nlist %d nprobe %d sample %d strips %d: %d of %d queries repaired\n", nlist, P,
                    plan.sample, plan.nseg, n_ovf, nq);
        }
        return GAMMA_HIP_OK;
    }
    if (mode == 0) {
        gh::launch_pairwise(s, true, d_x, nq, d, h->d_cc, nlist, h->w_mat.as<float>(), nlist);
    } else {
        // query norms: fused into the MFMA kernel (xn = nullptr) when a tile holds whole rows (d <= 128); longer rows
        // get them from their own pass -- inside the K-slab loop they cost a fifth of the kernel (d = 768: 3.46 -> 2.72 ms
        // per 8192 x 16384 with the conflict-free staging)
        const float* xn = nullptr;
        if (d > 128) {
            GH_CHECK(h, h->w_xn.ensure((size_t)nq * sizeof(float)));
            gh::launch_row_norms(s, d_x, nq, d, h->w_xn.as<float>());
            xn = h->w_xn.as<float>();
        }
        gh::launch_l2_gemmform(s, d_x, nq, d, h->d_cc, nlist, xn, h->d_cc_norms,
                               h->w_mat.as<float>(), nlist, true);
    }
    if (tie_on(p)) GH_CHECK(h, h->w_tieflag.ensure((size_t)nq));
    static const bool no_side = getenv("GAMMA_HIP_NO_SIDE_STREAM") != nullptr;
    const bool side = tie_on(p) && defer_join && !no_side;
    h->coarse_join_pending = gh::launch_coarse_select(s, h->w_mat.as<float>(), nlist, nq, P, out_dis, out_probe,
                                                      tie_on(p) ? h->w_tieflag.as<uint8_t>() : nullptr, h->d_tie_stats,
                                                      side ? h->side : nullptr, h->ev_fork, h->ev_join);
    return GAMMA_HIP_OK;
}

// ---- IVFPQ stage A: coarse + tables + scan + top-R + ids ------------------------------
// results: w_cand_dis [nq*R] (ADC distance, best first, sentinel pad), w_cand_ids [nq*R]
// What runs -- probes per workgroup, bounded or not, which filter pass over how many groups and slices, the slab stride -- is
// decided by gh::ScanPlan from a gh::ScanShape (scan_plan.h / .cpp: every threshold and switch of the stage); whether an
// eligible call runs bounded is BoundFeedback's answer (gamma_hip_internal.h).  The functions here carry the plan out.

// what the plan depends on, as plain values
static gh::ScanShape scan_shape(const H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nq, int R, bool shard,
                                bool compacted, const BoundXchg* bx) {
    gh::ScanShape sh;
    sh.nq = nq;
    sh.P = p->nprobe;
    sh.R = R;
    sh.M = h->M;
    sh.nlist = h->nlist;
    sh.max_list_len = h->max_list_len;
    sh.q_stride_cap = h->q_stride_cap;
    sh.l2 = p->metric == GAMMA_HIP_METRIC_L2;
    sh.pq4 = h->ksub == gh::kPq4Ksub;
    sh.table_mode = h->table_mode;
    sh.have_sums = h->d_sums && h->d_t2max;
    sh.prefiltered = h->prefiltered;
    sh.cmp_has_sums = h->cmp_has_sums;
    sh.cmp_by_clause = h->cmp_by_clause;
    sh.any_clause = fc.any_clause;
    sh.per_query_filters = fc.d_qf != nullptr;
    sh.rejects = (h->d_bitmap && h->bitmap_any) || h->n_moved > 0;
    sh.shard = shard;
    sh.compacted = compacted;
    sh.two_phase = bx && bx->two_phase;
    if (sh.two_phase) sh.G1 = bx->G1;
    sh.scan_bound = h->scan_bound;
    sh.sort_queries = h->sort_queries && h->d_list_rank;
    sh.lists = gh::scan_list_stats(h->ntotal, h->nlist, h->h_list_len.data(), h->h_list_mask.empty() ? nullptr : h->h_list_mask.data(), shard);
    return sh;
}

// the arguments every scan launch of a call shares (kernels.h ScanArgs); a call site adds its probe groups, bound, fused
// codebook, repair list or unit mode
static gh::ScanArgs scan_args(H* h, bool l2, const FiltCtx& fc, int nq, int P, const float* d_x, const float* dis0, int64_t q_stride,
                              int need_ids) {
    gh::ScanArgs a;
    a.l2 = l2;
    a.x = d_x;
    a.nq = nq;
    a.d = h->d;
    a.M = h->M;
    a.P = P;
    a.probe_list = h->w_probe.as<int>();
    a.coarse_dis = dis0;
    a.cc = h->d_cc;
    a.st2 = h->scan_st2(l2);
    a.T2 = h->d_T2;
    a.list_off = h->d_list_off;
    a.list_len = h->d_list_len;
    a.list_mask = h->d_list_mask;
    a.nlist = h->nlist;
    a.codes = h->d_codes;
    a.ids = h->d_ids;
    a.pair_off = h->w_pair_off.as<int>();
    a.q_stride = q_stride;
    a.out = h->w_dist.as<float>();
    a.ftab = fc.d_tab;
    a.qfil = fc.d_qf;
    a.need_ids = need_ids;
    return a;
}

// the consumer probes of a bounded scan list-major over byte tables (q8scan.hip), behind the producers' launch
static int scan_list_major(H* h, const gh::ScanPlan& pl, const gh::ScanShape& sh, const gh::ScanBound& sb, const FiltCtx& fc,
                           const float* d_x, const float* dis0) {
    const int nq = sh.nq, P = sh.P, M = sh.M, nlist = sh.nlist;
    GH_CHECK(h, h->w_q8.ensure((size_t)nq * M * 256));
    GH_CHECK(h, h->w_q8meta.ensure((size_t)nq * 4 * sizeof(float)));
    GH_CHECK(h, h->w_q8cand.ensure((size_t)nq * gh::q8_cand_cap(nq) * sizeof(uint32_t)));
    GH_CHECK(h, h->w_q8int.ensure(gh::q8_int_words(nq, P, pl.G, nlist) * sizeof(int)));
    gh::Q8Args qa;
    qa.nq = nq; qa.P = P; qa.G = pl.G; qa.M = M; qa.nlist = nlist;
    qa.mean_len = sh.lists.mean_len;
    qa.probe_list = h->w_probe.as<int>();
    qa.coarse_dis = dis0;
    qa.st2 = h->w_st2.as<float>();
    if (sh.shard && !gh::ScanSwitches::get().no_q8_demand) qa.xd = d_x;
    qa.pqc = h->d_pqc;
    qa.d = h->d;
    qa.T2 = h->d_T2;
    qa.t2max = h->d_t2max;
    qa.sums = h->d_sums;
    qa.codes = h->d_codes;
    qa.ids = h->d_ids;
    qa.list_off = h->d_list_off;
    qa.list_len = h->d_list_len;
    qa.list_mask = h->d_list_mask;
    qa.pair_off = h->w_pair_off.as<int>();
    qa.ready = sb.ready;
    qa.ftab = fc.d_tab;
    qa.need_ids = pl.need_ids;
    qa.surv = sb.surv;
    qa.gcnt = sb.gcnt;
    qa.cnt_stride = pl.nsl;
    qa.slice_cap = pl.cap;
    qa.rq_list = sb.rq_list;
    qa.rq_count = sb.rq_count;
    qa.q8 = h->w_q8.as<uint8_t>();
    qa.meta = reinterpret_cast<float4*>(h->w_q8meta.p);
    qa.cand = h->w_q8cand.as<uint32_t>();
    qa.iwork = h->w_q8int.as<int>();
    gh::launch_q8_consumers(h->stream, qa);
    return GAMMA_HIP_OK;
}

// GAMMA_HIP_BOUND_DBG=1: the bounded scan's statistics of the 9th .. 14th call; =shard: of list-shard calls only
// (synchronises the stream)
static void scan_bound_dump(H* h, bool shard, int nq, const gh::ScanBound& sb, const gh::ScanPlan& pl) {
    static const bool dbg_any = getenv("GAMMA_HIP_BOUND_DBG") != nullptr;
    static const bool dbg_shard = dbg_any && getenv("GAMMA_HIP_BOUND_DBG")[0] == 's';
    static const int dbg_from = 8;
    static int shown = 0;
    if (!(dbg_any && (!dbg_shard || shard) && shown++ >= dbg_from && shown <= dbg_from + 5)) return;
    std::vector<uint8_t> hf(nq);
    std::vector<int> hc((size_t)nq * pl.nsl);
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemcpy(hf.data(), h->w_sflag.p, nq, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hc.data(), sb.gcnt, hc.size() * sizeof(int), hipMemcpyDeviceToHost);
    std::vector<unsigned long long> hr(nq);
    (void)hipMemcpy(hr.data(), sb.ready, (size_t)nq * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    int64_t nf = 0, tot = 0, mx = 0, nobound = 0;
    for (int i = 0; i < nq; i++) {
        nf += hf[i];
        nobound += (hr[i] >> 32) != 1ull;
    }
    for (size_t i = 0; i < hc.size(); i++) {
        tot += hc[i];
        mx = std::max<int64_t>(mx, hc[i]);
    }
    unsigned long long timeouts = 0;
    (void)hipMemcpy(&timeouts, h->bound_fb.d_timeouts(), sizeof(timeouts), hipMemcpyDeviceToHost);
    fprintf(stderr, "scan bound: %lld of %d queries unfiltered (%lld without a bound), survivors per query mean %.1f, "
            "per slice max %lld; G %d, %d groups, %d slices, q_stride %lld; consumers that gave up waiting so far %llu\n",
            (long long)nf, nq, (long long)nobound, (double)tot / nq, (long long)mx, pl.G, pl.PGN, pl.nsl, (long long)pl.q_stride, timeouts);
}

int ivfpq_stage_a(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nq,
                  const float* d_x, int R, const float* pre_dis, const int* pre_probe,
                  bool shard, float* out_dis, int64_t* out_ids, BoundXchg* bx) {
    const int P = p->nprobe, d = h->d, M = h->M, nlist = h->nlist;
    const bool two = bx && bx->two_phase;
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    // 4-bit codes (pq4.hip) take ONE path: shared coarse quantizer, k_pq4_ip_table, pair offsets, k_ivfpq4_scan_pair
    // unbounded, the unfiltered selection -- the bounded scan with its feedback, fused / residual tables and the byte
    // passes (cf, c8, q8) are 8-bit kernels and the plan gates them off
    const bool pq4 = h->ksub == gh::kPq4Ksub;
    if (pq4 && (shard || bx)) return pq4_refuse(h, "a list-shard search");
    hipStream_t s = h->stream;
    // this call reads the lists through the version of their (offset, length) tables that is current now:
    // behind the writer's copies (ver_ev), and the version is not reused before the kernels below are done (rd_ev)
    const int ver = h->cur_ver;
    GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
    GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nq * P * sizeof(float)));
    GH_CHECK(h, h->w_probe.ensure((size_t)nq * P * sizeof(int)));
    GH_CHECK(h, h->w_pair_off.ensure((size_t)nq * (P + 1) * sizeof(int)));
    GH_CHECK(h, h->w_pair_base.ensure((size_t)nq * P * sizeof(int64_t)));
    GH_CHECK(h, h->w_qtotal.ensure((size_t)nq * sizeof(int)));
    GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq * R * sizeof(int)));
    // the top-R table goes to the workspace (stage B reads it there) or straight into the caller's
    // buffers (sharded search: 12 B x R per query would otherwise be copied once more)
    if (!out_dis) {
        GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq * R * sizeof(float)));
        out_dis = h->w_cand_dis.as<float>();
    }
    if (!out_ids) {
        GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq * R * sizeof(int64_t)));
        out_ids = h->w_cand_ids.as<int64_t>();
    }
    const bool compacted = shard && pre_dis && pre_probe;
    if (pre_dis && pre_probe) {
        if (shard) {
            // dense probe groups for the owned lists (kernels.hip, k_compact_probes)
            gh::launch_compact_probes(s, pre_probe, pre_dis, nq, two ? bx->P_in : P, h->d_list_len, h->d_list_mask, nlist,
                                      h->w_probe.as<int>(), h->w_coarse_dis.as<float>(), P);
        } else {
            GH_CHECK(h, hipMemcpyAsync(h->w_coarse_dis.p, pre_dis, (size_t)nq * P * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
            GH_CHECK(h, hipMemcpyAsync(h->w_probe.p, pre_probe, (size_t)nq * P * sizeof(int),
                                       hipMemcpyDeviceToDevice, s));
        }
    } else {
        GH_TRY(ivfpq_coarse(h, p, nq, d_x, nullptr, nullptr, /*defer_join=*/true));
    }
    h->scan_pairs += (int64_t)nq * P;
    // the plan, in two halves around the feedback's answer
    const gh::ScanSwitches& sw = gh::ScanSwitches::get();
    const gh::ScanShape sh = scan_shape(h, p, fc, nq, R, shard, compacted, bx);
    gh::ScanPlan pl = gh::scan_plan_groups(sh, sw);
    bool bounded = pl.bound_eligible;
    if (bounded)
        GH_CHECK(h, h->bound_fb.begin(s, gh::BoundFeedbackState::signature(P, R, l2, fc.any_clause, shard), !sw.no_bound_feedback, &bounded));
    gh::scan_plan_passes(pl, sh, sw, bounded);
    const int G = pl.G, PGN = pl.PGN, PGM = pl.PGM, nsl = pl.nsl, cap = pl.cap;
    const int64_t q_stride = pl.q_stride;
    // exact ties (ties.hip): queries whose top-R cut goes through a group of equal ADC distances are marked here
    // and redone by the replay at the end of stage B
    h->tie = H::TieCtx();
    // (a shard marks the cut ties of its own top-R too: the merge at the slice's owner asks for them,
    //  gamma_hip_ivfpq_shard_cut_flags)
    h->tie.on = tie_on(p);
    h->shard_cut_nq = (shard && h->tie.on) ? nq : 0;
    h->shard_cut_chunked = false;
    // the bounded scan's per-call state (repair list, ready words, survivor counts) is sized here, before the pair offsets,
    // whose kernel clears it together with the tie flags -- one launch instead of four fills in front of the scan
    unsigned long long* ready = nullptr;
    int* fl_count = nullptr;   // the fall-through list: count | list
    if (bounded) {
        GH_CHECK(h, h->w_scnt.ensure(pl.scnt_bytes));
        GH_CHECK(h, h->w_sflag.ensure((size_t)nq));
        GH_CHECK(h, h->w_surv.ensure((size_t)nq * nsl * cap * sizeof(unsigned long long)));
        ready = reinterpret_cast<unsigned long long*>(h->w_scnt.as<char>() + pl.ready_off);
        fl_count = reinterpret_cast<int*>(h->w_scnt.as<char>() + pl.fl_off);
    }
    const int* qperm = nullptr;
    {
        StageScope t(h, GAMMA_HIP_STAGE_TABLES);
        if (pq4) {
            GH_CHECK(h, h->w_st2.ensure((size_t)nq * M * gh::kPq4Ksub * sizeof(float)));
            gh::launch_pq4_ip_table(s, d_x, nq, d, M, h->d_pqc, h->w_st2.as<float>());
        } else if (!pl.fuse_ip && !pl.res) {
            GH_CHECK(h, h->w_st2.ensure((size_t)nq * M * 256 * sizeof(float)));
            gh::launch_pq_ip_table(s, d_x, nq, d, M, h->d_pqc, h->w_st2.as<float>());
        }
        GH_TRY(coarse_join(h));
        // a deferred replay of the previous call / chunk reads what is written from here on (flag lists, pair offsets,
        // slab, survivor slices, candidate tables): it has had the coarse quantizer and the tables to finish behind
        GH_TRY(replay_join(h));
        if (h->tie.on) {
            GH_CHECK(h, h->w_tcut.ensure((size_t)nq));
            GH_CHECK(h, h->w_tlist.ensure(((size_t)nq + 1) * sizeof(int)));   // count | list[nq]
        }
        gh::PairZero pz;
        int* qo_bins = nullptr;
        if (pl.order) {   // the queries run in spatial order (kernels.hip)
            GH_CHECK(h, h->w_qperm.ensure((size_t)2 * nq * sizeof(int)));   // qperm | qkey
            if (gh::query_order_grid(nq)) {
                if (!h->w_qbins.p) {   // histogram | cursors; every call leaves the histogram zero
                    GH_CHECK(h, h->w_qbins.ensure((size_t)2 * gh::query_order_bins() * sizeof(int)));
                    GH_CHECK(h, hipMemsetAsync(h->w_qbins.p, 0, (size_t)2 * gh::query_order_bins() * sizeof(int), s));
                }
                qo_bins = h->w_qbins.as<int>();
                pz.qo_rank = h->d_list_rank;
                pz.qo_key = h->w_qperm.as<int>() + nq;
                pz.qo_bins = qo_bins;
            }
        }
        if (h->tie.on) {
            pz.bytes = h->w_tcut.as<uint8_t>();
            pz.count_a = h->w_tlist.as<int>();
        }
        if (bounded) {
#ifdef GH_SCAN_TIMING   // timing experiments with INVALID results: only in a library built for them (-DGH_SCAN_TIMING)
            static const int scan_dbg_part = getenv("GAMMA_HIP_SCAN_PART") ? atoi(getenv("GAMMA_HIP_SCAN_PART")) : 0;
            // (timing experiment 3: every other call runs the consumers alone, on the bounds of the call before)
            static std::atomic<int> scan_dbg_calls{0};
            h->scan_dbg_now = scan_dbg_part == 3 ? ((scan_dbg_calls.fetch_add(1) & 1) ? 2 : 0) : scan_dbg_part;
#endif
            pz.words = h->scan_dbg_now == 2 ? nullptr : ready;
            pz.count_b = h->w_scnt.as<int>();
            pz.count_c = fl_count;
        }
        gh::launch_pair_offsets(s, h->w_probe.as<int>(), nq, P, h->d_list_len, h->d_list_mask, nlist,
                                h->w_pair_off.as<int>(), h->w_qtotal.as<int>(),
                                h->profile == 1 ? h->d_scan_codes : nullptr, h->d_list_off,
                                h->w_pair_base.as<int64_t>(), &pz);
        if (pl.order) {
            gh::launch_query_order(s, h->w_probe.as<int>(), nq, P, h->d_list_rank, nlist,
                                   h->w_qperm.as<int>() + nq, h->w_qperm.as<int>(), qo_bins, qo_bins != nullptr);
            qperm = h->w_qperm.as<int>();
        }
        h->last_qperm = qperm;   // stage B runs the re-rank in the same order
    }
    GH_CHECK(h, h->w_dist.ensure((size_t)nq * q_stride * sizeof(float)));
    // dis0 of every (query, probe) pair: the coarse distance (L2) or <x_q, centroid> (inner product)
    const float* dis0 = h->w_coarse_dis.as<float>();
    if (!l2) {
        StageScope t(h, GAMMA_HIP_STAGE_TABLES, false);
        GH_CHECK(h, h->w_pair_ip.ensure((size_t)nq * P * sizeof(float)));
        gh::launch_pair_ip(s, d_x, h->d_cc, h->w_probe.as<int>(), nq, P, d, nlist, h->w_pair_ip.as<float>());
        dis0 = h->w_pair_ip.as<float>();
    }
    // one scan launch: probe groups [pg_lo, pg_lo + pg_cnt) of every query, G probes each
    gh::ScanArgs sa = scan_args(h, l2, fc, nq, P, d_x, dis0, q_stride, pl.need_ids);
    sa.G = G;
    sa.qperm = qperm;
    auto scan = [&](int pg_lo, int pg_cnt, int sparse, const gh::ScanBound* bound, const float* pqc_fused) {
        gh::ScanArgs a = sa;
        a.pg_lo = pg_lo;
        a.pg_cnt = pg_cnt;
        a.sparse = sparse;
        a.bound = bound;
        a.pqc_fused = pqc_fused;
        gh::launch_ivfpq_scan_pair(s, a);
    };
    const float* pqc = pl.fuse_ip ? h->d_pqc : nullptr;
    if (!bounded) {
        {
            StageScope t(h, GAMMA_HIP_STAGE_SCAN, true);
            if (pq4)
                gh::launch_ivfpq4_scan_pair(s, l2, nq, M, P, h->w_probe.as<int>(), dis0, h->w_st2.as<float>(), h->d_T2, h->d_list_off,
                                            h->d_list_len, h->d_list_mask, nlist, h->d_codes, h->d_ids, h->w_pair_off.as<int>(),
                                            q_stride, h->w_dist.as<float>(), fc.d_tab, fc.d_qf, pl.need_ids, qperm, G, PGN);
            else
                scan(0, PGN, shard ? 1 : 0, nullptr, pqc);
        }
        StageScope t(h, GAMMA_HIP_STAGE_SELECT);
        gh::launch_select_topk(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), 0,
                               (int)std::min<int64_t>(q_stride, 1 << 30), nq, R,
                               out_dis, h->w_cand_pos.as<int>());
        gh::launch_map_candidates(s, h->w_cand_pos.as<int>(), nq, R, P, h->w_probe.as<int>(),
                                  h->w_pair_off.as<int>(), h->d_list_off, h->d_ids,
                                  out_ids);
        if (h->tie.on)
            gh::launch_flag_cut_ties(s, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nq, R, out_dis,
                                     h->w_cand_pos.as<int>(), h->w_tcut.as<uint8_t>());
    } else {
        gh::ScanBound sb = {};   // (every field starts at 0: part, dbg_part, c8 ...)
        sb.ready = ready;
        sb.surv = h->w_surv.as<unsigned long long>();
        sb.gcnt = reinterpret_cast<int*>(h->w_scnt.as<char>() + pl.gcnt_off);
        sb.K = R;
        sb.cnt_stride = nsl;
        // consumer groups with a bound keep only their survivors; what the unfiltered fallback and the tie replay of a
        // query without a usable bound need is stored by the repair launch below
        sb.store_all = 0;
        sb.rq_count = h->w_scnt.as<int>();
        sb.rq_list = h->w_scnt.as<int>() + 1;
        sb.sums = pl.cf_ok ? h->d_sums : nullptr;
        sb.t2max = pl.cf_ok ? h->d_t2max : nullptr;
        sb.t2max_all = h->t2max_all;
        sb.pair_base = h->w_pair_base.as<int64_t>();
        sb.cf_span = pl.cf_span;
        sb.timeouts = h->bound_fb.d_timeouts();
        sb.slice_cap = cap;
        sb.c8 = pl.c8;
        sb.dbg_part = h->scan_dbg_now;
        // two-phase shard search: the producers' bounds out, the reduced (global) bounds back into the ready words
        auto exchange = [&]() -> int {
            gh::launch_bound_export(s, l2, sb.ready, nq, bx->d_bound);
            GH_TRY(bx->reduce(h, nq, l2));
            gh::launch_bound_import(s, l2, bx->d_bound, nq, sb.ready);
            return GAMMA_HIP_OK;
        };
        if (!pl.q8_ok && two) {
            {   // phase 1: the producers alone (one group per query; the plain bounded kernel)
                StageScope t(h, GAMMA_HIP_STAGE_SCAN, true);
                scan(0, 1, 1, &sb, pqc);
            }
            GH_TRY(exchange());
            if (PGM > 1) {   // phase 2: the consumers alone, against the global bounds
                StageScope t(h, GAMMA_HIP_STAGE_SCAN, false);
                sb.part = 2;
                scan(0, PGM, shard ? 1 : 0, &sb, pqc);
                sb.part = 0;
            }
        } else if (!pl.q8_ok) {
            StageScope t(h, GAMMA_HIP_STAGE_SCAN, true);
            scan(0, PGM, shard ? 1 : 0, &sb, pqc);
        } else {
            // producers (the first G probes: exact, they publish the bounds), then the other probes list-major over byte
            // tables -- all of it one "scan launch" for the stage clock and the roofline figure
            StageScope t(h, GAMMA_HIP_STAGE_SCAN, true);
            scan(0, 1, 0, &sb, nullptr);
            if (two) GH_TRY(exchange());   // (the list-major pass below reads the ready words: now the global bounds)
            GH_TRY(scan_list_major(h, pl, sh, sb, fc, d_x, dis0));
        }
        // the queries that fall through the bound (a handful of a batch: ~5 of 16384 at C3): the launch behind k_select_final
        // and the repair scan walks its list of them, as the repair launch walks rq_list
        const gh::RowList fell(fl_count + 1, fl_count);
        StageScope t(h, GAMMA_HIP_STAGE_SELECT);
        gh::launch_select_final(s, l2, sb.surv, sb.gcnt, nsl, cap, sb.ready, h->w_pair_off.as<int>(), P, nq, R,
                                h->w_pair_base.as<int64_t>(), h->d_ids,
                                h->w_sflag.as<uint8_t>(), out_dis,
                                h->w_cand_pos.as<int>(), out_ids, h->tie.on ? h->w_tcut.as<uint8_t>() : nullptr,
                                h->d_tie_stats, sb.rq_list, sb.rq_count, h->bound_fb.d_slot(),
                                fl_count + 1, fl_count);
        GH_CHECK(h, h->bound_fb.end(s));
        if (PGN > 1 && !sb.store_all) {
            // queries the slices could not answer: their consumer groups are scored again, distances stored
            StageScope t2(h, GAMMA_HIP_STAGE_SCAN, false);
            gh::ScanArgs a = sa;
            a.qperm = nullptr;
            a.pg_lo = 1;
            a.pg_cnt = PGN - 1;
            a.sparse = shard ? 1 : 0;
            a.rq_list = sb.rq_list;
            a.rq_count = sb.rq_count;
            gh::launch_ivfpq_scan_pair(s, a);
        }
        // (one launch: a listed row's workgroup selects it, flags a tied cut and looks its ids up)
        gh::RowTail tail;
        tail.tflag = h->tie.on ? h->w_tcut.as<uint8_t>() : nullptr;
        tail.P = P;
        tail.probe_list = h->w_probe.as<int>();
        tail.pair_off = h->w_pair_off.as<int>();
        tail.list_off = h->d_list_off;
        tail.ids = h->d_ids;
        tail.cand_ids = out_ids;
        gh::launch_select_topk(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), 0,
                               (int)std::min<int64_t>(q_stride, 1 << 30), nq, R,
                               out_dis, h->w_cand_pos.as<int>(), fell, &tail);
        if (h->tie.on) {
            h->tie.bounded = true;
            h->tie.nsl = nsl;
            h->tie.cap = cap;
        }
        scan_bound_dump(h, shard, nq, sb, pl);
    }
    h->tie.G = G;
    h->tie.q_stride = q_stride;
    GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
    h->rd_set[ver] = true;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

// ---- the re-rank filter (rerank_filter.hip; the handle's rf) ---------------------------------------------------------------
// Does this fused re-rank run behind the filter?  Only over a dense fp32 store with rows of a multiple of 16 floats; the first
// call that qualifies builds the image (one pass for the per-dimension ranges, one that quantises: on the search stream, the
// caller holds mu so no writer is at work).  The handle's feedback may turn a call down: coarse quantizer's rule and plumbing.
static int rerank_filter_begin(H* h, bool l2, int nq, int R, int k, bool* use) {
    H::RerankImage& rf = h->rf;
    *use = false;
    if (rf.mode == 0 || (rf.mode == 1 && nq < H::RerankImage::kAutoMinNq)) return GAMMA_HIP_OK;
    if (!h->raw_f32() || h->raw_sparse || h->nraw <= 0 || !gh::rerank_filter_shape_ok(h->raw_d, R, k)) return GAMMA_HIP_OK;
    hipStream_t s = h->stream;
    const int d = h->raw_d;
    if (!rf.on) {
        if (!rf.par) {
            GH_CHECK(h, hipMalloc((void**)&rf.par, gh::rerank_image_par_bytes(gh::kRerankFilterMaxD)));
            GH_CHECK(h, hipMalloc((void**)&rf.d_stat, gh::rerank_filter_stat_bytes()));
            GH_CHECK(h, hipMemsetAsync(rf.d_stat, 0, gh::rerank_filter_stat_bytes(), s));
            GH_CHECK(h, hipHostMalloc((void**)&rf.pin_stat, gh::rerank_filter_stat_bytes(), hipHostMallocDefault));
            memset(rf.pin_stat, 0, gh::rerank_filter_stat_bytes());
            GH_CHECK(h, hipEventCreateWithFlags(&rf.copy_ev, hipEventDisableTiming));
            GH_CHECK(h, hipEventCreateWithFlags(&rf.built, hipEventDisableTiming));
        }
        GH_TRY(rerank_image_reserve(h, h->raw_cap()));
        gh::launch_rerank_image_params(s, h->raw_f32(), h->nraw, d, rf.par);
        gh::launch_rerank_image_rows(s, h->raw_f32(), nullptr, 0, h->nraw, d, rf.par, rf.rows.as<uint8_t>(), rf.aux.as<float>(), h->nraw);
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipEventRecord(rf.built, s));
        rf.on = true;
    }
    const uint64_t sig = ((uint64_t)R << 40) ^ ((uint64_t)k << 20) ^ ((uint64_t)d << 1) ^ (l2 ? 1u : 0u) ^ (1ull << 63);
    auto sums = [&](unsigned long long* out2) {
        out2[0] = 0;
        for (int i = 0; i < gh::kRerankFilterStatLines; i++) out2[0] += rf.pin_stat[16 * i];
        out2[1] = rf.cand_at_copy;   // (the copy stands behind the launch that brought the candidates to this count)
    };
    if (sig != rf.sig) {   // another kind of call: what was learnt does not carry over
        rf.sig = sig;
        rf.off_calls = 0;
        if (rf.copy_pending) {
            (void)hipEventSynchronize(rf.copy_ev);
            rf.copy_pending = false;
        }
        sums(rf.seen);
    }
    *use = true;
    if (rf.off_calls > 0) {
        if (--rf.off_calls > 0) *use = false;   // (0: this call probes again)
    } else {
        if (rf.copy_pending && hipEventQuery(rf.copy_ev) == hipSuccess) rf.copy_pending = false;
        else if (rf.copy_pending) (void)hipGetLastError();
        if (!rf.copy_pending) {   // the words are read only behind the copy that wrote them
            unsigned long long now[2];
            sums(now);
            const unsigned long long dn = now[1] - rf.seen[1], du = std::min(now[0] - rf.seen[0], dn);
            if (dn >= 4096) {
                rf.seen[0] = now[0];
                rf.seen[1] = now[1];
                if (2 * du > dn) {
                    rf.off_calls = 256;
                    rf.backoffs++;
                    *use = false;
                }
            }
        }
    }
    return GAMMA_HIP_OK;
}
// behind a filtered launch: the counters as of this call for a later call's decision (one copy in flight at a time)
static int rerank_filter_end(H* h, int64_t candidates) {
    H::RerankImage& rf = h->rf;
    rf.calls++;
    rf.cand += (unsigned long long)candidates;
    if (!rf.copy_pending) {
        GH_CHECK(h, hipMemcpyAsync(rf.pin_stat, rf.d_stat, gh::rerank_filter_stat_bytes(), hipMemcpyDeviceToHost, h->stream));
        rf.cand_at_copy = rf.cand;
        GH_CHECK(h, hipEventRecord(rf.copy_ev, h->stream));
        rf.copy_pending = true;
    }
    return GAMMA_HIP_OK;
}

// ---- stage B: compute_dis (gamma_index_ivfpq.cc:642-697) ------------------------------
int ivfpq_stage_b(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int R, int k,
                  const float* cand_dis, const int64_t* cand_ids, float* d_distances,
                  int64_t* d_labels, const int* qperm, int tie_mode) {
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    const float neutral = neutral_of(l2);
    hipStream_t s = h->stream;
    StageScope t(h, GAMMA_HIP_STAGE_RERANK);
    // exact ties: the final-stage kernel lists the queries with a tie among their first k+1 distances (or with a
    // tied top-R cut, stage A) and k_tie_replay redoes those the way the reference's heaps do (ties.hip)
    const bool ties = (tie_mode == 1 && h->tie.on) || tie_mode == 2;
    gh::TieFlags tf;
    if (ties) {
        tf.cut = h->w_tcut.as<uint8_t>();
        tf.count = h->w_tlist.as<int>();
        tf.list = h->w_tlist.as<int>() + 1;
        tf.stats = h->d_tie_stats;
    }
    auto replay = [&]() {
        gh::TieReplayArgs a;
        a.list = tf.list;
        a.count = tf.count;
        a.nq = nq;
        a.slab = h->w_dist.as<float>();
        a.q_stride = h->tie.q_stride;
        a.pair_off = h->w_pair_off.as<int>();
        a.pair_base = h->w_pair_base.as<int64_t>();
        a.ids = h->d_ids;
        a.P = p->nprobe;
        a.G = h->tie.G;
        const size_t rq_bytes = (((size_t)nq + 1) * sizeof(int) + 7) & ~(size_t)7;
        unsigned long long* ready = reinterpret_cast<unsigned long long*>(h->w_scnt.as<char>() + rq_bytes);
        a.ready = h->tie.bounded ? ready : nullptr;
        a.surv = h->w_surv.as<unsigned long long>();
        a.gcnt = reinterpret_cast<int*>(ready + nq);
        a.nsl = h->tie.nsl;
        a.slice_cap = h->tie.cap;
        a.x = d_x;
        a.d = h->d;
        a.rows = raw_rows_ref(h);
        a.nraw = h->nraw;
        a.R = R;
        a.k = k;
        a.has_rank = p->has_rank ? 1 : 0;
        a.min_score = p->min_score;
        a.max_score = p->max_score;
        a.neutral = neutral;
        a.cand_dis = const_cast<float*>(cand_dis);
        a.cand_ids = const_cast<int64_t*>(cand_ids);
        a.distances = d_distances;
        a.labels = d_labels;
        static const bool no_side = getenv("GAMMA_HIP_NO_SIDE_STREAM") != nullptr;
        if (h->defer_now && h->side2 && !no_side) {
            // beside whatever the search stream does next that does not touch the replay's inputs (replay_join)
            (void)hipEventRecord(h->ev_rfork, s);
            (void)hipStreamWaitEvent(h->side2, h->ev_rfork, 0);
            gh::launch_tie_replay(h->side2, l2, a);
            (void)hipEventRecord(h->ev_rdone, h->side2);
            h->replay_pending = true;
            h->replay_is_flat = false;
        } else {
            gh::launch_tie_replay(s, l2, a);
        }
    };
    if (p->has_rank) {
        if (!h->has_raw_rows() || h->raw_d != h->d) return fail(h, GAMMA_HIP_EINVAL, "has_rank needs the raw store");
        if (h->raw_sparse) return fail(h, GAMMA_HIP_EUNSUPPORTED, "has_rank on a handle that holds its shard's raw rows only: the exact distances travel with the candidates (gamma_hip_ivfpq_shard_exact / _merge_rerank_exact)");
        if (R <= 1024 && (nq >= 256 || ties)) {
            // one fused kernel: exact distances + top-k + output
            bool filt = false;
            GH_TRY(rerank_filter_begin(h, l2, nq, R, k, &filt));
            if (filt) {
                const int ran = gh::launch_rerank_topk_filtered(s, l2, d_x, nq, h->d, h->raw_f32(), h->nraw, h->rf.rows.as<uint8_t>(),
                                                                h->rf.aux.as<float>(), h->rf.par, cand_ids, R, k, p->min_score,
                                                                p->max_score, neutral, d_distances, d_labels, qperm,
                                                                ties ? &tf : nullptr, h->rf.d_stat, h->rf.form);
                if (ran) h->rf.last_form = ran;
                if (ran == 2) h->rf.wave_calls++;
                GH_TRY(rerank_filter_end(h, (int64_t)nq * R));
            } else {
                gh::launch_rerank_topk(s, l2, d_x, nq, h->d, raw_rows_ref(h), h->nraw, cand_ids, R, k, p->min_score,
                                       p->max_score, neutral, d_distances, d_labels, qperm, ties ? &tf : nullptr);
            }
            if (ties && tie_mode == 1) replay();
            GH_CHECK(h, hipGetLastError());
            return GAMMA_HIP_OK;
        }
        GH_CHECK(h, h->w_exact.ensure((size_t)nq * R * sizeof(float)));
        GH_CHECK(h, h->w_selv.ensure((size_t)nq * k * sizeof(float)));
        GH_CHECK(h, h->w_selp.ensure((size_t)nq * k * sizeof(int)));
        gh::launch_rerank_dist(s, l2, d_x, nq, h->d, raw_rows_ref(h), h->nraw, cand_ids, R, p->min_score,
                               p->max_score, h->w_exact.as<float>());
        gh::launch_select_topk(s, l2, h->w_exact.as<float>(), R, nullptr, R, R, nq, k,
                               h->w_selv.as<float>(), h->w_selp.as<int>());
        gh::launch_finalize_topk(s, h->w_selv.as<float>(), h->w_selp.as<int>(), nq, k, cand_ids, R, 0,
                                 neutral, d_distances, d_labels);
        if (ties) {
            // recall_num beyond 1024: the flags of the fused kernel, made here -- equal exact distances among the k selected
            // or at the k cut (the row of exact distances against the selection), or a tied top-R cut (stage A)
            GH_CHECK(h, h->w_textra.ensure((size_t)nq));
            GH_CHECK(h, hipMemsetAsync(h->w_textra.p, 0, (size_t)nq, s));
            gh::launch_flag_cut_ties(s, h->w_exact.as<float>(), R, nullptr, nq, k, h->w_selv.as<float>(), h->w_selp.as<int>(),
                                     h->w_textra.as<uint8_t>(), R, 1);
            gh::launch_tie_list(s, tf.cut, h->w_textra.as<uint8_t>(), nq, tf.list, tf.count, tf.stats);
            if (tie_mode == 1) replay();
        }
    } else {
        gh::launch_finalize_norank(s, cand_dis, cand_ids, nq, R, k, p->min_score, p->max_score, neutral,
                                   d_distances, d_labels, ties ? &tf : nullptr);
        if (ties && tie_mode == 1) replay();
    }
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

// ---- small batches (nq <= 512; measured cross-over with the regular chain ~1000): four or five launches instead of eleven ---------------------------------
// exact coarse distances + query tables | top-nprobe + slab offsets | scan | top-recall_num + ids + re-rank + top-k
// (kernels.hip k_small_coarse_ip, select.hip k_small_coarse_select / k_small_tail).  Each launch of the regular
// chain costs ~4 us of launch + drain at this size, whatever it computes.
bool ivfpq_small_ok(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nq, int R) {
    static const bool off = getenv("GAMMA_HIP_NO_SMALL_PATH") != nullptr;
    constexpr int max_nq = 512;   // (the section's header: the measured cross-over with the regular chain is ~1000)
    // exact coarse distances (faiss below 20 queries) come from the fused first kernel, which covers 16 queries; the
    // GEMM form (20 queries and more) from the regular matrix kernel
    // (a 4-bit handle takes the regular chain: the small path's fused kernels are 8-bit)
    return !off && h->ksub == 256 && h->small_path && nq >= 1 && nq <= max_nq &&
           p->nprobe <= 128 && R <= 1024 && !h->profile && !fc.d_qf && !h->d_list_mask &&
           h->nlist <= 16384 &&
           (int64_t)p->nprobe * std::max(1, h->max_list_len) <= (1 << 22) &&
           // long lists: beyond ~5e7 codes per call the regular chain's bound filter wins (full-size C4, 390 k codes per
           // query: 64 queries 0.46 ms against 1.04, 256 queries 1.63 against 1.33)
           // (raw_f32() is null on a float16, byte or sq8 raw store: its has_rank calls take the regular chain, whose stage B reads the narrow rows)
           (int64_t)nq * p->nprobe * (h->ntotal / std::max(1, h->nlist)) <= 48000000LL && (!p->has_rank || (h->raw_f32() && h->raw_d == h->d && !h->raw_sparse));
}

// d_x: the vectors that are quantised (a handle with an OPQ matrix: the rotated queries), d_xraw: the caller's, which the
// exact re-rank and the tie replay measure against the raw store
int ivfpq_small(H* h, const gamma_hip_search_params* p, const FiltCtx& fc, int nq, const float* d_x, const float* d_xraw, int R, int k,
                float* d_distances, int64_t* d_labels) {
    const int P = p->nprobe, d = h->d, M = h->M, nlist = h->nlist;
    hipStream_t s = h->stream;
    const int ver = h->cur_ver;
    GH_CHECK(h, hipStreamWaitEvent(s, h->ver_ev[ver], 0));
    GH_CHECK(h, h->w_mat.ensure((size_t)nq * nlist * sizeof(float)));
    GH_CHECK(h, h->w_st2.ensure((size_t)nq * M * 256 * sizeof(float)));
    GH_CHECK(h, h->w_coarse_dis.ensure((size_t)nq * P * sizeof(float)));
    GH_CHECK(h, h->w_probe.ensure((size_t)nq * P * sizeof(int)));
    GH_CHECK(h, h->w_pair_off.ensure((size_t)nq * (P + 1) * sizeof(int)));
    GH_CHECK(h, h->w_pair_base.ensure((size_t)nq * P * sizeof(int64_t)));
    GH_CHECK(h, h->w_qtotal.ensure((size_t)nq * sizeof(int)));
    GH_CHECK(h, h->w_cand_pos.ensure((size_t)nq * R * sizeof(int)));
    GH_CHECK(h, h->w_cand_dis.ensure((size_t)nq * R * sizeof(float)));
    GH_CHECK(h, h->w_cand_ids.ensure((size_t)nq * R * sizeof(int64_t)));
    const int64_t q_stride = slab_q_stride(h, P);
    GH_CHECK(h, h->w_dist.ensure((size_t)nq * q_stride * sizeof(float)));
    // (folding the selection into the first launch -- last workgroup done selects -- was tried: the device-scope
    // release / acquire it needs costs more than the launch it saves, 24 us against 4 + 8: the XCDs' L2s are
    // written back and invalidated either way)
    // long lists: the scan walks a work list of (query, probe, chunk of the list) units written by the selection kernel,
    // pieces of even size for a grid that fills the chip, instead of one workgroup per pair that runs for as long as its
    // list is (small_presel: tests force the path on short lists)
    int chunk_len = 0, max_units = 0;
    uint32_t* d_units = nullptr;
    int* d_nunits = nullptr;
    if (h->ntotal / std::max(1, nlist) > 1024 || h->max_list_len > 8192 || h->small_presel > 0) {
        chunk_len = 512;
        const int64_t mu = (int64_t)nq * P * (1 + (int64_t)h->max_list_len / chunk_len);
        max_units = (int)std::min<int64_t>(mu, INT32_MAX);
        GH_CHECK(h, h->w_lm_units.ensure((size_t)mu * sizeof(uint32_t)));
        GH_CHECK(h, h->w_lm_cnt.ensure(64));
        d_units = h->w_lm_units.as<uint32_t>();
        d_nunits = h->w_lm_cnt.as<int>();
    }
    if (p->coarse_mode == 1) {
        if (d_nunits) GH_CHECK(h, hipMemsetAsync(d_nunits, 0, sizeof(int), s));
        gh::launch_l2_gemmform(s, d_x, nq, d, h->d_cc, nlist, nullptr, h->d_cc_norms, h->w_mat.as<float>(), nlist, true);
        gh::launch_pq_ip_table(s, d_x, nq, d, M, h->d_pqc, h->w_st2.as<float>());
    } else if (!gh::launch_small_coarse_ip(s, d_x, nq, d, h->d_cc, nlist, h->w_mat.as<float>(), M, h->d_pqc,
                                           h->w_st2.as<float>(), d_nunits)) {
        // exact coarse distances for more than 16 queries (an explicit coarse_mode 0, or a combined batch of requests
        // that are each below faiss's 20-query switch): the regular chain's kernel, then the small chain
        if (d_nunits) GH_CHECK(h, hipMemsetAsync(d_nunits, 0, sizeof(int), s));
        gh::launch_pairwise(s, true, d_x, nq, d, h->d_cc, nlist, h->w_mat.as<float>(), nlist);
        gh::launch_pq_ip_table(s, d_x, nq, d, M, h->d_pqc, h->w_st2.as<float>());
    }
    const bool l2 = p->metric == GAMMA_HIP_METRIC_L2;
    if (!l2) GH_CHECK(h, h->w_pair_ip.ensure((size_t)nq * P * sizeof(float)));
    gh::launch_small_coarse_select(s, h->w_mat.as<float>(), nlist, nq, P, h->w_coarse_dis.as<float>(), h->w_probe.as<int>(),
                                   h->d_list_len, h->d_list_mask, h->d_list_off, h->w_pair_off.as<int>(),
                                   h->w_qtotal.as<int>(), h->w_pair_base.as<int64_t>(), d_x, h->d_cc, d,
                                   l2 ? nullptr : h->w_pair_ip.as<float>(), d_units, d_nunits, chunk_len,
                                   tie_on(p) ? 1 : 0, h->d_tie_stats);
    h->scan_pairs += (int64_t)nq * P;
    const int need_ids = (!h->prefiltered && (fc.any_clause || (h->d_bitmap && h->bitmap_any) || h->n_moved > 0)) ? 1 : 0;
    // one probe per workgroup, every probe; with a unit list: the work list of list chunks
    gh::ScanArgs sa = scan_args(h, l2, fc, nq, P, d_x, l2 ? h->w_coarse_dis.as<float>() : h->w_pair_ip.as<float>(), q_stride, need_ids);
    sa.pg_cnt = P;
    sa.rq_list = reinterpret_cast<const int*>(d_units);
    sa.rq_count = d_nunits;
    sa.chunk_len = chunk_len;
    sa.max_units = max_units;
    gh::launch_ivfpq_scan_pair(s, sa);
    const float neutral = neutral_of(l2);
    // long candidate rows (expected nprobe x 1.5 mean list lengths beyond what one workgroup keeps in registers): a first
    // selection over slices of the row by several workgroups per query, then the tail among their survivors
    const int smax = small_presel_slices(h, P, nq);
    if (smax > 0) {
        GH_CHECK(h, h->w_selv.ensure((size_t)nq * smax * R * sizeof(float)));
        GH_CHECK(h, h->w_selp.ensure(((size_t)nq * smax * R + (size_t)nq * smax) * sizeof(int)));   // + a cut flag per slice
    }
    // exact ties: a query with a tie at the recall_num or k cut is replayed through the reference's heaps inside the
    // tail kernel (tie_dev.h), from the whole slab row
    gh::TieReplayArgs tr;
    const bool ties = tie_on(p) && R <= gh::tie_small_max_k();   // (ivfpq_small_ok: recall_num <= 1024)
    if (ties) {
        tr.list = nullptr;
        tr.count = nullptr;
        tr.nq = nq;
        tr.slab = h->w_dist.as<float>();
        tr.q_stride = q_stride;
        tr.pair_off = h->w_pair_off.as<int>();
        tr.pair_base = h->w_pair_base.as<int64_t>();
        tr.ids = h->d_ids;
        tr.P = P;
        tr.G = 1;
        tr.ready = nullptr;
        tr.surv = nullptr;
        tr.gcnt = nullptr;
        tr.nsl = 0;
        tr.slice_cap = 0;
        tr.x = d_xraw;
        tr.d = d;
        tr.rows = gh::RowsRef{h->raw_f32()};   // (ivfpq_small_ok: fp32 rows or no re-rank)
        tr.nraw = h->nraw;
        tr.R = R;
        tr.k = k;
        tr.has_rank = p->has_rank ? 1 : 0;
        tr.min_score = p->min_score;
        tr.max_score = p->max_score;
        tr.neutral = neutral;
        tr.cand_dis = h->w_cand_dis.as<float>();
        tr.cand_ids = h->w_cand_ids.as<int64_t>();
        tr.distances = d_distances;
        tr.labels = d_labels;
    }
    gh::launch_small_tail(s, l2, h->w_dist.as<float>(), q_stride, h->w_qtotal.as<int>(), nq, R, P, h->w_probe.as<int>(),
                          h->w_pair_off.as<int>(), h->d_list_off, h->d_ids, h->w_cand_dis.as<float>(),
                          h->w_cand_pos.as<int>(), h->w_cand_ids.as<int64_t>(), p->has_rank ? 1 : 0, d_xraw, d, h->raw_f32(),
                          h->nraw, k, p->min_score, p->max_score, neutral, d_distances, d_labels, smax,
                          smax ? h->w_selv.as<float>() : nullptr, smax ? h->w_selp.as<int>() : nullptr, 0,
                          ties ? &tr : nullptr, h->d_tie_stats);
    h->tie = H::TieCtx();
    h->tie.G = 1;
    h->tie.q_stride = q_stride;
    h->last_qperm = nullptr;
    GH_CHECK(h, hipEventRecord(h->rd_ev[ver], s));
    h->rd_set[ver] = true;
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int ivfpq_check(H* h, const gamma_hip_search_params* p, int nq, int k) {
    GH_TRY(check_params(h, p, nq, k));
    if (!h->ivf_init || h->ivfflat) return fail(h, GAMMA_HIP_EINVAL, "ivfpq not initialised");
    if (!h->trained) return fail(h, GAMMA_HIP_ENOTTRAINED, "ivfpq not trained");
    if (p->nprobe <= 0 || p->nprobe > h->nlist) return fail(h, GAMMA_HIP_EINVAL, "nprobe out of range");
    if (std::max(p->recall_num, k) > 4096) return fail(h, GAMMA_HIP_EINVAL, "recall_num > 4096 unsupported");
    return GAMMA_HIP_OK;
}

int coarse_chunk(H* h, int nq) {
    const int64_t by_mat = (int64_t)(h->dist_budget_bytes / ((size_t)h->nlist * sizeof(float)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(by_mat, nq));
}
int scan_chunk(H* h, int nq, int P) {
    const int64_t q_stride = std::max<int64_t>(1, (int64_t)P * std::max(1, h->max_list_len));
    const int64_t by_dist = (int64_t)(h->dist_budget_bytes / (q_stride * sizeof(float)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(by_dist, nq));
}
int query_chunk(H* h, int nq, int P) { return std::min(coarse_chunk(h, nq), scan_chunk(h, nq, P)); }

int compact_lists_for_call(H* h, FiltCtx* fc, int64_t est, bool allowed, ListCompaction* lc) {
    const bool need = fc->any_clause || (h->d_bitmap && h->bitmap_any) || h->n_moved > 0;
    const char* env = getenv("GAMMA_HIP_LIST_COMPACT");
    const bool want = env ? atoi(env) != 0 : est >= 4 * std::max<int64_t>(1, h->ntotal);
    if (!(need && want && allowed && !fc->d_qf && !h->d_list_mask && h->arena_cap > 0)) return GAMMA_HIP_OK;
    // the shadow arena is an optimisation: without the memory for it the call runs over the lists as they are, testing
    // the predicate per scored code (same results)
    if (h->w_cmp_codes.ensure((size_t)h->arena_cap * h->code_size) != hipSuccess ||
        h->w_cmp_ids.ensure((size_t)h->arena_cap * sizeof(int64_t)) != hipSuccess ||
        h->w_cmp_len.ensure((size_t)h->nlist * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        h->w_cmp_codes.release();
        h->w_cmp_ids.release();
        return GAMMA_HIP_OK;
    }
    // the per-code sums of the scan's filter pass go along (same offsets), so the pass stays on over the shadow lists
    const bool with_sums = h->d_sums && h->w_cmp_sums.ensure((size_t)h->arena_cap * sizeof(float)) == hipSuccess;
    if (!with_sums) (void)hipGetLastError();
    // standing deletes (no clause of the call's own): the shadow lists of the last call are still right unless a writer
    // has run since -- Add / Update / Delete / bitmap / compaction all count in write_gen
    static const bool no_cache = getenv("GAMMA_HIP_NO_COMPACT_CACHE") != nullptr;
    const bool reuse = !no_cache && !fc->any_clause && h->cmp_gen == h->write_gen && h->cmp_sums_built == with_sums;
    GH_CHECK(h, hipStreamWaitEvent(h->stream, h->ver_ev[h->cur_ver], 0));   // the version's lists are in place
    if (!reuse) {
        GH_TRY(replay_join(h));   // a deferred replay may still read the shadow lists of the previous call
        StageScope t(h, GAMMA_HIP_STAGE_SCAN, false);   // profiled as part of the scan it shortens
        gh::launch_compact_lists(h->stream, h->d_list_off, h->d_list_len, h->nlist, h->d_codes, h->d_ids, h->code_size,
                                 fc->d_tab, h->w_cmp_codes.as<uint8_t>(), h->w_cmp_ids.as<int64_t>(), h->w_cmp_len.as<int>(),
                                 with_sums ? h->d_sums : nullptr, with_sums ? h->w_cmp_sums.as<float>() : nullptr);
        h->cmp_gen = fc->any_clause ? 0 : h->write_gen;   // shadow lists under a request's own clauses serve that request only
        h->cmp_sums_built = with_sums;
    }
    if (with_sums) h->d_sums = h->w_cmp_sums.as<float>();
    h->cmp_has_sums = with_sums;
    h->cmp_by_clause = fc->any_clause;
    h->d_codes = h->w_cmp_codes.as<uint8_t>();
    h->d_ids = h->w_cmp_ids.as<int64_t>();
    h->d_list_len = h->w_cmp_len.as<int>();
    h->prefiltered = true;
    lc->on = true;
    fc->any_clause = false;
    return GAMMA_HIP_OK;
}

// given != nullptr: the filter context of a combined batch (p's own filter clauses are ignored)
int ivfpq_search_device_locked(H* h, const gamma_hip_search_params* p, int nq, const float* d_x, int k,
                               float* d_distances, int64_t* d_labels, const FiltCtx* given) {
    GH_TRY(ivfpq_check(h, p, nq, k));
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    p = &pp;
    if (k <= 0 || nq == 0) {   // gamma_index_ivfpq.cc:753-756
        // (the deferred-replay contract: the previous call is complete after ANY next search call, an empty one too)
        if (h->replay_pending) {
            GH_CHECK(h, hipSetDevice(h->device));
            GH_TRY(replay_join(h));
        }
        return GAMMA_HIP_OK;
    }
    GH_CHECK(h, hipSetDevice(h->device));
    const int R = std::max(p->recall_num, k);
    FiltCtx fc;
    if (given) {
        fc = *given;
    } else {
        gh::FilterDesc filt;
        GH_TRY(build_filter(h, p, &filt, nullptr, (int64_t)nq * p->nprobe * (h->ntotal / std::max(1, h->nlist))));
        GH_TRY(filt_ctx_single(h, filt, &fc));
    }
    // faiss picks the coarse path from the size of the WHOLE call (faiss:utils/distances.cpp:346);
    // the internal chunks must not re-decide it
    if (pp.coarse_mode < 0) pp.coarse_mode = nq < 20 ? 0 : 1;
    if (pp.coarse_mode == 1 && blas_form_not_restated(nq, h->nlist, h->d)) h->blas_unrestated++;
    // OPQ (gamma_hip_opq_set): the coarse quantizer, the query tables and the scan see the rotated queries, the exact
    // re-rank and the tie replay the caller's (gamma_index_ivfpq.cc:514-566 rotates before search_preassigned, compute_dis
    // reads the raw store with the raw query).  The whole call is rotated here, once, before its first chunk: nothing
    // grows the buffer while the call's kernels are queued.
    const float* d_xq = d_x;
    if (h->d_opq) {
        GH_CHECK(h, h->w_xrot.ensure((size_t)nq * h->d * sizeof(float)));
        StageScope t(h, GAMMA_HIP_STAGE_COARSE, false);
        gh::launch_opq_apply(h->stream, h->d_opq, h->d, d_x, nq, h->w_xrot.as<float>());
        GH_CHECK(h, hipGetLastError());
        d_xq = h->w_xrot.as<float>();
    }
    if (ivfpq_small_ok(h, p, fc, nq, R)) {
        GH_TRY(replay_join(h));
        GH_TRY(ivfpq_small(h, p, fc, nq, d_xq, d_x, R, k, d_distances, d_labels));
        h->last_nq = nq;
        h->last_P = p->nprobe;
        h->last_R = R;
        return GAMMA_HIP_OK;
    }
    ListCompaction restore(h);
    GH_TRY(compact_lists_for_call(h, &fc, (int64_t)nq * p->nprobe * (h->ntotal / std::max(1, h->nlist)),
                                  !given, &restore));
    int chunk = scan_chunk(h, nq, p->nprobe);
    const int P = p->nprobe;
    // long lists (C4: 64 probes x lists of tens of thousands) make the ADC slab the limit: the coarse
    // quantizer then still runs over the whole call (one GEMM instead of one per slab chunk)
    const bool coarse_first = chunk < nq;
    struct StrideScope {   // the measured stride holds for this call only
        H* h;
        ~StrideScope() { h->q_stride_cap = 0; }
    } stride_scope{h};
    if (coarse_first) {
        GH_CHECK(h, h->w_full_cdis.ensure((size_t)nq * P * sizeof(float)));
        GH_CHECK(h, h->w_full_probe.ensure((size_t)nq * P * sizeof(int)));
        const int cc = coarse_chunk(h, nq);
        for (int q0 = 0; q0 < nq; q0 += cc)
            GH_TRY(ivfpq_coarse(h, p, std::min(cc, nq - q0), d_xq + (size_t)q0 * h->d,
                                h->w_full_cdis.as<float>() + (size_t)q0 * P, h->w_full_probe.as<int>() + (size_t)q0 * P));
        // The general slab stride is nprobe x the LONGEST list; the batch's longest candidate row is what it needs (full-size
        // C4: the longest list is ~5 x the mean, so the budget cut 8192 queries into three chunks -- and the list-major pass
        // of a third of the batch finds 11 queries per list where the whole batch has 32: half-empty tiles of 8).  The
        // assignment is on the device: measure, read one word back (the call is tens of milliseconds long), size the
        // chunks by it -- what the list shards do (gamma_hip_ivfpq_search_shard_preassigned).
        static const bool no_measure = getenv("GAMMA_HIP_NO_ROW_MEASURE") != nullptr;
        if (!no_measure && !given) {
            GH_TRY(coarse_join(h));
            GH_CHECK(h, h->w_shard_cut.ensure(std::max<size_t>((size_t)nq, 16)));
            gh::launch_max_local_total(h->stream, h->w_full_probe.as<int>(), nq, P, h->d_list_len, h->d_list_mask, h->nlist,
                                       h->w_shard_cut.as<int>());
            int mx[2] = {0, 0};
            GH_CHECK(h, hipMemcpyAsync(mx, h->w_shard_cut.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            GH_CHECK(h, hipStreamSynchronize(h->stream));
            h->q_stride_cap = (std::max<int64_t>(mx[0], 1) + 3) & ~(int64_t)3;
            const int64_t by_dist = (int64_t)(h->dist_budget_bytes / ((size_t)h->q_stride_cap * sizeof(float)));
            chunk = (int)std::max<int64_t>(chunk, std::min<int64_t>(by_dist, nq));
        }
    }
    // a call of several chunks: the tie replay of chunk i runs on its own stream beside chunk i + 1 (what
    // gamma_hip_set_deferred_replay does across calls); a caller that has not asked for that gets the join at the end
    struct DeferScope {
        H* h;
        bool saved;
        ~DeferScope() { h->defer_now = saved; }
    } defer_scope{h, h->defer_now};
    const bool defer_inside = chunk < nq && !h->defer_now && h->side2 != nullptr;
    if (defer_inside) h->defer_now = true;
    static const bool no_rerank_order = getenv("GAMMA_HIP_NO_RERANK_ORDER") != nullptr;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nc = std::min(chunk, nq - q0);
        if (coarse_first)
            GH_TRY(ivfpq_stage_a(h, p, fc.at(q0), nc, d_xq + (size_t)q0 * h->d, R,
                                 h->w_full_cdis.as<float>() + (size_t)q0 * P, h->w_full_probe.as<int>() + (size_t)q0 * P));
        else
            GH_TRY(ivfpq_stage_a(h, p, fc.at(q0), nc, d_xq + (size_t)q0 * h->d, R));
        GH_TRY(ivfpq_stage_b(h, p, nc, d_x + (size_t)q0 * h->d, R, k, h->w_cand_dis.as<float>(),
                             h->w_cand_ids.as<int64_t>(), d_distances + (size_t)q0 * k,
                             d_labels + (size_t)q0 * k, no_rerank_order ? nullptr : h->last_qperm,
                             /*tie_mode=*/1));
        h->last_nq = nc;
    }
    if (defer_inside) GH_TRY(replay_join(h));
    h->last_P = p->nprobe;
    h->last_R = R;
    return GAMMA_HIP_OK;
}

// ---- what the exact scanners (IVFFLAT, flat) share ------------------------------------
void flat_tie_args(H* h, gh::TieReplayArgs* tr, bool l2, int nq, int64_t q_stride, int P, int k, const float* d_x, float* cand_dis,
                   int64_t* cand_ids, float* d_distances, int64_t* d_labels, int fixed_n) {
    tr->list = nullptr;
    tr->count = nullptr;
    tr->nq = nq;
    tr->slab = h->w_dist.as<float>();
    tr->q_stride = q_stride;
    tr->pair_off = P > 0 ? h->w_pair_off.as<int>() : nullptr;
    tr->pair_base = P > 0 ? h->w_pair_base.as<int64_t>() : nullptr;
    tr->ids = h->d_ids;
    tr->P = P;
    tr->G = 1;
    tr->ready = nullptr;
    tr->surv = nullptr;
    tr->gcnt = nullptr;
    tr->nsl = 0;
    tr->slice_cap = 0;
    tr->x = d_x;
    tr->d = h->d;
    tr->rows = gh::RowsRef{h->raw_f32()};   // (has_rank 0: no row is read -- the fp32 kernels, whatever the store holds)
    tr->nraw = h->nraw;
    tr->R = k;
    tr->k = k;
    tr->has_rank = 0;
    tr->min_score = -INFINITY;
    tr->max_score = INFINITY;
    tr->neutral = neutral_of(l2);
    tr->cand_dis = cand_dis;
    tr->cand_ids = cand_ids;
    tr->distances = d_distances;
    tr->labels = d_labels;
    tr->pop_push = 1;
    tr->fixed_n = fixed_n;
}

int ivfpq_search_host_locked(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x,
                                   int k, float* distances, int64_t* labels) {
    SearchLock lk(h);
    GH_TRY(ivfpq_check(h, p, nq, k));
    if (nq > 0 && k > 0 && (!x || !distances || !labels)) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    return host_search(h, nq, h->d, x, k, distances, labels, [&](const float* dx, float* dd, int64_t* dl) {
        return ivfpq_search_device_locked(h, p, nq, dx, k, dd, dl);
    }, true, &lk);
}

// A LARGE host-buffer call (the plugin's Search with thousands of queries) when several client threads share the
// handle: the reference's Search is re-entrant (tests/test.h:1033-1062).  The call's queries are uploaded on a stream of
// their own into one of two staging slots BEFORE the search lock is taken (the previous caller's kernels are running);
// under the lock the search is enqueued with its tie replay on the side stream, the results follow the replay down into
// pinned memory, and the lock is released: the caller waits for ITS completion event while the next caller's coarse
// quantizer / tables / scan run beside this call's replay and copies.  One caller alone loses nothing.
int ivfpq_search_host_overlap(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x, int k,
                              float* distances, int64_t* labels) {
    const int d = h->d;
    H::HostSlot* sl = nullptr;
    {
        std::unique_lock<std::mutex> g(h->hs_mu);
        h->hs_cv.wait(g, [&] { return !h->hslot[0].busy || !h->hslot[1].busy; });
        sl = !h->hslot[0].busy ? &h->hslot[0] : &h->hslot[1];
        sl->busy = true;
    }
    struct Release {
        H* h; H::HostSlot* sl;
        ~Release() {
            { std::lock_guard<std::mutex> g(h->hs_mu); sl->busy = false; }
            h->hs_cv.notify_one();
        }
    } release{h, sl};
    GH_CHECK(h, hipSetDevice(h->device));
    const size_t bx = (size_t)nq * d * sizeof(float), bd = (size_t)nq * k * sizeof(float), bi = (size_t)nq * k * sizeof(int64_t);
    // (the queries through pinned memory too -- a CPU copy, then a true asynchronous upload -- measured slower: 10.66 against
    //  10.90 M q/s with two callers, 7.5 against 8.2 with one)
    const size_t off_i = 0, off_d = (bi + 63) & ~(size_t)63, need = off_d + bd;
    GH_CHECK(h, sl->x.ensure(bx));
    GH_CHECK(h, sl->D.ensure(bd));
    GH_CHECK(h, sl->I.ensure(bi));
    if (need > sl->pin_bytes) {
        if (sl->pin) (void)hipHostFree(sl->pin);
        sl->pin = nullptr;
        sl->pin_bytes = 0;
        GH_CHECK(h, hipHostMalloc(&sl->pin, need + need / 4, hipHostMallocDefault));
        sl->pin_bytes = need + need / 4;
    }
    if (!sl->ev_up) GH_CHECK(h, hipEventCreateWithFlags(&sl->ev_up, hipEventDisableTiming));
    if (!sl->ev_done) GH_CHECK(h, hipEventCreateWithFlags(&sl->ev_done, hipEventDisableTiming));
    {
        std::lock_guard<std::mutex> g(h->hs_mu);
        if (!h->up_stream) GH_CHECK(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
    }
    // (pageable source: the runtime stages it; the thread is held here while the copy engine works -- beside whatever
    //  the search stream is running for the previous caller)
    char* pin = static_cast<char*>(sl->pin);
    GH_CHECK(h, hipMemcpyAsync(sl->x.p, x, bx, hipMemcpyHostToDevice, h->up_stream));
    GH_CHECK(h, hipEventRecord(sl->ev_up, h->up_stream));
    {
        SearchLock lk(h);
        GH_TRY(ivfpq_check(h, p, nq, k));
        GH_CHECK(h, hipStreamWaitEvent(h->stream, sl->ev_up, 0));
        h->defer_now = h->side2 != nullptr;
        const int rc = ivfpq_search_device_locked(h, p, nq, sl->x.as<float>(), k, sl->D.as<float>(), sl->I.as<int64_t>());
        h->defer_now = false;
        if (rc != GAMMA_HIP_OK) return rc;
        hipStream_t ts = h->replay_pending ? h->side2 : h->stream;   // behind this call's replay, if it has one
        GH_CHECK(h, hipMemcpyAsync(pin + off_d, sl->D.p, bd, hipMemcpyDeviceToHost, ts));
        GH_CHECK(h, hipMemcpyAsync(pin + off_i, sl->I.p, bi, hipMemcpyDeviceToHost, ts));
        GH_CHECK(h, hipEventRecord(sl->ev_done, ts));
    }
    if (hipEventSynchronize(sl->ev_done) != hipSuccess) return fail(h, GAMMA_HIP_EDEVICE, "waiting for the call's completion event");
    std::memcpy(distances, pin + off_d, bd);
    std::memcpy(labels, pin + off_i, bi);
    return GAMMA_HIP_OK;
}

}  // namespace ghi

using namespace ghi;

extern "C" {

/* ---- search ----------------------------------------------------------------------------- */
int gamma_hip_ivfpq_search_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                  const float* d_x, int k, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    h->defer_now = h->defer_replay;
    const int rc = ivfpq_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
    h->defer_now = false;
    return rc;
}

int gamma_hip_ivfpq_search_device_wait(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                       const float* d_x, int k, float* d_distances, int64_t* d_labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    CallTicket t(h->call_slots);   // this call's completion event: its own until the wait below is over (call_slots.h)
    {
        SearchLock lk(h);
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, t.take());
        h->defer_now = h->side2 != nullptr;   // the replay of this call's flagged queries: side stream, beside the next caller's head
        const int rc = ivfpq_search_device_locked(h, p, nq, d_x, k, d_distances, d_labels);
        h->defer_now = false;
        if (rc != GAMMA_HIP_OK) return rc;
        // everything of the call precedes the replay's fork; the replay (if one is pending: this call's) ends the call
        GH_CHECK(h, CallSlots::arm(t.slot(), h->replay_pending ? h->side2 : h->stream));
    }
    // the handle is free from here on: the next caller enqueues while this one waits for its own call
    const hipError_t e = CallSlots::wait(t.slot());
    return e == hipSuccess ? GAMMA_HIP_OK : GAMMA_HIP_EDEVICE;
}

int gamma_hip_ivfpq_search(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* x,
                           int k, float* distances, int64_t* labels) {
    if (!h) return GAMMA_HIP_EINVAL;
    if (h->combine && p && nq > 0 && nq <= COMB_MAX_NQ && k > 0 && x && distances && labels && h->ivf_init && h->d > 0 &&
        (!p->has_range || (p->n_range >= 0 && p->n_range <= gh::kMaxRange && (p->n_range == 0 || p->range))) &&
        p->n_field >= 0 && p->n_field <= gh::kMaxField && (p->n_field == 0 || p->field) &&
        p->n_term >= 0 && p->n_term <= gh::kMaxTerm && (p->n_term == 0 || p->term))
        return combined_search(h, p, nq, x, k, distances, labels);
    // large calls: staged so that concurrent callers overlap (ivfpq_search_host_overlap); GAMMA_HIP_NO_HOST_OVERLAP=1: the plain path
    static const bool no_overlap = getenv("GAMMA_HIP_NO_HOST_OVERLAP") != nullptr;
    // (a caller that finds the handle idle takes the plain path: results straight into its buffers, 1.89 against 1.96 ms per
    //  16384-query call; one that finds another large call in flight takes the staged path -- two alternating callers are
    //  both on it from their second call on)
    struct InFlight {
        std::atomic<int>& n;
        int before;
        explicit InFlight(std::atomic<int>& c) : n(c), before(c.fetch_add(1)) {}
        ~InFlight() { n.fetch_sub(1); }
    };
    const bool big = p && nq > 0 && k > 0 && x && distances && labels && h->ivf_init && !h->ivfflat && h->d > 0 &&
                     (size_t)nq * h->d * sizeof(float) > ((size_t)1 << 20);
    if (!big) return ivfpq_search_host_locked(h, p, nq, x, k, distances, labels);
    InFlight fl(h->big_calls_in_flight);
    // (sticky for 50 ms: alternating callers are now and then both between two calls)
    const int64_t now_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (fl.before > 0) h->big_calls_overlap_seen_ns.store(now_ns, std::memory_order_relaxed);
    const bool recent = now_ns - h->big_calls_overlap_seen_ns.load(std::memory_order_relaxed) < 50000000LL;
    if (!no_overlap && h->side2 && (fl.before > 0 || recent)) return ivfpq_search_host_overlap(h, p, nq, x, k, distances, labels);
    return ivfpq_search_host_locked(h, p, nq, x, k, distances, labels);
}

int gamma_hip_ivfpq_last_stages(gamma_hip_index* h, float* coarse_dis, int64_t* coarse_idx,
                                float* recall_dis, int64_t* recall_ids) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_TRY(replay_join(h));
    const int nq = h->last_nq, P = h->last_P, R = h->last_R;
    if (nq <= 0) return fail(h, GAMMA_HIP_EINVAL, "no previous search");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    if (coarse_dis) GH_CHECK(h, hipMemcpy(coarse_dis, h->w_coarse_dis.p, (size_t)nq * P * sizeof(float), hipMemcpyDeviceToHost));
    if (coarse_idx) {
        std::vector<int> tmp((size_t)nq * P);
        GH_CHECK(h, hipMemcpy(tmp.data(), h->w_probe.p, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); i++) coarse_idx[i] = tmp[i];
    }
    if (recall_dis) GH_CHECK(h, hipMemcpy(recall_dis, h->w_cand_dis.p, (size_t)nq * R * sizeof(float), hipMemcpyDeviceToHost));
    if (recall_ids) GH_CHECK(h, hipMemcpy(recall_ids, h->w_cand_ids.p, (size_t)nq * R * sizeof(int64_t), hipMemcpyDeviceToHost));
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_coarse_device(gamma_hip_index* h, const gamma_hip_search_params* p, int nq,
                                  const float* d_x, float* d_coarse_dis, int32_t* d_probe) {
    if (!h) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (h->d_opq) return opq_refuse(h, "gamma_hip_ivfpq_coarse_device");
    GH_TRY(replay_join(h));
    GH_TRY(ivfpq_check(h, p, nq, 1));
    if (nq == 0) return GAMMA_HIP_OK;
    if (!d_x || !d_coarse_dis || !d_probe) return fail(h, GAMMA_HIP_EINVAL, "null buffer");
    GH_CHECK(h, hipSetDevice(h->device));
    const int P = p->nprobe;
    gamma_hip_search_params pp;
    GH_TRY(resolve_ties(h, p, &pp, p->nprobe <= gh::tie_replay_max_probes(), "exact_ties = 1 with nprobe > 1024"));
    // the caller resolves coarse_mode -1 on the size of the whole batch; a slice that arrives unresolved decides by itself
    if (pp.coarse_mode < 0) pp.coarse_mode = nq < 20 ? 0 : 1;
    if (pp.coarse_mode == 1 && blas_form_not_restated(nq, h->nlist, h->d)) h->blas_unrestated++;
    p = &pp;
    const int chunk = coarse_chunk(h, nq);
    for (int q0 = 0; q0 < nq; q0 += chunk)
        GH_TRY(ivfpq_coarse(h, p, std::min(chunk, nq - q0), d_x + (size_t)q0 * h->d, d_coarse_dis + (size_t)q0 * P,
                            d_probe + (size_t)q0 * P));
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

int gamma_hip_ivfpq_max_list_len(gamma_hip_index* h) { return (h && h->ivf_init) ? h->max_list_len : 0; }

int gamma_hip_debug_heap_stream(gamma_hip_index* h, int op, int k, int n, const float* vals, float* arr_vals, int32_t* arr_ids,
                                float* sorted_vals, int32_t* sorted_ids) {
    if (!h || op < 0 || op > 4 || (op == 4 && n < 1) || k < 1 || k > gh::tie_small_max_k() || n < 0 || (n > 0 && !vals) || !arr_vals || !arr_ids ||
        !sorted_vals || !sorted_ids)
        return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, h->w_stage.ensure((size_t)std::max(n, 1) * sizeof(float) + (size_t)2 * k * sizeof(uint2) + 16));
    float* d_vals = h->w_stage.as<float>();
    uint2* d_arr = reinterpret_cast<uint2*>(h->w_stage.as<char>() + (((size_t)std::max(n, 1) * sizeof(float) + 15) & ~(size_t)15));
    uint2* d_sorted = d_arr + k;
    if (n > 0) GH_CHECK(h, hipMemcpyAsync(d_vals, vals, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    gh::launch_debug_heap_stream(h->stream, op, k, n, d_vals, d_arr, d_sorted);
    std::vector<uint2> out((size_t)2 * k);
    GH_CHECK(h, hipMemcpyAsync(out.data(), d_arr, (size_t)2 * k * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    GH_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < k; i++) {
        memcpy(&arr_vals[i], &out[i].x, 4);
        arr_ids[i] = (int32_t)out[i].y;
        memcpy(&sorted_vals[i], &out[k + i].x, 4);
        sorted_ids[i] = (int32_t)out[k + i].y;
    }
    return GAMMA_HIP_OK;
}

}  // extern "C"
