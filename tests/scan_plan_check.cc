// scan_plan_check.cc -- TEST INFRASTRUCTURE (tests/test_scan_plan.py builds it with g++ -fsanitize=address,undefined and runs it):
// the scan stage's plan and its bound feedback (gamma_amd/csrc/scan_plan.h / .cpp, linked alone -- no HIP, no GPU) on shapes whose
// plans follow from the rules by hand.  Exit status 0: every expectation held; otherwise each miss is printed.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gamma_amd/csrc/scan_plan.h"

static int g_failed = 0;
#define EXPECT_EQ(what, got, want)                                                                                   \
    do {                                                                                                             \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                               \
        if (g_ != w_) {                                                                                              \
            printf("FAIL %s line %d: %s = %lld, expected %lld\n", what, __LINE__, #got, g_, w_);                     \
            g_failed++;                                                                                              \
        }                                                                                                            \
    } while (0)

using gh::BoundFeedbackState;
using gh::ScanPlan;
using gh::ScanShape;
using gh::ScanSwitches;

// sums and t2max present, table mode 1, L2, no filter, not a shard, lists short enough for the list-major pass's positions
static ScanShape shape(int nlist, int M, int64_t ntotal, int P, int R, int nq) {
    ScanShape sh;
    sh.nq = nq;
    sh.P = P;
    sh.R = R;
    sh.M = M;
    sh.nlist = nlist;
    sh.max_list_len = (int)(2 * ntotal / nlist);
    sh.have_sums = true;
    sh.sort_queries = true;
    sh.lists = gh::scan_list_stats(ntotal, nlist, nullptr, nullptr, false);
    return sh;
}

// the whole plan with the feedback answering "bounded" whenever the call is eligible
static ScanPlan plan(const ScanShape& sh, const ScanSwitches& sw = ScanSwitches()) {
    ScanPlan pl = gh::scan_plan_groups(sh, sw);
    gh::scan_plan_passes(pl, sh, sw, pl.bound_eligible);
    return pl;
}

static void check_plans() {
    {   // C3
        const ScanPlan pl = plan(shape(4096, 16, 1000000, 32, 200, 16384));
        EXPECT_EQ("C3", pl.G, 5);
        EXPECT_EQ("C3", pl.PGN, 7);
        EXPECT_EQ("C3", pl.bounded, 1);
        EXPECT_EQ("C3", pl.cf_ok, 1);
        EXPECT_EQ("C3", pl.q8_ok, 0);
        EXPECT_EQ("C3", pl.c8, 1);
        EXPECT_EQ("C3", pl.cf_span, 0);
        EXPECT_EQ("C3", pl.PGM, 2);
        EXPECT_EQ("C3", pl.nsl, 2);
        EXPECT_EQ("C3", pl.cap, 1024);
        EXPECT_EQ("C3", pl.fuse_ip, 0);
        EXPECT_EQ("C3", pl.res, 0);
        EXPECT_EQ("C3", pl.need_ids, 0);
        EXPECT_EQ("C3", pl.order, 1);   // 4096 x 16 x 256 floats of T2 = 64 MB > 8 MB
        EXPECT_EQ("C3", pl.q_stride, 32 * 488);
        // rq (count + 16384 ints, 8-byte aligned) | ready | gcnt [nq][2] | fl (count + list)
        EXPECT_EQ("C3", pl.ready_off, 65544);
        EXPECT_EQ("C3", pl.gcnt_off, 65544 + 16384 * 8);
        EXPECT_EQ("C3", pl.fl_off, 65544 + 16384 * 8 + 16384 * 2 * 4);
        EXPECT_EQ("C3", pl.scnt_bytes, 65544 + 16384 * 8 + 16384 * 2 * 4 + 16385 * 4);
    }
    // the 5 -> 4 -> 2 stepping of small batches
    EXPECT_EQ("C3 nq 586", plan(shape(4096, 16, 1000000, 32, 200, 586)).G, 5);
    for (int nq : {585, 512}) {
        const ScanPlan pl = plan(shape(4096, 16, 1000000, 32, 200, nq));
        EXPECT_EQ("C3 nq 585 / 512", pl.G, 4);
        EXPECT_EQ("C3 nq 585 / 512", pl.bounded, 1);
    }
    {
        const ScanPlan pl = plan(shape(4096, 16, 1000000, 32, 200, 511));
        EXPECT_EQ("C3 nq 511", pl.G, 2);
        EXPECT_EQ("C3 nq 511", pl.bound_eligible, 0);
        EXPECT_EQ("C3 nq 511", pl.bounded, 0);
        EXPECT_EQ("C3 nq 511", pl.PGM, 16);
    }
    {   // (not in the issue's table) eight probes: the byte-image rule leaves the group of 8 alone -- one group per query, fused tables
        const ScanPlan pl = plan(shape(4096, 16, 1000000, 8, 200, 16384));
        EXPECT_EQ("C3 nprobe 8", pl.G, 8);
        EXPECT_EQ("C3 nprobe 8", pl.PGN, 1);
        EXPECT_EQ("C3 nprobe 8", pl.bounded, 1);
        EXPECT_EQ("C3 nprobe 8", pl.fuse_ip, 1);
        EXPECT_EQ("C3 nprobe 8", pl.cf_ok, 0);
        ScanSwitches sw;
        sw.no_fused_ip = true;
        EXPECT_EQ("C3 nprobe 8, GAMMA_HIP_NO_FUSED_IP", plan(shape(4096, 16, 1000000, 8, 200, 16384), sw).fuse_ip, 0);
    }
    {   // the switch between the query-major and the list-major pass
        const ScanPlan pl = plan(shape(4096, 16, (int64_t)976 * 4096, 32, 100, 8192));
        EXPECT_EQ("976 per list", pl.G, 4);
        EXPECT_EQ("976 per list", pl.PGN, 8);
        EXPECT_EQ("976 per list", pl.q8_ok, 1);
        EXPECT_EQ("976 per list", pl.cf_ok, 0);
        EXPECT_EQ("976 per list", pl.c8, 0);
        EXPECT_EQ("976 per list", pl.PGM, 1);
        EXPECT_EQ("976 per list", pl.nsl, 8);
        const ScanPlan ps = plan(shape(4096, 16, (int64_t)732 * 4096, 32, 100, 8192));
        EXPECT_EQ("732 per list", ps.cf_ok, 1);
        EXPECT_EQ("732 per list", ps.q8_ok, 0);
        ScanSwitches sw;
        sw.no_q8 = true;
        const ScanPlan pn = plan(shape(4096, 16, (int64_t)976 * 4096, 32, 100, 8192), sw);
        EXPECT_EQ("976 per list, GAMMA_HIP_NO_Q8", pn.q8_ok, 0);
        EXPECT_EQ("976 per list, GAMMA_HIP_NO_Q8", pn.cf_ok, 1);
    }
    {   // C4 shape at 8 M
        const ScanPlan pl = plan(shape(16384, 32, (int64_t)488 * 16384, 64, 100, 8192));
        EXPECT_EQ("C4 8 M", pl.G, 8);
        EXPECT_EQ("C4 8 M", pl.PGN, 8);
        EXPECT_EQ("C4 8 M", pl.cf_ok, 1);
        EXPECT_EQ("C4 8 M", pl.c8, 0);
        EXPECT_EQ("C4 8 M", pl.PGM, 2);
        EXPECT_EQ("C4 8 M", pl.nsl, 2);
        const ScanPlan pf = plan(shape(16384, 32, (int64_t)6100 * 16384, 64, 100, 8192));
        EXPECT_EQ("C4 full size", pf.G, 4);
        EXPECT_EQ("C4 full size", pf.PGN, 16);
        EXPECT_EQ("C4 full size", pf.cf_ok, 0);
        EXPECT_EQ("C4 full size", pf.q8_ok, 1);
        EXPECT_EQ("C4 full size", pf.PGM, 1);
        EXPECT_EQ("C4 full size", pf.nsl, 16);
    }
    {   // the limits of the bounded scan
        EXPECT_EQ("R 1024", plan(shape(4096, 16, 1000000, 32, 1024, 16384)).bounded, 1);
        EXPECT_EQ("R 1024", plan(shape(4096, 16, 1000000, 32, 1024, 16384)).cap, 2048);
        EXPECT_EQ("R 1025", plan(shape(4096, 16, 1000000, 32, 1025, 16384)).bounded, 0);
        EXPECT_EQ("P 128", plan(shape(4096, 16, 1000000, 128, 200, 16384)).bounded, 1);
        EXPECT_EQ("P 129", plan(shape(4096, 16, 1000000, 129, 200, 16384)).bounded, 0);
        ScanShape off = shape(4096, 16, 1000000, 32, 200, 16384);
        off.scan_bound = false;
        EXPECT_EQ("GAMMA_HIP_NO_SCAN_BOUND", plan(off).bounded, 0);
    }
    {   // 4-bit codes: one path
        ScanShape sh = shape(4096, 16, 1000000, 32, 200, 16384);
        sh.pq4 = true;
        const ScanPlan pl = plan(sh);
        EXPECT_EQ("4-bit", pl.bounded, 0);
        EXPECT_EQ("4-bit", pl.cf_ok, 0);
        EXPECT_EQ("4-bit", pl.q8_ok, 0);
        EXPECT_EQ("4-bit", pl.fuse_ip, 0);
        EXPECT_EQ("4-bit", pl.res, 0);
        sh.P = 8;
        EXPECT_EQ("4-bit nprobe 8", plan(sh).fuse_ip, 0);
    }
    {   // table mode 0: residual tables, nothing built on the sums
        ScanShape sh = shape(4096, 16, 1000000, 8, 200, 16384);
        sh.table_mode = 0;
        const ScanPlan p8 = plan(sh);
        EXPECT_EQ("table mode 0", p8.res, 1);
        EXPECT_EQ("table mode 0", p8.fuse_ip, 0);
        EXPECT_EQ("table mode 0", p8.bounded, 1);
        for (int64_t per_list : {244, 976}) {
            ScanShape s2 = shape(4096, 16, per_list * 4096, 32, 200, 16384);
            s2.table_mode = 0;
            s2.have_sums = false;
            const ScanPlan pl = plan(s2);
            EXPECT_EQ("table mode 0, no sums", pl.res, 1);
            EXPECT_EQ("table mode 0, no sums", pl.bounded, 1);
            EXPECT_EQ("table mode 0, no sums", pl.cf_ok, 0);
            EXPECT_EQ("table mode 0, no sums", pl.q8_ok, 0);
            EXPECT_EQ("table mode 0, no sums", pl.c8, 0);
            EXPECT_EQ("table mode 0, no sums", pl.PGM, pl.PGN);
            EXPECT_EQ("table mode 0, no sums", pl.nsl, pl.PGN);
        }
        ScanShape ip = shape(4096, 16, 1000000, 32, 200, 16384);
        ip.l2 = false;
        ip.table_mode = 0;
        EXPECT_EQ("inner product", plan(ip).res, 0);
        EXPECT_EQ("inner product", plan(ip).cf_ok, 0);
    }
    {   // two-phase list shard: the producers' group is G1, and it bounds although G < 4
        ScanShape sh = shape(4096, 16, 1000000, 32, 200, 16384);
        sh.shard = sh.compacted = sh.two_phase = true;
        sh.G1 = 2;
        const ScanPlan pl = plan(sh);
        EXPECT_EQ("two-phase", pl.G, 2);
        EXPECT_EQ("two-phase", pl.PGN, 16);
        EXPECT_EQ("two-phase", pl.bounded, 1);
        sh.two_phase = false;   // a shard without a supplied assignment has nothing to bound from
        sh.compacted = false;
        EXPECT_EQ("sparse shard", plan(sh).bounded, 0);
    }
    {   // the query order: from 256 queries on, when the T2 rows are more than 8 MiB.  The first shape is the one the ordered legs of
        // tests/test_gpu_rerank_filter_shapes.py run (1024 lists x 16 x 1 KiB = 16 MiB, 300 queries, 32 probes)
        for (int R : {200, 600}) {
            EXPECT_EQ("ordered leg", plan(shape(1024, 16, 40000, 32, R, 300)).order, 1);
            EXPECT_EQ("ordered leg, 1027 queries", plan(shape(1024, 16, 40000, 32, R, 1027)).order, 1);
            EXPECT_EQ("ordered leg, a chunk of 400", plan(shape(1024, 16, 40000, 32, R, 400)).order, 1);
            EXPECT_EQ("ordered leg, 256 queries", plan(shape(1024, 16, 40000, 32, R, 256)).order, 1);
            EXPECT_EQ("ordered leg, 255 queries", plan(shape(1024, 16, 40000, 32, R, 255)).order, 0);
            EXPECT_EQ("ordered leg, 512 lists", plan(shape(512, 16, 40000, 32, R, 300)).order, 0);   // 8 MiB: not more
        }
    }
    {   // what can reject an entry
        ScanShape sh = shape(4096, 16, 1000000, 32, 200, 16384);
        sh.rejects = true;
        EXPECT_EQ("deletes", plan(sh).need_ids, 1);
        sh.prefiltered = true;
        EXPECT_EQ("deletes, compacted lists", plan(sh).need_ids, 0);
        EXPECT_EQ("compacted lists without sums", plan(sh).cf_ok, 0);
    }
}

static void check_list_stats() {
    // 8 lists over W = 2 shards; this shard's: 0, 2, 4 (empty), 6
    const std::vector<int> len = {10, 50, 30, 50, 0, 50, 20, 50};
    const std::vector<uint8_t> mask = {1, 0, 1, 0, 1, 0, 1, 0};
    const gh::ListStats whole = gh::scan_list_stats(260, 8, len.data(), mask.data(), false);
    EXPECT_EQ("whole index", whole.owned, 8);
    EXPECT_EQ("whole index", whole.live, 8);
    EXPECT_EQ("whole index", (int)(whole.mean_len * 100), 3250);
    const gh::ListStats masked = gh::scan_list_stats(260, 8, len.data(), mask.data(), true);
    EXPECT_EQ("masked shard", masked.owned, 3);
    EXPECT_EQ("masked shard", masked.live, 3);
    EXPECT_EQ("masked shard", (int)(masked.mean_len * 100), 2000);
    // a shard that holds its lists only (the others are empty here): as the parent commit has it, the mean stays the whole
    // index's and `owned` nlist; only `live` counts the lists
    const std::vector<int> own = {10, 0, 30, 0, 0, 0, 20, 0};
    const gh::ListStats unmasked = gh::scan_list_stats(60, 8, own.data(), nullptr, true);
    EXPECT_EQ("unmasked shard", unmasked.owned, 8);
    EXPECT_EQ("unmasked shard", unmasked.live, 3);
    EXPECT_EQ("unmasked shard", (int)(unmasked.mean_len * 100), 750);
    // a compacted shard with few expected candidates per query: one workgroup takes all of a query's probes
    ScanShape sh = shape(4096, 16, 1000000, 32, 200, 16384);
    sh.shard = sh.compacted = true;
    sh.lists.live = 512;   // W = 8: 32 x 512 / 4096 = 4 probes of ~244 codes
    const ScanPlan pl = plan(sh);
    EXPECT_EQ("compacted shard", pl.G, 32);
    EXPECT_EQ("compacted shard", pl.PGN, 1);
    EXPECT_EQ("compacted shard", pl.fuse_ip, 1);
    EXPECT_EQ("compacted shard", pl.order, 0);   // 512 x 16 x 256 floats = 8 MB: not more
}

static void check_switches() {
    for (const char* n : {"GAMMA_HIP_NO_C8", "GAMMA_HIP_NO_FUSED_IP", "GAMMA_HIP_NO_SCAN_CF", "GAMMA_HIP_SCAN_CF_CODES", "GAMMA_HIP_NO_Q8",
                          "GAMMA_HIP_Q8_MINLEN", "GAMMA_HIP_NO_Q8_DEMAND", "GAMMA_HIP_NO_BOUND_FEEDBACK", "GAMMA_HIP_SCAN_G"})
        unsetenv(n);
    const ScanSwitches d = ScanSwitches::from_env();
    EXPECT_EQ("defaults", d.no_c8 || d.no_fused_ip || d.no_scan_cf || d.no_q8 || d.no_q8_demand || d.no_bound_feedback, 0);
    EXPECT_EQ("defaults", (int)d.cf_codes, 65536);
    EXPECT_EQ("defaults", (int)d.q8_minlen, 800);
    setenv("GAMMA_HIP_NO_C8", "1", 1);
    setenv("GAMMA_HIP_Q8_MINLEN", "700", 1);
    setenv("GAMMA_HIP_SCAN_CF_CODES", "4096", 1);
    const ScanSwitches s = ScanSwitches::from_env();
    EXPECT_EQ("set", s.no_c8, 1);
    EXPECT_EQ("set", (int)s.q8_minlen, 700);
    // without the byte image the first group keeps its 8 probes; consumer groups of at most 4096 codes: 24 probes x 244 in two
    const ScanPlan pl = plan(shape(4096, 16, 1000000, 32, 200, 16384), s);
    EXPECT_EQ("GAMMA_HIP_NO_C8", pl.G, 8);
    EXPECT_EQ("GAMMA_HIP_NO_C8", pl.c8, 0);
    EXPECT_EQ("GAMMA_HIP_SCAN_CF_CODES", pl.cf_span, 12);
    EXPECT_EQ("GAMMA_HIP_SCAN_CF_CODES", pl.PGM, 3);
    EXPECT_EQ("GAMMA_HIP_Q8_MINLEN", plan(shape(4096, 16, (int64_t)732 * 4096, 32, 100, 8192), s).q8_ok, 1);
    ScanSwitches nocf;
    nocf.no_scan_cf = true;
    EXPECT_EQ("GAMMA_HIP_NO_SCAN_CF", plan(shape(4096, 16, 1000000, 32, 200, 16384), nocf).cf_ok, 0);
    EXPECT_EQ("GAMMA_HIP_NO_SCAN_CF", plan(shape(4096, 16, (int64_t)976 * 4096, 32, 100, 8192), nocf).q8_ok, 0);
    // GAMMA_HIP_SCAN_G is read per call
    setenv("GAMMA_HIP_SCAN_G", "6", 1);
    EXPECT_EQ("GAMMA_HIP_SCAN_G", plan(shape(4096, 16, 1000000, 32, 200, 16384)).G, 6);
    unsetenv("GAMMA_HIP_SCAN_G");
    EXPECT_EQ("GAMMA_HIP_SCAN_G", plan(shape(4096, 16, 1000000, 32, 200, 16384)).G, 5);
}

static void check_feedback() {
    const uint64_t sig = BoundFeedbackState::signature(32, 200, true, false, false);
    {
        BoundFeedbackState fb;
        EXPECT_EQ("fresh kind", fb.new_kind(sig), 1);
        EXPECT_EQ("fresh kind", fb.new_kind(sig), 0);
        BoundFeedbackState::Sample s = {2047, 2047};   // too few queries: decides nothing
        EXPECT_EQ("2047 queries", fb.step(true, &s), 1);
        EXPECT_EQ("2047 queries", fb.seen[1], 0);
        EXPECT_EQ("2047 queries", fb.backoffs, 0);
        s = {1024, 2048};   // half fell through: not MORE than half
        EXPECT_EQ("1024 of 2048", fb.step(true, &s), 1);
        EXPECT_EQ("1024 of 2048", fb.seen[0], 1024);
        EXPECT_EQ("1024 of 2048", fb.seen[1], 2048);
        EXPECT_EQ("1024 of 2048", fb.backoffs, 0);
        s = {1000, 2000};   // runs backwards: ignored
        EXPECT_EQ("backwards", fb.step(true, &s), 1);
        EXPECT_EQ("backwards", fb.seen[1], 2048);
        s = {900, 8192};   // fewer fallen through than seen: ignored as well
        EXPECT_EQ("backwards", fb.step(true, &s), 1);
        EXPECT_EQ("backwards", fb.seen[1], 2048);
        EXPECT_EQ("no sample", fb.step(true, nullptr), 1);
    }
    {
        BoundFeedbackState fb;
        fb.new_kind(sig);
        BoundFeedbackState::Sample s = {1025, 2048};
        EXPECT_EQ("1025 of 2048", fb.step(true, &s), 0);
        EXPECT_EQ("1025 of 2048", fb.backoffs, 1);
        EXPECT_EQ("1025 of 2048", fb.consults(), 0);
        s = {1025, 4096};   // (not looked at while the handle is backed off)
        for (int i = 1; i <= 255; i++) EXPECT_EQ("backed off", fb.step(true, &s), 0);
        EXPECT_EQ("re-probe", fb.step(true, nullptr), 1);   // the 256th call after the back-off
        EXPECT_EQ("re-probe", fb.backoffs, 1);
        EXPECT_EQ("re-probe", fb.seen[1], 2048);
        s = {1025 + 5000, 2048 + 4096};   // du is capped by dn: 4096 of 4096
        EXPECT_EQ("du capped", fb.step(true, &s), 0);
        EXPECT_EQ("du capped", fb.backoffs, 2);
        // feedback off: every eligible call is bounded, at once
        fb.set_on(false);
        for (int i = 0; i < 3; i++) EXPECT_EQ("feedback off", fb.step(true, &s), 1);
        fb.set_on(true);
        s = {20000, 20000};
        EXPECT_EQ("environment switch", fb.step(false, &s), 1);
        EXPECT_EQ("environment switch", fb.backoffs, 2);
    }
    {
        BoundFeedbackState fb;
        fb.new_kind(sig);
        const int slot0 = fb.slot();
        BoundFeedbackState::Sample s = {4096, 4096};
        EXPECT_EQ("kind 1", fb.step(true, &s), 0);
        fb.calls = 7;
        EXPECT_EQ("other kind", fb.new_kind(BoundFeedbackState::signature(32, 100, true, false, false)), 1);
        EXPECT_EQ("other kind", fb.slot(), slot0 ^ 1);
        EXPECT_EQ("other kind", fb.off_calls, 0);
        EXPECT_EQ("other kind", fb.calls, 0);
        EXPECT_EQ("other kind", fb.seen[0] + fb.seen[1], 0);
        EXPECT_EQ("other kind", fb.backoffs, 1);   // (a total of the handle)
        EXPECT_EQ("other kind", fb.step(true, nullptr), 1);
        // the copy back: the first four calls of a kind, then every 16th
        int due = 0;
        for (fb.calls = 0; fb.calls < 64; fb.calls++) due += fb.copy_due();
        EXPECT_EQ("copies in 64 calls", due, 4 + 3);
        // every part of the signature tells kinds apart
        EXPECT_EQ("signature", sig != BoundFeedbackState::signature(33, 200, true, false, false), 1);
        EXPECT_EQ("signature", sig != BoundFeedbackState::signature(32, 200, false, false, false), 1);
        EXPECT_EQ("signature", sig != BoundFeedbackState::signature(32, 200, true, true, false), 1);
        EXPECT_EQ("signature", sig != BoundFeedbackState::signature(32, 200, true, false, true), 1);
    }
}

int main() {
    check_switches();   // (first: it leaves the environment clean)
    check_plans();
    check_list_stats();
    check_feedback();
    if (g_failed) {
        printf("%d expectations failed\n", g_failed);
        return 1;
    }
    printf("scan plan ok\n");
    return 0;
}
