// ivfflat_plan_check.cc -- TEST INFRASTRUCTURE (tests/test_ivfflat_plan.py builds it with g++ -fsanitize=address,undefined and runs
// it): which scan the IVFFLAT scan stage runs over a chunk (gamma_amd/csrc/ivfflat_plan.h / .cpp, linked alone -- no HIP, no GPU).
// Every expectation below is written out from the table in ivfflat_plan.cpp, none is computed from the functions under test.
// Exit status 0: every expectation held; otherwise each miss is printed.
#include <stdio.h>
#include <stdlib.h>

#include "../gamma_amd/csrc/ivfflat_plan.h"

static int g_failed = 0;
#define EXPECT_EQ(what, got, want)                                                                                   \
    do {                                                                                                             \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                               \
        if (g_ != w_) {                                                                                              \
            printf("FAIL %s line %d: %s = %lld, expected %lld\n", what, __LINE__, #got, g_, w_);                     \
            g_failed++;                                                                                              \
        }                                                                                                            \
    } while (0)

using gh::IvfflatScanPlan;
using gh::IvfflatScanShape;
using gh::IvfflatSwitches;

enum { FILL = IvfflatScanPlan::FILL, PAIR = IvfflatScanPlan::PAIR, FIXED = IvfflatScanPlan::LM_FIXED,
       SLICED = IvfflatScanPlan::LM_SLICED, TAIL = IvfflatScanPlan::LM_TAIL };

// nlist 8, nprobe 4 throughout: 4 queries are 16 pairs = 2 nlist (lists are shared), 3 queries are 12 (they are not)
static const int NLIST = 8, P = 4;
// the scratch of a list-major launch over nc = 4: (16 pairs + 4 * 8 + 1) ints = 196 bytes; a shard rounds it to 208 and puts the
// masked length table (8 ints) behind it: 240
static const size_t LM_BYTES = 196, SHARD_MLEN_OFF = 208, SHARD_BYTES = 240;

struct Dim {
    int d;
    int lm;     // the list-major form of the length: FIXED, SLICED, or PAIR for none
    bool tail;  // 1 <= d <= 4096, d % 16 != 0: the tail kernel's lengths
};
static const Dim DIMS[] = {{16, FIXED, false}, {48, SLICED, false},   {128, FIXED, false}, {4096, SLICED, false},
                           {4112, PAIR, false}, {20, PAIR, true},      {1, PAIR, true},     {100, PAIR, true}};

static IvfflatScanShape shape(int nc, int d, int et, bool shard, bool masked, bool sparse, bool sparse_empty, bool lm_tails) {
    IvfflatScanShape sh;
    sh.nc = nc;
    sh.P = P;
    sh.nlist = NLIST;
    sh.d = d;
    sh.et = et;
    sh.shard = shard;
    sh.masked = masked;
    sh.sparse = sparse;
    sh.sparse_empty = sparse_empty;
    sh.lm_tails = lm_tails;
    return sh;
}

static void expect_plan(const char* what, const IvfflatScanPlan& pl, int kind, bool masked_len, size_t scratch, size_t mlen_off) {
    EXPECT_EQ(what, pl.kind, kind);
    EXPECT_EQ(what, pl.masked_len, masked_len);
    EXPECT_EQ(what, pl.scratch_bytes, scratch);
    EXPECT_EQ(what, pl.mlen_off, mlen_off);
}

static void check_single_handle() {
    IvfflatSwitches on, off;
    off.no_lm = true;
    for (const Dim& D : DIMS)
        for (int et = 0; et <= 4; et++)
            for (int tails = 0; tails <= 1; tails++) {
                // shared lists, no mask: the tail kernel where the switch is on, the length has a tail and the rows are numbers;
                // else the length's list-major form for every element type, sq8 included; else the pair kernel
                int want = D.lm;
                if (tails && D.tail && et <= 3) want = TAIL;
                const size_t bytes = want == PAIR ? 0 : LM_BYTES;
                expect_plan("single", gh::ivfflat_scan_plan(shape(4, D.d, et, false, false, false, false, tails), on), want, false,
                            bytes, 0);
                // one query fewer, a mask, or the switch: the pair kernel, no scratch
                expect_plan("single 12 pairs", gh::ivfflat_scan_plan(shape(3, D.d, et, false, false, false, false, tails), on), PAIR,
                            false, 0, 0);
                expect_plan("single masked", gh::ivfflat_scan_plan(shape(4, D.d, et, false, true, false, false, tails), on), PAIR,
                            false, 0, 0);
                expect_plan("single no_lm", gh::ivfflat_scan_plan(shape(4, D.d, et, false, false, false, false, tails), off), PAIR,
                            false, 0, 0);
                // (a single handle has no sparse store; the flags change nothing if they are set)
                expect_plan("single sparse flags", gh::ivfflat_scan_plan(shape(4, D.d, et, false, false, true, true, tails), on), want,
                            false, bytes, 0);
            }
}

static void check_shard() {
    IvfflatSwitches on, off;
    off.no_lm = true;
    for (const Dim& D : DIMS)
        for (int et = 0; et <= 4; et++)
            for (int tails = 0; tails <= 1; tails++)
                for (int masked = 0; masked <= 1; masked++)
                    for (int sparse = 0; sparse <= 1; sparse++) {
                        // shared lists: the length's list-major form, under a mask too (over the masked length table); the
                        // tail switch changes nothing; room for the table is reserved mask or not
                        const bool lm = D.lm != PAIR;
                        expect_plan("shard", gh::ivfflat_scan_plan(shape(4, D.d, et, true, masked, sparse, false, tails), on), D.lm,
                                    lm && masked, lm ? SHARD_BYTES : 0, lm ? SHARD_MLEN_OFF : 0);
                        expect_plan("shard 12 pairs", gh::ivfflat_scan_plan(shape(3, D.d, et, true, masked, sparse, false, tails), on),
                                    PAIR, false, 0, 0);
                        expect_plan("shard no_lm", gh::ivfflat_scan_plan(shape(4, D.d, et, true, masked, sparse, false, tails), off),
                                    PAIR, false, 0, 0);
                        // a sparse store that never took a row: nothing is scanned, whatever else holds
                        expect_plan("shard empty", gh::ivfflat_scan_plan(shape(4, D.d, et, true, masked, true, true, tails), on), FILL,
                                    false, 0, 0);
                        expect_plan("shard empty 12 pairs, no_lm",
                                    gh::ivfflat_scan_plan(shape(3, D.d, et, true, masked, true, true, tails), off), FILL, false, 0, 0);
                    }
}

// where the two drivers differ, one line each
static void check_asymmetries() {
    const IvfflatSwitches sw;
    expect_plan("single, masked, d 16", gh::ivfflat_scan_plan(shape(4, 16, 0, false, true, false, false, false), sw), PAIR, false, 0, 0);
    expect_plan("shard, masked, d 16", gh::ivfflat_scan_plan(shape(4, 16, 0, true, true, false, false, false), sw), FIXED, true, 240,
                208);
    expect_plan("shard, d 20, lm_tails", gh::ivfflat_scan_plan(shape(4, 20, 0, true, false, false, false, true), sw), PAIR, false, 0, 0);
    expect_plan("single, d 20, lm_tails", gh::ivfflat_scan_plan(shape(4, 20, 0, false, false, false, false, true), sw), TAIL, false,
                196, 0);
    expect_plan("single, d 20, lm_tails, sq8", gh::ivfflat_scan_plan(shape(4, 20, 4, false, false, false, false, true), sw), PAIR,
                false, 0, 0);
    expect_plan("single, d 48, sq8", gh::ivfflat_scan_plan(shape(4, 48, 4, false, false, false, false, false), sw), SLICED, false, 196,
                0);
    // the scratch grows with the chunk: 64 queries x 4 probes over 8 lists = (256 + 33) ints
    expect_plan("single, 64 queries", gh::ivfflat_scan_plan(shape(64, 128, 0, false, false, false, false, false), sw), FIXED, false,
                1156, 0);
    expect_plan("shard, 64 queries", gh::ivfflat_scan_plan(shape(64, 128, 0, true, true, false, false, false), sw), FIXED, true,
                1168 + 32, 1168);
}

static void check_pairs_predicate() {
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(4, 4, 8), 1);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(3, 4, 8), 0);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(1, 1, 1), 0);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(2, 1, 1), 1);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(128, 32, 2048), 1);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists(127, 32, 2048), 0);
    EXPECT_EQ("pairs", gh::ivfflat_pairs_share_lists((int64_t)1 << 31, 1024, 1 << 30), 1);   // no 32-bit product anywhere
}

// the values tests/test_ivfflat_lm_cpu.py and test_ivfflat_lm_tails_cpu.py assert through the library
static void check_shapes() {
    int kind = -1, slab = -1, qtile = -1;
    const int fixed[] = {16, 32, 64, 96, 128};
    for (int d : fixed) {
        EXPECT_EQ("lm_shape", gh::ivfflat_lm_shape(d, &kind, &slab, &qtile), 1);
        EXPECT_EQ("lm_shape", kind, 1);
        EXPECT_EQ("lm_shape", slab, d);
        EXPECT_EQ("lm_shape", qtile, 32);
        EXPECT_EQ("lm_supported", gh::ivfflat_lm_supported(d), 1);
    }
    const int sliced[] = {48, 80, 112, 144, 256, 768, 1024, 4080, 4096};
    for (int d : sliced) {
        EXPECT_EQ("lm_shape", gh::ivfflat_lm_shape(d, &kind, &slab, &qtile), 2);
        EXPECT_EQ("lm_shape", kind, 2);
        EXPECT_EQ("lm_shape", slab, 128);
        EXPECT_EQ("lm_shape", qtile, 16);
        EXPECT_EQ("lm_supported", gh::ivfflat_lm_supported(d), 0);
    }
    const int none[] = {-16, 0, 1, 8, 15, 17, 20, 100, 130, 4095, 4097, 4112, 8192};
    for (int d : none) {
        EXPECT_EQ("lm_shape", gh::ivfflat_lm_shape(d, &kind, &slab, &qtile), 0);
        EXPECT_EQ("lm_shape", kind, 0);
        EXPECT_EQ("lm_shape", slab, 0);
        EXPECT_EQ("lm_shape", qtile, 0);
    }
    // the tail form: kind 3 for 1 <= d <= 4096 with d % 16 != 0; load_bytes = gcd(16, d * elem_bytes) whatever the kind
    struct { int d, esz, kind, load; } const tails[] = {
        {1, 4, 3, 4},   {1, 2, 3, 2},   {1, 1, 3, 1},    {2, 4, 3, 8},    {4, 4, 3, 16},   {20, 4, 3, 16},  {20, 2, 3, 8},
        {20, 1, 3, 4},  {100, 4, 3, 16}, {100, 2, 3, 8}, {100, 1, 3, 4},  {130, 4, 3, 8},  {130, 2, 3, 4},  {130, 1, 3, 2},
        {4095, 4, 3, 4}, {4095, 1, 3, 1}, {8, 1, 3, 8},  {16, 4, 0, 16},  {128, 1, 0, 16}, {4096, 2, 0, 16}, {0, 4, 0, 16},
        {4097, 4, 0, 4}, {4100, 1, 0, 4}, {-3, 4, 0, 4}};
    for (const auto& t : tails) {
        int load = -1;
        EXPECT_EQ("tail_shape", gh::ivfflat_lm_tail_shape(t.d, t.esz, &kind, &load, &qtile), t.kind);
        EXPECT_EQ("tail_shape", kind, t.kind);
        EXPECT_EQ("tail_shape", load, t.load);
        EXPECT_EQ("tail_shape", qtile, 16);
    }
    EXPECT_EQ("scratch", gh::ivfflat_lm_scratch_bytes(4, 4, 8), 196);
    EXPECT_EQ("scratch", gh::ivfflat_lm_scratch_bytes(4096, 32, 4096), (4096 * 32 + 4 * 4096 + 1) * 4);
    EXPECT_EQ("scratch", gh::ivfflat_lm_scratch_bytes(1 << 20, 1024, 1), ((1ll << 30) + 5) * 4);   // no 32-bit product
    EXPECT_EQ("constants", gh::FL_QT, 32);
    EXPECT_EQ("constants", gh::FS_QT, 16);
    EXPECT_EQ("constants", gh::FS_SLAB, 128);
}

static void check_switches() {
    unsetenv("GAMMA_HIP_NO_IVFFLAT_LM");
    unsetenv("GAMMA_HIP_NO_SMALL_PATH");
    IvfflatSwitches s = IvfflatSwitches::from_env();
    EXPECT_EQ("switches", s.no_lm, 0);
    EXPECT_EQ("switches", s.no_small_path, 0);
    setenv("GAMMA_HIP_NO_IVFFLAT_LM", "1", 1);
    s = IvfflatSwitches::from_env();
    EXPECT_EQ("switches", s.no_lm, 1);
    EXPECT_EQ("switches", s.no_small_path, 0);
    unsetenv("GAMMA_HIP_NO_IVFFLAT_LM");
    setenv("GAMMA_HIP_NO_SMALL_PATH", "", 1);   // set is set, whatever the value
    s = IvfflatSwitches::from_env();
    EXPECT_EQ("switches", s.no_lm, 0);
    EXPECT_EQ("switches", s.no_small_path, 1);
    const IvfflatSwitches& g = IvfflatSwitches::get();   // read once: a later change of the environment does not reach it
    unsetenv("GAMMA_HIP_NO_SMALL_PATH");
    EXPECT_EQ("switches", IvfflatSwitches::get().no_small_path, 1);
    EXPECT_EQ("switches", &g == &IvfflatSwitches::get(), 1);
}

int main() {
    check_single_handle();
    check_shard();
    check_asymmetries();
    check_pairs_predicate();
    check_shapes();
    check_switches();
    if (g_failed) {
        printf("%d expectation(s) failed\n", g_failed);
        return 1;
    }
    printf("ivfflat plan ok\n");
    return 0;
}
