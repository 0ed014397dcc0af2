// group_protocol.cc -- TEST INFRASTRUCTURE: the list-sharded search protocol of the REAL gamma_amd/csrc/gamma_hip_group.cpp
// (a thread per member, the meeting points, the go / no-go snapshots, the slice offsets of the exchanges, the tie rounds) on a
// CPU, under ThreadSanitizer and under AddressSanitizer + UBSan, over BOTH transports and W = 2, 3, 4 members.  Nothing here
// computes a search: every list-shard entry of the members is SCRIPTED -- it writes a recognisable pattern, checks that what the
// group handed it is the pattern its peers wrote for exactly the rows it should see, and can be told to fail on one chosen
// member.  The HIP calls of the group go to fakehip/ (host memory, copies on the calling thread); its RCCL calls to fakerccl/, a
// stand-in communicator linked into this program under RCCL's soname (strict about counts, the in-place rule, the pairing of
// sends and recvs and "all ranks enter a collective"; fakerccl_selftest.cc holds it to that); the other entries of the members
// come from stub_abi.cpp (-DGAMMA_STUB_SCRIPTED_SHARD leaves the list-shard ones to this file).
//
// Clean runs, per W and per transport: both families, IVFPQ with raw rows replicated / sharded / has_rank = 0 and with the
// maximum as the bound reduction (inner product), host and _device entry points, shapes with a padded last slice, an empty
// slice, one query, and two tie rounds of one owner.  After EVERY search the stand-in's counters must say which transport
// carried it: over RCCL 2 all-gathers, 1 all-reduce and the sends / recvs of its slices and columns per member and no
// bound_combine; over copies, for IVFFLAT members and after a refused ncclCommInitAll, no RCCL call at all.  The program stops
// at once if the group's first search did not form its communicator in the stand-in.  Failure sweep (W = 3, both transports):
// every scripted entry x every member; the call must RETURN that member's error (a member that skipped a meeting point, or
// entered a collective its peers skipped, would leave them waiting: the watchdog reports the case and aborts) and the next
// call on the same group must be correct.
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <string>
#include <vector>

#include "../../gamma_amd/csrc/gamma_hip_group_ext.h"
#include "../../include/gamma_hip.h"
#include "fakerccl/fakerccl.h"

namespace {

constexpr int D = 4, NLIST = 6, K = 2, RECALL = 5;
int W = 0, P = 3;   // members of the group under test; probes of the call under way (main thread, between calls)

enum Entry {
    COARSE, SCAN_BEFORE_REDUCE, SCAN, BOUND_COMBINE, CUT_FLAGS, SHARD_EXACT, SET_SHARD_FLAGS, MERGE, MERGE_FLAGGED, GATHER_ROWS,
    EXPORT_ROWS, EXPORT, EXPORT_EXACT, REPLAY, N_ENTRIES
};
const char* const kEntryName[N_ENTRIES] = {"coarse", "scan-before-reduce", "scan", "bound_combine", "cut_flags", "shard_exact",
                                           "set_shard_flags", "merge", "merge_flagged", "gather_rows", "export_rows", "export",
                                           "export_exact", "replay"};

struct Round { int o, f0, nf; };
typedef std::vector<std::vector<int32_t>> Flags;

// what the call under way looks like (written by the main thread between calls, read by the members' threads during one)
struct Call {
    bool pq = true, rs = false;
    int nq = 0, per = 0, width = 0;
    int take_max = 0;                  // the reduction the scripted scan asks for (inner product: the maximum)
    Flags flagged;                     // per member: slice-local indices, what merge_flagged answers
    std::vector<Round> rounds;
    int64_t stride = 0;
    int fail_entry = -1, fail_member = -1, fail_skip = 0, fail_code = 0;
    std::vector<std::array<int, N_ENTRIES>> calls;   // (row m: member m's thread only)
    std::vector<int> next_round, round;
    bool check() const { return fail_entry < 0; }   // the stub-side checks are those of a clean run
} C;

std::vector<gamma_hip_index*> g_member;
std::atomic<int> g_bad{0};
thread_local int tl_member = -1;
char g_case[160] = "setup";

int who(gamma_hip_index* h) {
    for (int i = 0; i < W; i++)
        if (g_member[i] == h) return i;
    abort();
}
int q0_of(int m) { return std::min(C.nq, m * C.per); }
int nql_of(int m) { return std::min(C.nq, q0_of(m) + C.per) - q0_of(m); }

void bad(const char* what, int m, long a, long b) {
    if (g_bad++ < 20) fprintf(stderr, "CHECK FAILED [%s] %s (member %d, at %ld / %ld)\n", g_case, what, m, a, b);
}
#define CHECK(cond, what, m, a, b) do { if (C.check() && !(cond)) bad(what, m, (long)(a), (long)(b)); } while (0)

// true: this call of `e` by member m is the one to fail
bool inject(int e, int m) {
    const int n = C.calls[m][e]++;
    return e == C.fail_entry && m == C.fail_member && n == C.fail_skip;
}

// ---- the patterns ----
float px(int q, int c) { return (float)(q * D + c) + 0.5f; }
float pcd(int q, int p) { return (float)(1000 * q + p); }
int32_t ppr(int q, int p) { return q * P + p; }
float pcand(int m, int q, int r) { return (float)(m * 1000000 + q * C.width + r); }
float pexact(int m, int q, int r) { return pcand(m, q, r) + 0.5f; }
uint8_t pcut(int m, int q) { return (uint8_t)((m * 31 + q) % 251); }
float pbound(int q) { return (float)(100 * q); }   // reduced over the members; member m's own is + m
float preduced(int q) { return pbound(q) + (C.take_max ? (float)(W - 1) : 0.f); }   // the minimum (L2) / the maximum (inner product)
float pmerged(int q, int c) { return (float)(5000000 + q * K + c); }
float preplayed(int q, int c) { return (float)(7000000 + q * K + c); }
float pexp(int m, int round, int f, int c) { return (float)(m * 1000000 + round * 10000 + f * (int)C.stride + c); }
int32_t poff(int m, int f, int p) { return m * 1000 + f * (P + 1) + p; }
int64_t prowmax(int m) { return 1 + 3 * m; }

// ---- the scripted entries, one per step of the protocol (superset signatures; unused arguments null) ----
int s_coarse(gamma_hip_index* h, int n, const float* x, float* cd, int32_t* pr) {
    const int m = who(h), q0 = q0_of(m);
    if (inject(COARSE, m)) return C.fail_code;
    CHECK(n == nql_of(m), "coarse: rows of the own slice", m, n, nql_of(m));
    for (int q = 0; q < n; q++) {
        for (int c = 0; c < D; c++) CHECK(x[q * D + c] == px(q0 + q, c), "coarse: query slice", m, q, c);
        for (int p = 0; p < P; p++) {
            cd[q * P + p] = pcd(q0 + q, p);
            pr[q * P + p] = ppr(q0 + q, p);
        }
    }
    return GAMMA_HIP_OK;
}

int s_scan(gamma_hip_index* h, int nq, const float* x, const float* cd, const int32_t* pr, int k, float* rdis, int64_t* rids,
           float* bound, gamma_hip_bound_reduce_fn reduce, void* user) {
    const int m = who(h);
    tl_member = m;
    if (C.pq && inject(SCAN_BEFORE_REDUCE, m)) return C.fail_code;
    CHECK(nq == C.nq && k == K, "scan: the whole batch", m, nq, k);
    for (int q = 0; q < nq; q++) {   // every member's slice of the assignment arrived where it belongs
        for (int c = 0; c < D; c++) CHECK(x[q * D + c] == px(q, c), "scan: batch", m, q, c);
        for (int p = 0; p < P; p++) CHECK(cd[q * P + p] == pcd(q, p) && pr[q * P + p] == ppr(q, p), "scan: assignment", m, q, p);
        for (int r = 0; r < C.width; r++) {
            rdis[(size_t)q * C.width + r] = pcand(m, q, r);
            rids[(size_t)q * C.width + r] = (int64_t)pcand(m, q, r);
        }
    }
    if (C.pq) {
        for (int q = 0; q < nq; q++) bound[q] = pbound(q) + (float)m;
        if (reduce(user, bound, nq, C.take_max, nullptr) != 0) return C.fail_code ? C.fail_code : GAMMA_HIP_EDEVICE;   // exactly once
        for (int q = 0; q < nq; q++) CHECK(bound[q] == preduced(q), "scan: reduced bound", m, q, 0);
    }
    if (inject(SCAN, m)) return C.fail_code;
    return GAMMA_HIP_OK;
}

int s_export_rows(gamma_hip_index* h, int nf, const int32_t* spr, int64_t* mine) {
    const int m = who(h);
    if (inject(EXPORT_ROWS, m)) return C.fail_code;
    C.round[m] = C.next_round[m]++;
    if (C.check()) {
        const Round& r = C.rounds[C.round[m]];
        CHECK(nf == r.nf, "export_rows: round size", m, nf, r.nf);
        for (int f = 0; f < nf; f++)
            for (int p = 0; p < P; p++)
                CHECK(spr[f * P + p] == ppr(q0_of(r.o) + C.flagged[r.o][r.f0 + f], p), "export_rows: tie input probe", m, f, p);
    }
    *mine = prowmax(m);
    return GAMMA_HIP_OK;
}

int s_export(gamma_hip_index* h, int nf, const float* sx, const float* scd, const int32_t* spr, int64_t stride, float* vals,
             int64_t* ids, int32_t* off) {
    const int m = who(h);
    if (inject(EXPORT, m)) return C.fail_code;
    CHECK(stride == C.stride, "export: the common 4-aligned stride", m, stride, C.stride);
    if (C.check()) {
        const Round& r = C.rounds[C.round[m]];
        for (int f = 0; f < nf; f++) {
            const int q = q0_of(r.o) + C.flagged[r.o][r.f0 + f];
            for (int c = 0; c < D; c++) CHECK(sx[f * D + c] == px(q, c), "export: tie input x", m, f, c);
            for (int p = 0; p < P; p++) CHECK(spr[f * P + p] == ppr(q, p) && (!scd || scd[f * P + p] == pcd(q, p)), "export: tie input", m, f, p);
        }
    }
    for (int f = 0; f < nf; f++) {
        for (int c = 0; c < stride; c++) {
            vals[f * stride + c] = pexp(m, C.round[m], f, c);
            ids[f * stride + c] = (int64_t)pexp(m, C.round[m], f, c);
        }
        for (int p = 0; p <= P; p++) off[f * (P + 1) + p] = poff(m, f, p);
    }
    return GAMMA_HIP_OK;
}

int s_merge(gamma_hip_index* h, const float* x, int nsh, int per, int k, const float* adis, const int64_t* aids, const float* aex,
            int q0, int nql, float* Dd, int64_t* Id) {
    const int m = who(h), s0 = q0_of(m);
    if (inject(MERGE, m)) return C.fail_code;
    CHECK(nsh == W && per == C.per && k == K && q0 == 0 && nql == nql_of(m), "merge: shape", m, per, nql);
    CHECK((aex != nullptr) == C.rs, "merge: exact distances travel with sharded rows only", m, 0, 0);
    for (int q = 0; q < nql; q++) {
        for (int c = 0; x && c < D; c++) CHECK(x[q * D + c] == px(s0 + q, c), "merge: query slice", m, q, c);
        for (int j = 0; j < W; j++)   // slot j: what member j wrote for the rows of THIS member's slice
            for (int r = 0; r < C.width; r++) {
                const size_t at = ((size_t)j * per + q) * C.width + r;
                CHECK(adis[at] == pcand(j, s0 + q, r) && aids[at] == (int64_t)pcand(j, s0 + q, r), "merge: candidates", m, j, q);
                CHECK(!aex || aex[at] == pexact(j, s0 + q, r), "merge: exact distances", m, j, q);
            }
        for (int c = 0; c < K; c++) {
            Dd[q * K + c] = pmerged(s0 + q, c);
            Id[q * K + c] = (int64_t)pmerged(s0 + q, c);
        }
    }
    return GAMMA_HIP_OK;
}

int s_replay(gamma_hip_index* h, int nsh, int nf, const float* x, int64_t stride, const float* av, const int64_t* ai, const int32_t* ao,
             const float* ae, int k, const int32_t* list, float* Dd, int64_t* Id) {
    const int m = who(h), s0 = q0_of(m);
    if (inject(REPLAY, m)) return C.fail_code;
    if (C.check()) {
        const Round& r = C.rounds[C.round[m]];
        CHECK(r.o == m && nf == r.nf && nsh == W && k == K && stride == C.stride, "replay: at the owner of the round", m, r.o, nf);
        CHECK(list == C.flagged[m].data() + r.f0, "replay: the round's part of the list", m, r.f0, 0);
        CHECK((ae != nullptr) == C.rs, "replay: exact distances travel with sharded rows only", m, 0, 0);
        CHECK(x[0] == px(s0, 0), "replay: query slice", m, 0, 0);
        for (int j = 0; j < W; j++)
            for (int f = 0; f < nf; f++) {
                for (int c = 0; c < stride; c++) {
                    const size_t at = ((size_t)j * nf + f) * stride + c;
                    CHECK(av[at] == pexp(j, C.round[m], f, c) && ai[at] == (int64_t)pexp(j, C.round[m], f, c), "replay: exports", m, j, f);
                    CHECK(!ae || ae[at] == pexp(j, C.round[m], f, c) + 0.25f, "replay: exported exact distances", m, j, f);
                }
                for (int p = 0; p <= P; p++) CHECK(ao[((size_t)j * nf + f) * (P + 1) + p] == poff(j, f, p), "replay: offsets", m, j, f);
            }
    }
    for (int f = 0; f < nf; f++)
        for (int c = 0; c < K; c++) {
            Dd[list[f] * K + c] = preplayed(s0 + list[f], c);
            Id[list[f] * K + c] = (int64_t)preplayed(s0 + list[f], c);
        }
    return GAMMA_HIP_OK;
}

// ---- the IVFFLAT table: the scripted entries under the signatures of gamma_group_ext::ShardFamily ----
int f_search_device(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, int, float*, int64_t*) { return GAMMA_HIP_EUNSUPPORTED; }
int f_coarse(gamma_hip_index* h, const gamma_hip_search_params*, int n, const float* x, float* cd, int32_t* pr) { return s_coarse(h, n, x, cd, pr); }
int f_scan(gamma_hip_index* h, const gamma_hip_search_params*, int nq, const float* x, const float* cd, const int32_t* pr, int k, float* rdis,
           int64_t* rids, float* bound, gamma_hip_bound_reduce_fn reduce, void*) {
    CHECK(!bound && !reduce, "scan: no bound reduction for IVFFLAT", who(h), 0, 0);
    return s_scan(h, nq, x, cd, pr, k, rdis, rids, nullptr, nullptr, nullptr);
}
int f_export_rows(gamma_hip_index* h, const gamma_hip_search_params*, int nf, const int32_t* spr, int64_t* mine) { return s_export_rows(h, nf, spr, mine); }
int f_export(gamma_hip_index* h, const gamma_hip_search_params*, int nf, const float* sx, const float* scd, const int32_t* spr, int64_t stride,
             float* vals, int64_t* ids, int32_t* off) {
    CHECK(!scd, "export: no coarse distances for IVFFLAT", who(h), 0, 0);
    return s_export(h, nf, sx, nullptr, spr, stride, vals, ids, off);
}
int f_merge(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int per, const float* x, int k, const float* adis, const int64_t* aids,
            int q0, int nql, float* Dd, int64_t* Id) {
    return s_merge(h, x, nsh, per, k, adis, aids, nullptr, q0, nql, Dd, Id);
}
int f_replay(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int nf, const float* x, int64_t stride, const float* av, const int64_t* ai,
             const int32_t* ao, int k, const int32_t* list, float* Dd, int64_t* Id) {
    return s_replay(h, nsh, nf, x, stride, av, ai, ao, nullptr, k, list, Dd, Id);
}
const gamma_group_ext::ShardFamily kFlatFamily = {"ivfflat_search", f_search_device, f_coarse, f_scan, f_export_rows, f_export, f_merge, f_replay,
                                                  false, false, false, false, false};

// sharded raw rows: the group only asks whether the (empty) stores may change form
int r_drop(gamma_hip_index*, int64_t, const int64_t*) { return GAMMA_HIP_OK; }
int64_t r_count(gamma_hip_index*) { return 0; }
int r_clear(gamma_hip_index*) { return GAMMA_HIP_OK; }
const gamma_group_ext::RawOps kRawOps = {r_drop, r_count, r_clear};

}  // namespace

// ---- the list-shard entries of the public ABI that the group calls by name (IVFPQ members, and what both families share) ----
extern "C" {
int gamma_hip_bound_combine(void*, float* acc, const float* in, int n, int take_max) {
    if (inject(BOUND_COMBINE, tl_member)) return C.fail_code;
    for (int q = 0; q < n; q++) acc[q] = take_max ? std::max(acc[q], in[q]) : std::min(acc[q], in[q]);
    return GAMMA_HIP_OK;
}
int gamma_hip_raw_put(gamma_hip_index*, int64_t n, const int64_t*, const float*) { return n == 0 ? GAMMA_HIP_OK : GAMMA_HIP_EUNSUPPORTED; }
int gamma_hip_ivfpq_coarse_device(gamma_hip_index* h, const gamma_hip_search_params*, int n, const float* x, float* cd, int32_t* pr) {
    return s_coarse(h, n, x, cd, pr);
}
int gamma_hip_ivfpq_search_shard_bounded(gamma_hip_index* h, const gamma_hip_search_params*, int nq, const float* x, const float* cd,
                                         const int32_t* pr, int k, float* rdis, int64_t* rids, float* bound, gamma_hip_bound_reduce_fn reduce,
                                         void* user) {
    return s_scan(h, nq, x, cd, pr, k, rdis, rids, bound, reduce, user);
}
int gamma_hip_ivfpq_search_shard_preassigned(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, const float*, const int32_t*,
                                             int, float*, int64_t*) { return GAMMA_HIP_EUNSUPPORTED; }
int gamma_hip_ivfpq_shard_cut_flags(gamma_hip_index* h, int nq, uint8_t* cutf) {
    const int m = who(h);
    if (inject(CUT_FLAGS, m)) return C.fail_code;
    for (int q = 0; q < nq; q++) cutf[q] = pcut(m, q);
    return GAMMA_HIP_OK;
}
int gamma_hip_ivfpq_shard_exact(gamma_hip_index* h, const gamma_hip_search_params*, int nq, const float*, const int64_t* rids, int R, float* rex) {
    const int m = who(h);
    if (inject(SHARD_EXACT, m)) return C.fail_code;
    CHECK(C.rs && R == C.width && nq == C.nq, "shard_exact: only with sharded rows", m, R, nq);
    for (int q = 0; q < nq; q++)
        for (int r = 0; r < R; r++) {
            CHECK(rids[(size_t)q * R + r] == (int64_t)pcand(m, q, r), "shard_exact: the scan's ids", m, q, r);
            rex[(size_t)q * R + r] = pexact(m, q, r);
        }
    return GAMMA_HIP_OK;
}
int gamma_hip_ivfpq_merge_set_shard_flags(gamma_hip_index* h, const uint8_t* cutall) {
    const int m = who(h);
    if (inject(SET_SHARD_FLAGS, m)) return C.fail_code;
    for (int j = 0; j < W; j++)
        for (int q = 0; q < nql_of(m); q++) CHECK(cutall[(size_t)j * C.per + q] == pcut(j, q0_of(m) + q), "cut flags of the own slice", m, j, q);
    return GAMMA_HIP_OK;
}
int gamma_hip_ivfpq_merge_rerank(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int per, const float* x, int k, const float* adis,
                                 const int64_t* aids, int q0, int nql, float* Dd, int64_t* Id) {
    return s_merge(h, x, nsh, per, k, adis, aids, nullptr, q0, nql, Dd, Id);
}
int gamma_hip_ivfpq_merge_rerank_exact(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int per, const float* x, int k,
                                       const float* adis, const int64_t* aids, const float* aex, int q0, int nql, float* Dd, int64_t* Id) {
    return s_merge(h, x, nsh, per, k, adis, aids, aex, q0, nql, Dd, Id);
}
int gamma_hip_ivfpq_merge_flagged(gamma_hip_index* h, int* nf, const int32_t** list) {
    const int m = who(h);
    if (inject(MERGE_FLAGGED, m)) return C.fail_code;
    *nf = (int)C.flagged[m].size();
    *list = C.flagged[m].data();
    return GAMMA_HIP_OK;
}
int gamma_hip_gather_rows(gamma_hip_index* h, const void* src, int row_words, const int32_t* list, int n, void* dst) {
    const int m = who(h);
    if (inject(GATHER_ROWS, m)) return C.fail_code;
    if (C.check()) {
        const Round& r = C.rounds[C.next_round[m]];   // (the owner gathers before anybody counts the round)
        CHECK(r.o == m && n == r.nf && list == C.flagged[m].data() + r.f0, "gather: the round's part of the owner's list", m, r.o, n);
    }
    for (int f = 0; f < n; f++)
        memcpy((char*)dst + (size_t)f * row_words * 4, (const char*)src + (size_t)list[f] * row_words * 4, (size_t)row_words * 4);
    return GAMMA_HIP_OK;
}
int gamma_hip_ivfpq_shard_export_rows(gamma_hip_index* h, const gamma_hip_search_params*, int nf, const int32_t* spr, int64_t* mine) {
    return s_export_rows(h, nf, spr, mine);
}
int gamma_hip_ivfpq_shard_export(gamma_hip_index* h, const gamma_hip_search_params*, int nf, const float* sx, const float* scd, const int32_t* spr,
                                 int64_t stride, float* vals, int64_t* ids, int32_t* off) {
    return s_export(h, nf, sx, scd, spr, stride, vals, ids, off);
}
int gamma_hip_ivfpq_shard_export_exact(gamma_hip_index* h, const gamma_hip_search_params*, int nf, const float*, const float* vals, const int64_t*,
                                       const int32_t*, int64_t stride, const float* sbd, float* ex) {
    const int m = who(h);
    if (inject(EXPORT_EXACT, m)) return C.fail_code;
    if (C.check()) {
        const Round& r = C.rounds[C.round[m]];
        CHECK(C.rs, "export_exact: only with sharded rows", m, 0, 0);
        for (int f = 0; f < nf; f++) CHECK(sbd[f] == preduced(q0_of(r.o) + C.flagged[r.o][r.f0 + f]),"export_exact: the flagged queries' bounds", m, f, 0);
    }
    for (int64_t t = 0; t < (int64_t)nf * stride; t++) ex[t] = vals[t] + 0.25f;
    return GAMMA_HIP_OK;
}
int gamma_hip_ivfpq_merge_replay(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int nf, const float* x, int64_t stride, const float* av,
                                 const int64_t* ai, const int32_t* ao, int k, const int32_t* list, float* Dd, int64_t* Id) {
    return s_replay(h, nsh, nf, x, stride, av, ai, ao, nullptr, k, list, Dd, Id);
}
int gamma_hip_ivfpq_merge_replay_exact(gamma_hip_index* h, const gamma_hip_search_params*, int nsh, int nf, const float* x, int64_t stride,
                                       const float* av, const int64_t* ai, const int32_t* ao, const float* ae, int k, const int32_t* list, float* Dd,
                                       int64_t* Id) {
    return s_replay(h, nsh, nf, x, stride, av, ai, ao, ae, k, list, Dd, Id);
}
}  // extern "C"

namespace {

void on_alarm(int) {   // a member missed a meeting point (or entered a collective its peers skipped): its peers wait for ever
    const char a[] = "\nWATCHDOG: the call did not return -- ";
    (void)!write(2, a, sizeof(a) - 1);
    (void)!write(2, g_case, strlen(g_case));
    (void)!write(2, "\n", 1);
    _exit(3);
}

struct Cfg { const char* name; bool pq, raw_sharded; int has_rank; bool ip; };

// which transport the group is set to, and whether a communicator stands behind it (main thread)
enum Transport { COPIES = 0, RCCL = 1, FALLBACK = 2, N_TRANSPORTS };
const char* const kTransportName[N_TRANSPORTS] = {"copies", "rccl", "rccl-refused"};
int g_transport = COPIES;

gamma_hip_group* G = nullptr;
int n_calls = 0, n_cases = 0, n_failures = 0;
int n_clean[5][N_TRANSPORTS], n_injected[5][N_TRANSPORTS];   // [W][transport]

// the stand-in's counters of member m's communicator (none formed: zeros)
fakerccl_counts counts_of(int m) {
    fakerccl_counts n = {0, 0, 0, 0, 0};
    void* c = fakerccl_live_comm(m);
    if (c && (fakerccl_comm_rank(c) != m || fakerccl_get_counts(c, &n) != 0)) bad("transport: the live communicators are not this group's, in rank order", m, 0, 0);
    return n;
}

// one search of nq queries; flag[m]: slice-local queries member m's merge flags.  Returns the call's code; results checked when OK.
// Whatever the outcome, the stand-in's counters must say that the transport the group is set to carried the call, and no other.
int search(const Cfg& cfg, int nq, bool device, const Flags& flag, int fail_entry = -1, int fail_member = -1, int fail_skip = 0, int probes = 3) {
    P = probes;
    C.pq = cfg.pq;
    C.rs = cfg.pq && cfg.raw_sharded && cfg.has_rank != 0;
    C.take_max = cfg.ip ? 1 : 0;
    C.nq = nq;
    C.per = (nq + W - 1) / W;
    C.width = cfg.pq ? std::max(RECALL, K) : K;
    C.rounds.clear();
    C.flagged = flag;
    for (int o = 0; o < W; o++)
        for (int f0 = 0; f0 < (int)flag[o].size(); f0 += 256) C.rounds.push_back({o, f0, std::min(256, (int)flag[o].size() - f0)});
    C.stride = (prowmax(W - 1) + 3) & ~(int64_t)3;
    C.fail_entry = fail_entry;
    C.fail_member = fail_member;
    C.fail_skip = fail_skip;
    C.fail_code = GAMMA_HIP_EFULL;
    C.calls.assign(W, std::array<int, N_ENTRIES>());
    C.next_round.assign(W, 0);
    C.round.assign(W, 0);
    gamma_hip_search_params p;
    memset(&p, 0, sizeof(p));
    p.metric = cfg.ip ? GAMMA_HIP_METRIC_IP : GAMMA_HIP_METRIC_L2;
    p.nprobe = P;
    p.recall_num = RECALL;
    p.has_rank = cfg.has_rank;
    p.coarse_mode = -1;
    std::vector<float> x((size_t)nq * D), Dd((size_t)nq * K, -1.f);
    std::vector<int64_t> Id((size_t)nq * K, -1);
    for (int q = 0; q < nq; q++)
        for (int c = 0; c < D; c++) x[q * D + c] = px(q, c);
    std::vector<fakerccl_counts> before(W);
    for (int m = 0; m < W; m++) before[m] = counts_of(m);
    int64_t t0[2], t1[2];
    gamma_hip_group_transport(G, t0);
    alarm(60);
    const int rc = cfg.pq ? (device ? gamma_hip_group_ivfpq_search_device : gamma_hip_group_ivfpq_search)(G, &p, nq, x.data(), K, Dd.data(), Id.data())
                          : (device ? gamma_hip_group_ivfflat_search_device : gamma_hip_group_ivfflat_search)(G, &p, nq, x.data(), K, Dd.data(), Id.data());
    alarm(0);
    n_calls++;
    // ---- which transport carried it (a communicator formed by this very call starts from zero: `before` is zeros then) ----
    gamma_hip_group_transport(G, t1);
    const bool through_rccl = g_transport == RCCL && cfg.pq;
    const int ncols = 3 + (C.rs ? 1 : 0);   // candidate distances, ids, cut flags; exact distances with sharded rows
    int owners = 0;                         // members with a slice: everybody sends them their rows
    for (int j = 0; j < W; j++) owners += nql_of(j) > 0;
    if (t1[1] - t0[1] != (through_rccl ? 1 : 0)) bad("transport: rccl_searches moved by", -1, t1[1] - t0[1], through_rccl);
    if (t1[0] != (g_transport == RCCL ? 1 : 0)) bad("transport: a communicator in use", -1, t1[0], g_transport);
    fakerccl_counts first = {0, 0, 0, 0, 0};
    for (int m = 0; m < W; m++) {
        const fakerccl_counts a = counts_of(m);
        const fakerccl_counts n = {a.all_gather - before[m].all_gather, a.all_reduce - before[m].all_reduce, a.send - before[m].send,
                                   a.recv - before[m].recv, a.group_end - before[m].group_end};
        if (m == 0) first = n;
        if (!through_rccl) {   // IVFFLAT, or the group set to copies, or no communicator: nothing goes through the library
            if (n.all_gather || n.all_reduce || n.send || n.recv || n.group_end) bad("transport: RCCL calls in a search over copies", m, n.all_gather, n.send);
            if (C.check() && cfg.pq && C.calls[m][BOUND_COMBINE] != W - 1) bad("transport: bound_combine calls over copies", m, C.calls[m][BOUND_COMBINE], W - 1);
            continue;
        }
        if (C.calls[m][BOUND_COMBINE] != 0) bad("transport: bound_combine belongs to the copy path", m, C.calls[m][BOUND_COMBINE], 0);
        // all members enter a collective, or none (a member alone in one never comes back: the watchdog's case)
        if (n.all_gather != first.all_gather || n.all_reduce != first.all_reduce) bad("transport: collectives entered by some members only", m, n.all_gather, n.all_reduce);
        if (!C.check()) continue;
        if (n.all_gather != 2 || n.all_reduce != 1) bad("transport: 2 all-gathers and 1 all-reduce per member", m, n.all_gather, n.all_reduce);
        if (n.send != ncols * owners) bad("transport: sends = columns x members with a slice", m, n.send, ncols * owners);
        if (n.recv != (nql_of(m) > 0 ? ncols * W : 0)) bad("transport: recvs = columns x members, at a member with a slice", m, n.recv, ncols * W);
        if (n.group_end != 2) bad("transport: one group per exchange", m, n.group_end, 2);
    }
    if (rc != GAMMA_HIP_OK) return rc;
    int wrong = 0;
    for (int q = 0; q < nq; q++) {
        const int m = q / C.per, ql = q - m * C.per;
        const bool tie = std::find(flag[m].begin(), flag[m].end(), ql) != flag[m].end();
        for (int c = 0; c < K; c++) {
            const float want = tie ? preplayed(q, c) : pmerged(q, c);
            wrong += !(Dd[q * K + c] == want && Id[q * K + c] == (int64_t)want);
        }
    }
    if (wrong) {
        fprintf(stderr, "RESULTS WRONG [%s]: %d of %d values\n", g_case, wrong, nq * K);
        n_failures++;
    }
    return rc;
}

void clean(const Cfg& cfg, int nq, bool device, const Flags& flag, const char* shape, int probes = 3) {
    snprintf(g_case, sizeof(g_case), "clean W=%d %s %s %s nq=%d %s", W, kTransportName[g_transport], cfg.name, device ? "device" : "host", nq, shape);
    const int bad0 = g_bad.load();
    const int rc = search(cfg, nq, device, flag, -1, -1, 0, probes);
    int rounds_seen = 0;
    for (int m = 0; m < W; m++) rounds_seen += C.next_round[m] == (int)C.rounds.size();
    const std::string note = gamma_hip_group_transport_note(G);
    // an IVFFLAT search of a group set to RCCL runs over copies and the group says so
    const bool noted = cfg.pq || g_transport == COPIES || note.find("IVFFLAT search: peer copies") != std::string::npos;
    const bool ok = rc == GAMMA_HIP_OK && g_bad.load() == bad0 && rounds_seen == W && noted;
    n_cases++;
    n_clean[W][g_transport]++;
    if (!ok) {
        n_failures++;
        fprintf(stderr, "FAILED [%s]: rc %d (%s), %d of %d members saw every tie round, transport note \"%s\"\n", g_case, rc, gamma_hip_group_last_error(G),
                rounds_seen, W, note.c_str());
    }
    printf("%-88s %s (%zu tie rounds)\n", g_case, ok ? "ok" : "FAILED", C.rounds.size());
}

void failing(const Cfg& cfg, int e, int m, int skip, bool device, const Flags& flag) {
    snprintf(g_case, sizeof(g_case), "inject %s %s %s: %s fails at member %d (its call %d)", kTransportName[g_transport], cfg.name, device ? "device" : "host",
             kEntryName[e], m, skip);
    const int bad00 = g_bad.load();
    const int rc = search(cfg, 7, device, flag, e, m, skip);
    const std::string msg = gamma_hip_group_last_error(G);
    const bool returned = rc == GAMMA_HIP_EFULL && msg.rfind("member " + std::to_string(m) + ":", 0) == 0 && g_bad.load() == bad00;
    const int bad0 = g_bad.load(), fail0 = n_failures;
    const size_t len = strlen(g_case);
    snprintf(g_case + len, sizeof(g_case) - len, " -- the call after");
    const bool recovered = search(cfg, 7, device, flag) == GAMMA_HIP_OK && g_bad.load() == bad0 && n_failures == fail0;
    g_case[len] = 0;
    n_cases++;
    n_injected[W][g_transport]++;
    if (!returned || !recovered) n_failures++;
    printf("%-88s %s (%d, \"%s\"), %s\n", g_case, returned ? "returned with its error" : "WRONG ANSWER", rc, msg.c_str(),
           recovered ? "recovered" : "NOT RECOVERED");
}

std::vector<int32_t> upto(int n) {
    std::vector<int32_t> v(n);
    for (int t = 0; t < n; t++) v[t] = t;
    return v;
}

int set_transport(int t) {
    g_transport = t;
    return gamma_hip_group_set_transport(G, t == COPIES ? 0 : 1);
}

const Cfg kCfgs[] = {{"ivfpq", true, false, 1, false}, {"ivfpq-rows-sharded", true, true, 1, false}, {"ivfpq-rows-sharded-norank", true, true, 0, false},
                     {"ivfflat", false, false, 1, false},
                     // the scripted scan asks for the MAXIMUM over the members (what an inner-product scan does): clean runs only
                     {"ivfpq-inner-product", true, false, 1, true}};

int new_group(int members) {
    W = members;
    std::vector<int> devs(W);
    for (int i = 0; i < W; i++) devs[i] = i;
    if (gamma_hip_group_create(devs.data(), W, &G) != GAMMA_HIP_OK) return 2;
    g_member.assign(W, nullptr);
    for (int i = 0; i < W; i++) {
        g_member[i] = gamma_hip_group_member(G, i);
        if (gamma_hip_ivfpq_init(g_member[i], D, NLIST, 2, 8, 1, 100, 1000) != GAMMA_HIP_OK) return 2;
    }
    return gamma_hip_group_set_owners(G, nullptr) != GAMMA_HIP_OK ? 2 : 0;
}

// The shapes follow from W by rule (at W = 3: the batches of 7, 2, 900 and 700 this program has always run, and one query):
//   2W+1 queries: slices of 3, the last one short (W = 4: empty); W-1: one slice empty; 300 W: one owner flags its whole slice,
//   rounds of 256 + 44; 233 W + 1: slices of 234, the last one shorter, member 0 flags all of its own; 1 query: q0 < i * per for
//   the trailing members.  The first shape of a fresh group is one query with 96 probes: the in-place all-gather of the
//   assignment then moves W rows of 384 bytes into buffers that hold exactly W * per of them -- more than the slack a buffer is
//   allocated with, so that one sized by nq shows under AddressSanitizer.
int matrix(bool sweep) {
    Flags none(W), ties(W), empty_slice(W), two_rounds(W), full_slice(W), one(W);
    for (int m = 0; m < W; m++) {
        const int nql = std::min(2 * W + 1, (m + 1) * 3) - std::min(2 * W + 1, m * 3);
        if (m == 0) ties[m] = {0, 2};
        else if (nql >= 2) ties[m] = {1};
        else if (nql == 1) ties[m] = {0};
        if (m < W - 1) empty_slice[m] = {0};
    }
    two_rounds[0] = {5};
    two_rounds[1] = upto(300);
    if (W > 2) two_rounds[W - 1] = {299, 7};
    const int nq_full = 233 * W + 1, last = nq_full - (W - 1) * 234;
    full_slice[0] = upto(234);
    full_slice[W - 1] = {last - 1};
    one[0] = {0};
    for (const Cfg& cfg : kCfgs) {
        if (gamma_group_ext::set_raw_sharded(G, cfg.raw_sharded ? 1 : 0) != GAMMA_HIP_OK) {
            fprintf(stderr, "set_raw_sharded: %s\n", gamma_hip_group_last_error(G));
            return 2;
        }
        for (int device = 0; device < 2; device++) {
            clean(cfg, 1, device, one, "96 probes", 96);
            clean(cfg, 2 * W + 1, device, none, "no ties");
            clean(cfg, 2 * W + 1, device, ties, "ties at every owner");
            clean(cfg, W - 1, device, empty_slice, "an empty slice");
            clean(cfg, 300 * W, device, two_rounds, "rounds of 256 and 44 at one owner");
            clean(cfg, nq_full, device, full_slice, "a whole slice flagged");
            clean(cfg, 1, device, one, "one query");
        }
        // the failure sweep: W = 3, over peer copies every entry; over RCCL every entry the RCCL path reaches -- all but
        // bound_combine, which search() asserts is never called there (IVFFLAT members run over copies either way: swept there)
        if (!sweep || cfg.ip || (g_transport == RCCL && !cfg.pq)) continue;
        const bool rs = cfg.pq && cfg.raw_sharded && cfg.has_rank != 0;
        int nth = 0;
        for (int e = 0; e < N_ENTRIES; e++) {
            if (!cfg.pq && (e == SCAN_BEFORE_REDUCE || e == BOUND_COMBINE)) continue;
            if (!rs && (e == SHARD_EXACT || e == EXPORT_EXACT)) continue;
            if (g_transport == RCCL && e == BOUND_COMBINE) continue;
            // later calls of the entries a member reaches more than once: the owner's gathers of one round, the second tie round
            const int later = e == GATHER_ROWS ? (rs ? 3 : cfg.pq ? 2 : 1) : (e == EXPORT_ROWS || e == EXPORT || e == BOUND_COMBINE) ? 1 : 0;
            for (int skip = 0; skip <= later; skip++)
                for (int m = 0; m < W; m++) failing(cfg, e, m, skip, (nth++ & 1) != 0, ties);
        }
    }
    return 0;
}

void plain_case(const char* name, bool ok) {
    n_cases++;
    n_failures += !ok;
    printf("%-88s %s\n", name, ok ? "ok" : "FAILED");
}

}  // namespace

int main() {
    signal(SIGALRM, on_alarm);
    setvbuf(stdout, nullptr, _IOLBF, 0);
    gamma_group_ext::register_ivfflat_ops(&kFlatFamily);
    gamma_group_ext::register_raw_ops(&kRawOps);
    char name[160];
    for (int members = 2; members <= 4; members++) {
        const int64_t comms0 = fakerccl_comms_created(), inits0 = fakerccl_init_calls();
        if (new_group(members)) return 2;
        // ---- RCCL first: the group is fresh, its communicator forms at the first search ----
        if (set_transport(RCCL) != GAMMA_HIP_OK) return 2;
        Flags one(W);
        one[0] = {0};
        clean(kCfgs[0], 1, false, one, "the first search of the group", 96);
        // the stand-in must BE the library the group found: otherwise every RCCL case below would quietly run over copies
        if (std::string(gamma_hip_group_transport_note(G)) != "RCCL" || fakerccl_comms_created() != comms0 + W || counts_of(0).all_gather != 2) {
            fprintf(stderr, "group_protocol: the group did not form its communicator in the stand-in (transport note \"%s\", %lld communicators created)\n",
                    gamma_hip_group_transport_note(G), (long long)(fakerccl_comms_created() - comms0));
            return 2;
        }
        if (matrix(W == 3)) return 2;
        // ---- peer copies (a communicator exists, and must stay idle) ----
        if (set_transport(COPIES) != GAMMA_HIP_OK) return 2;
        if (matrix(W == 3)) return 2;
        // ---- and back: the communicator formed above is used again, no second one is created ----
        if (set_transport(RCCL) != GAMMA_HIP_OK) return 2;
        Flags ties(W);
        ties[0] = {0, 2};
        clean(kCfgs[4], 2 * W + 1, true, ties, "back on RCCL");
        snprintf(name, sizeof(name), "W=%d: one ncclCommInitAll, %d communicators, used again after copies", W, W);
        plain_case(name, fakerccl_comms_created() == comms0 + W && fakerccl_init_calls() == inits0 + 1 && std::string(gamma_hip_group_transport_note(G)).rfind("RCCL", 0) == 0);
        gamma_hip_group_destroy(G);
        snprintf(name, sizeof(name), "W=%d: the group destroys its communicators", W);
        plain_case(name, fakerccl_live_comm(0) == nullptr);
    }
    // ---- ncclCommInitAll fails: the group says so, searches over copies, and does not try again at every call ----
    {
        const int64_t comms0 = fakerccl_comms_created(), inits0 = fakerccl_init_calls();
        if (new_group(3)) return 2;
        fakerccl_fail_next_init(fakeNcclInternalError);
        if (set_transport(FALLBACK) != GAMMA_HIP_OK) return 2;
        Flags ties(W), one(W);
        ties[0] = {0, 2}, ties[1] = {1}, ties[2] = {0};
        one[0] = {0};
        for (const Cfg& cfg : kCfgs) {
            if (gamma_group_ext::set_raw_sharded(G, cfg.raw_sharded ? 1 : 0) != GAMMA_HIP_OK) return 2;
            for (int device = 0; device < 2; device++) {
                clean(cfg, 7, device, ties, "ties at every owner");
                clean(cfg, 1, device, one, "one query");
            }
        }
        int64_t t[2];
        gamma_hip_group_transport(G, t);
        const std::string note = gamma_hip_group_transport_note(G);
        plain_case("ncclCommInitAll refused: said in the note, tried once, every search over copies",
                   note.rfind("ncclCommInitAll failed", 0) == 0 && t[0] == 0 && t[1] == 0 && fakerccl_comms_created() == comms0 && fakerccl_init_calls() == inits0 + 1);
        gamma_hip_group_destroy(G);
    }
    std::string tally;
    for (int w = 2; w <= 4; w++)
        for (int t = 0; t < N_TRANSPORTS; t++)
            if (n_clean[w][t] + n_injected[w][t]) {
                snprintf(name, sizeof(name), "%sW=%d %s: %d clean + %d injected", tally.empty() ? "" : "; ", w, kTransportName[t], n_clean[w][t], n_injected[w][t]);
                tally += name;
            }
    printf("group_protocol: %d searches, %d cases (%s), %d stub-side checks failed, %d failures\n", n_calls, n_cases, tally.c_str(), g_bad.load(),
           n_failures + (g_bad.load() ? 1 : 0));
    return n_failures || g_bad.load() ? 1 : 0;
}
