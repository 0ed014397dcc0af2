// gamma_hip_group.cpp -- several GPUs behind ONE index object in one process: a group of handles, the index sharded by
// IVF list (include/gamma_hip.h, "several GPUs in ONE process").  The reference's GPU model does this with faiss's
// IndexShards (index/impl/gpu/gamma_gpu_cloner.cpp:200-269, index/impl/gpu/gamma_index_ivfpq_gpu.cc:356-436,
// faiss:IndexShards.cpp:283-345: a host thread per GPU, results merged on the host); here the split is by list (SURVEY
// 8e), the exchange is device-to-device and the merge runs on the GPU that owns the query.
//
// Built on the public C ABI of the members only (plus the HIP runtime for the peer copies and events): a member is an
// ordinary handle with a list mask.  One host thread per member enqueues that member's share of a call on the member's
// own stream; cross-device ordering is by events.  gamma_amd/dist.py is the same sequence of steps with one PROCESS per
// GPU and RCCL collectives.
//
// THE MEETING POINTS OF A LIST-SHARDED SEARCH.  The members' threads meet (Barrier::arrive) in this order, the same for IVFPQ and
// IVFFLAT members except where said, and EVERY member reaches EVERY one of them on EVERY path -- a member with an error arrives
// with "not ok", skips its own work and goes on to the next one; a member that left one out would leave its peers waiting:
//   1. after the coarse quantizer                      (every member's slice of the assignment is on its stream)
//   2. IVFPQ only: inside the scan's bound reduction   (every member's bounds are on its stream; a member that never got to
//                                                       its reduction arrives from scan_owned_lists instead)
//   3. after the scan                                  (every member's candidate tables are on its stream)
//   4. after the merge and gamma_hip_ivfpq_merge_flagged (every owner's list of flagged queries is known)
//   5. per tie round (at most 256 flagged queries of one owner), four times:
//        the owner's compact inputs are ready | every member's longest export row is known | every export is complete |
//        the exports may be overwritten
//   6. at the end                                      (nobody reads this member's tables any more)
// Whether a phase runs is decided from the snapshot the meeting point before it returns -- the same answer for all members --
// never from a member's own status: points 2 and 5 exist only where point 1 / point 4 answered "go" for everybody.  Replicated
// lists (gamma_hip_group_set_placement): every member answers its slice alone and the threads meet nowhere.  member_search()
// below is this sequence; each meeting point is one call site.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/gamma_hip.h"
#include "gamma_hip_group_ext.h"
#include "gamma_hip_group_rccl.h"

namespace {

struct GBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// all members' threads meet here; reusable
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, waiting = 0;
    uint64_t gen = 0;
    bool acc_ok = true, phase_ok[2] = {true, true};
    // Every member passes its own status; all of them get the SAME answer for the phase: whether every member was fine
    // when it arrived.  The go / no-go decisions of a multi-phase call are taken from this snapshot only -- a member that
    // fails after the barrier cannot make the others disagree about which barriers are still to come.
    bool arrive(bool my_ok = true) {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = gen;
        acc_ok = acc_ok && my_ok;
        if (++waiting == n) {
            waiting = 0;
            phase_ok[g & 1] = acc_ok;   // (a member can be at most one generation ahead of the slowest reader)
            acc_ok = true;
            gen++;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
        return phase_ok[g & 1];
    }
};

}  // namespace

// ---- optional transport: RCCL over xGMI (the north star's wording: an all-gather of the assignment, the per-shard
//      top-recall_num tables exchanged before the final merge).  Resolved at run time (dlopen: no link-time dependency on
//      the library, whose copy inside the process may be the one a host framework already loaded); one communicator per
//      member from ncclCommInitAll, every member's thread issues its own calls on its own stream.  Off by default
//      (GAMMA_HIP_GROUP_RCCL=1 or gamma_hip_group_set_transport): peer copies and the barriers below do the same job, and a
//      group whose members share a device (tests) cannot form a communicator. ----
namespace {
// (the entries' pointer types and the enumerators: gamma_hip_group_rccl.h, checked against the installed rccl.h by the tests)
using gamma_group_rccl::RcclApi;
using gamma_group_rccl::kNcclChar;
using gamma_group_rccl::kNcclFloat;
using gamma_group_rccl::kNcclMax;
using gamma_group_rccl::kNcclMin;
RcclApi* rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* l = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);   // a copy already in the process first
        if (!l) l = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!l) l = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!l) l = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!l) return;
        api.lib = l;
        api.CommInitAll = reinterpret_cast<int (*)(void**, int, const int*)>(dlsym(l, "ncclCommInitAll"));
        api.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(l, "ncclCommDestroy"));
        api.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(l, "ncclAllGather"));
        api.AllReduce = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(dlsym(l, "ncclAllReduce"));
        api.Send = reinterpret_cast<int (*)(const void*, size_t, int, int, void*, hipStream_t)>(dlsym(l, "ncclSend"));
        api.Recv = reinterpret_cast<int (*)(void*, size_t, int, int, void*, hipStream_t)>(dlsym(l, "ncclRecv"));
        api.GroupStart = reinterpret_cast<int (*)()>(dlsym(l, "ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<int (*)()>(dlsym(l, "ncclGroupEnd"));
        api.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(l, "ncclGetErrorString"));
    });
    return &api;
}
}  // namespace

struct gamma_hip_group {
    std::vector<gamma_hip_index*> m;
    std::vector<int> dev;
    std::vector<int> owner;   // list -> member; empty until gamma_hip_group_set_owners
    std::string err;
    std::mutex mu;            // one group-level call at a time
    int next_enc = 0;         // members take turns encoding Add / Update batches
    bool replicate = false;   // gamma_hip_group_set_placement: every member holds every list, queries are split
    // gamma_hip_group_set_raw_placement: every raw row exactly once, in the sparse store of the member that owns its list;
    // the exact distances of a has_rank search are computed there and travel with the candidates
    bool raw_sharded = false;
    // 0: peer copies; 1 (default since round 6; GAMMA_HIP_GROUP_RCCL=0 turns it off): RCCL wherever a communicator of the
    // members' DISTINCT devices can be formed -- members sharing a device, a missing librccl.so or a failing
    // ncclCommInitAll fall back to peer copies and say so (gamma_hip_group_transport)
    int transport = (getenv("GAMMA_HIP_GROUP_RCCL") && atoi(getenv("GAMMA_HIP_GROUP_RCCL")) == 0) ? 0 : 1;
    std::vector<void*> comm;  // one per member once formed
    bool comm_tried = false;
    std::string transport_note;
    int64_t rccl_calls = 0;   // searches whose exchanges went through RCCL

    struct Member {
        GBuf x, cdis, probe, rdis, rids, all_dis, all_ids, D, I;
        // exact ties across members: flagged queries' inputs (owner side / shard side), exports, the owner's copy of all exports
        GBuf fx, fcd, fpr, sx, scd, spr, ex_vals, ex_ids, ex_off, av, ai, ao, cutf, cutall;
        // two-phase shard search: the bounds this member's scan exports (what its peers read), its working copy, a peer's
        GBuf bound, bound_pub, bound_peer;
        // raw rows sharded with the lists: exact distances of this member's candidates, of the own slice's candidates from every
        // member; tie phase: the flagged queries' bounds (owner side / shard side), the export's exact distances, the owner's copy
        GBuf rex, all_ex, fbd, sbd, ex_ex, ae;
        hipEvent_t ev_coarse = nullptr, ev_scan = nullptr, ev_tie = nullptr, ev_bound = nullptr;
    };
    std::vector<Member> mb;

    // one persistent thread per member: run(job) executes job(i) on thread i and returns when all are done
    std::vector<std::thread> th;
    std::mutex pmu;
    std::condition_variable pcv, dcv;
    std::function<void(int)> job;
    uint64_t job_gen = 0;
    int job_left = 0;
    bool stop = false;
    Barrier bar;

    void worker(int i) {
        (void)hipSetDevice(dev[i]);
        uint64_t seen = 0;
        for (;;) {
            std::function<void(int)> f;
            {
                std::unique_lock<std::mutex> lk(pmu);
                pcv.wait(lk, [&] { return stop || job_gen != seen; });
                if (stop) return;
                seen = job_gen;
                f = job;
            }
            f(i);
            {
                std::lock_guard<std::mutex> lk(pmu);
                if (--job_left == 0) dcv.notify_all();
            }
        }
    }
    void run(const std::function<void(int)>& f) {
        std::unique_lock<std::mutex> lk(pmu);
        job = f;
        job_left = (int)m.size();
        job_gen++;
        pcv.notify_all();
        dcv.wait(lk, [&] { return job_left == 0; });
    }
};

namespace {

int gfail(gamma_hip_group* g, int code, const std::string& msg) {
    g->err = msg;
    return code;
}
int member_fail(gamma_hip_group* g, int i, int rc) {
    g->err = "member " + std::to_string(i) + ": " + gamma_hip_strerror(rc) + " (" + gamma_hip_last_error(g->m[i]) + ")";
    return rc;
}

// the sparse raw store's entries this file may not name (gamma_hip_group_ext.h); null in a build without them
const gamma_group_ext::RawOps*& raw_ops() {
    static const gamma_group_ext::RawOps* ops = nullptr;
    return ops;
}

// Narrow raw rows sharded with their lists: the members convert the caller's fp32 rows.  Every member's store has one element
// type and one set of sq8 ranges -- checked once, when the placement is switched on: neither can change while a store is
// sparse or holds rows -- so one member's acceptance predicate speaks for all.  It runs over ALL rows of a call before any
// member is touched: a row a store would refuse fails the call with nothing changed on any member.
int members_same_rows(gamma_hip_group* g, const char* what) {
    const gamma_group_ext::RawOps* rops = raw_ops();
    // (a table without the two entries -- one that registered the fp32 sparse store's only -- has nothing to compare or refuse)
    for (size_t i = 1; rops && rops->same_rows && i < g->m.size(); i++)
        if (!rops->same_rows(g->m[0], g->m[i]))
            return gfail(g, GAMMA_HIP_EINVAL, std::string(what) + ": the members' raw stores differ in element type, row length or sq8 ranges");
    return GAMMA_HIP_OK;
}
int rows_storable(gamma_hip_group* g, int64_t n, const float* vecs) {
    const gamma_group_ext::RawOps* rops = raw_ops();
    if (!g->raw_sharded || g->replicate || !rops || !rops->rows_check || g->m.empty()) return GAMMA_HIP_OK;
    const int rk = rops->rows_check(g->m[0], n, vecs);
    return rk ? member_fail(g, 0, rk) : GAMMA_HIP_OK;
}

gamma_group_ext::MemberMarkFn& member_mark() {
    static gamma_group_ext::MemberMarkFn fn = nullptr;
    return fn;
}

// the IVFFLAT family: entries this file may not name either (gamma_hip_group_ext.h); null in a build without them
const gamma_group_ext::ShardFamily*& ivfflat_family() {
    static const gamma_group_ext::ShardFamily* f = nullptr;
    return f;
}

// src on device sd -> dst on device dd, ordered on stream s (a stream of device dd)
hipError_t copy_between(void* dst, int dd, const void* src, int sd, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (dd == sd) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
    return hipMemcpyPeerAsync(dst, dd, src, sd, bytes, s);
}

}  // namespace

namespace gamma_group_ext {

int register_raw_ops(const RawOps* ops) {
    raw_ops() = ops;
    return 1;
}

int register_member_mark(MemberMarkFn fn) {
    member_mark() = fn;
    return 1;
}

int register_ivfflat_ops(const ShardFamily* family) {
    ivfflat_family() = family;
    return 1;
}

int set_raw_sharded(gamma_hip_group* g, int sharded) {
    if (!g || (sharded != 0 && sharded != 1)) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->raw_sharded == (sharded != 0)) return GAMMA_HIP_OK;
    const RawOps* rops = raw_ops();
    if (!rops) return gfail(g, GAMMA_HIP_EUNSUPPORTED, "set_raw_placement: sharded raw rows are not built in");
    if (sharded && g->replicate) return gfail(g, GAMMA_HIP_EINVAL, "set_raw_placement: sharded raw rows cannot go with replicated lists");
    for (size_t i = 0; i < g->m.size(); i++)
        if (rops->raw_count(g->m[i]) != 0) return gfail(g, GAMMA_HIP_EINVAL, "set_raw_placement: before any raw row is written");
    if (sharded) {
        const int same = members_same_rows(g, "set_raw_placement");
        if (same) return same;
        // every member's (empty) store takes the sparse form now: a member that owns no vector yet answers all the same
        for (size_t i = 0; i < g->m.size(); i++) {
            const int rc = gamma_hip_raw_put(g->m[i], 0, nullptr, nullptr);
            if (rc) return member_fail(g, (int)i, rc);
        }
    } else {
        // back to rows by vector id: the (empty) sparse stores become untyped again
        for (size_t i = 0; i < g->m.size(); i++) {
            const int rc = rops->raw_clear(g->m[i]);
            if (rc) return member_fail(g, (int)i, rc);
        }
    }
    g->raw_sharded = sharded != 0;
    return GAMMA_HIP_OK;
}

int raw_sharded(const gamma_hip_group* g) { return g && g->raw_sharded ? 1 : 0; }

int raw_put(gamma_hip_group* g, int64_t n, const int64_t* vids, const float* vecs, int64_t* n_skipped) {
    if (n_skipped) *n_skipped = 0;
    if (!g || n < 0 || n > INT32_MAX || (n > 0 && (!vids || !vecs))) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->raw_sharded) return gfail(g, GAMMA_HIP_EINVAL, "raw_put: gamma_hip_group_set_raw_placement(g, 1) first");
    if (n == 0) return GAMMA_HIP_OK;
    const int W = (int)g->m.size();
    const int d = gamma_hip_ivfpq_dim(g->m[0]);
    if (d <= 0) return gfail(g, GAMMA_HIP_EINVAL, "raw_put: members not initialised");
    {
        const int rk = rows_storable(g, n, vecs);
        if (rk) return rk;
    }
    std::vector<int> where(n, -1);
    std::vector<uint8_t> has(n);
    for (int i = 0; i < W; i++) {
        const int rc = gamma_hip_ivfpq_has_vid(g->m[i], vids, (int)n, has.data());
        if (rc) return member_fail(g, i, rc);
        for (int64_t j = 0; j < n; j++)
            if (has[j]) where[j] = i;
    }
    int64_t skipped = 0;
    for (int i = 0; i < W; i++) {
        std::vector<int64_t> v;
        std::vector<float> x;
        for (int64_t j = 0; j < n; j++) {
            if (where[j] != i) continue;
            v.push_back(vids[j]);
            x.insert(x.end(), vecs + (size_t)j * d, vecs + (size_t)(j + 1) * d);
        }
        if (v.empty()) continue;
        const int rc = gamma_hip_raw_put(g->m[i], (int64_t)v.size(), v.data(), x.data());
        if (rc) return member_fail(g, i, rc);
    }
    for (int64_t j = 0; j < n; j++) skipped += where[j] < 0;
    if (n_skipped) *n_skipped = skipped;
    return GAMMA_HIP_OK;
}

}  // namespace gamma_group_ext

extern "C" {

int gamma_hip_group_create(const int* devices, int n, gamma_hip_group** out) {
    if (!out || !devices || n <= 0 || n > 64) return GAMMA_HIP_EINVAL;
    *out = nullptr;
    gamma_hip_group* g = new (std::nothrow) gamma_hip_group();
    if (!g) return GAMMA_HIP_ENOMEM;
    g->dev.assign(devices, devices + n);
    g->mb.resize(n);
    for (int i = 0; i < n; i++) {
        gamma_hip_index* h = nullptr;
        const int rc = gamma_hip_create(devices[i], &h);
        if (rc != GAMMA_HIP_OK) {
            for (auto* mh : g->m) gamma_hip_destroy(mh);
            delete g;
            return rc;
        }
        g->m.push_back(h);
        if (member_mark()) (void)member_mark()(h);
    }
    // direct copies between the members' devices where the fabric allows it (xGMI); failure is not an error, the
    // runtime then stages peer copies itself
    for (int i = 0; i < n; i++) {
        (void)hipSetDevice(devices[i]);
        for (int j = 0; j < n; j++) {
            if (devices[j] == devices[i]) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(devices[j], 0);
                if (e != hipSuccess) (void)hipGetLastError();   // already enabled, or refused: both fine
            }
        }
        if (hipEventCreateWithFlags(&g->mb[i].ev_coarse, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g->mb[i].ev_tie, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g->mb[i].ev_bound, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g->mb[i].ev_scan, hipEventDisableTiming) != hipSuccess) {
            for (auto* mh : g->m) gamma_hip_destroy(mh);
            delete g;
            return GAMMA_HIP_EDEVICE;
        }
    }
    g->bar.n = n;
    for (int i = 0; i < n; i++) g->th.emplace_back([g, i] { g->worker(i); });
    *out = g;
    return GAMMA_HIP_OK;
}

int gamma_hip_group_destroy(gamma_hip_group* g) {
    if (!g) return GAMMA_HIP_OK;
    {
        std::lock_guard<std::mutex> lk(g->pmu);
        g->stop = true;
        g->pcv.notify_all();
    }
    for (auto& t : g->th)
        if (t.joinable()) t.join();
    for (size_t i = 0; i < g->m.size(); i++) {
        (void)hipSetDevice(g->dev[i]);
        (void)gamma_hip_synchronize(g->m[i]);
        gamma_hip_group::Member& b = g->mb[i];
        for (GBuf* p : {&b.x, &b.cdis, &b.probe, &b.rdis, &b.rids, &b.all_dis, &b.all_ids, &b.D, &b.I, &b.fx, &b.fcd, &b.fpr, &b.sx,
                        &b.scd, &b.spr, &b.ex_vals, &b.ex_ids, &b.ex_off, &b.av, &b.ai, &b.ao, &b.cutf, &b.cutall, &b.bound, &b.bound_pub, &b.bound_peer, &b.rex, &b.all_ex, &b.fbd, &b.sbd,
                        &b.ex_ex, &b.ae})
            p->release();
        if (b.ev_tie) (void)hipEventDestroy(b.ev_tie);
        if (b.ev_bound) (void)hipEventDestroy(b.ev_bound);
        if (b.ev_coarse) (void)hipEventDestroy(b.ev_coarse);
        if (b.ev_scan) (void)hipEventDestroy(b.ev_scan);
    }
    if (!g->comm.empty() && rccl_api()->CommDestroy)
        for (void* c : g->comm)
            if (c) (void)rccl_api()->CommDestroy(c);
    for (auto* h : g->m) gamma_hip_destroy(h);
    delete g;
    return GAMMA_HIP_OK;
}

int gamma_hip_group_set_transport(gamma_hip_group* g, int rccl) {
    if (!g || (rccl != 0 && rccl != 1)) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    g->transport = rccl;
    if (rccl == 1 && g->comm.empty()) g->comm_tried = false;   // (formed at the next sharded search)
    return GAMMA_HIP_OK;
}

int gamma_hip_group_transport(gamma_hip_group* g, int64_t* out2) {
    if (!g || !out2) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    out2[0] = (g->transport == 1 && !g->comm.empty()) ? 1 : 0;
    out2[1] = g->rccl_calls;
    return GAMMA_HIP_OK;
}

const char* gamma_hip_group_transport_note(gamma_hip_group* g) { return g ? g->transport_note.c_str() : ""; }

int gamma_hip_group_size(const gamma_hip_group* g) { return g ? (int)g->m.size() : 0; }
gamma_hip_index* gamma_hip_group_member(gamma_hip_group* g, int i) {
    return (g && i >= 0 && i < (int)g->m.size()) ? g->m[i] : nullptr;
}
const char* gamma_hip_group_last_error(gamma_hip_group* g) { return g ? g->err.c_str() : "null group"; }

int gamma_hip_group_set_owners(gamma_hip_group* g, const int64_t* weights) {
    if (!g) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    const int W = (int)g->m.size();
    const int nlist = gamma_hip_ivfpq_nlist(g->m[0]);
    if (nlist <= 0) return gfail(g, GAMMA_HIP_EINVAL, "set_owners: members not initialised");
    for (int i = 1; i < W; i++)
        if (gamma_hip_ivfpq_nlist(g->m[i]) != nlist) return gfail(g, GAMMA_HIP_EINVAL, "set_owners: members differ in nlist");
    g->owner.assign(nlist, 0);
    if (g->replicate) {
        // every member holds every list (member 0 answers the per-list getters); no mask
        for (int i = 0; i < W; i++) {
            const int rc = gamma_hip_ivfpq_set_list_mask(g->m[i], nullptr);
            if (rc) return member_fail(g, i, rc);
        }
        return GAMMA_HIP_OK;
    }
    if (!weights) {
        for (int l = 0; l < nlist; l++) g->owner[l] = l % W;
    } else {
        // greedy longest-processing-time on the weights (gamma_amd/dist.py balance_lists): heaviest list first onto the
        // lightest member; the +1 spreads empty lists as well
        std::vector<int> order(nlist);
        for (int l = 0; l < nlist; l++) order[l] = l;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weights[a] > weights[b]; });
        std::vector<int64_t> load(W, 0);
        for (int l : order) {
            int best = 0;
            for (int i = 1; i < W; i++)
                if (load[i] < load[best]) best = i;
            g->owner[l] = best;
            load[best] += std::max<int64_t>(0, weights[l]) + 1;
        }
    }
    std::vector<uint8_t> mask(nlist);
    for (int i = 0; i < W; i++) {
        for (int l = 0; l < nlist; l++) mask[l] = g->owner[l] == i ? 1 : 0;
        const int rc = gamma_hip_ivfpq_set_list_mask(g->m[i], mask.data());
        if (rc) return member_fail(g, i, rc);
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_group_set_placement(gamma_hip_group* g, int replicate) {
    if (!g) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->owner.empty() && g->replicate != (replicate != 0))
        return gfail(g, GAMMA_HIP_EINVAL, "set_placement: before gamma_hip_group_set_owners");
    if (replicate && g->raw_sharded) return gfail(g, GAMMA_HIP_EINVAL, "set_placement: replicated lists cannot go with sharded raw rows");
    g->replicate = replicate != 0;
    return GAMMA_HIP_OK;
}
int gamma_hip_group_placement(const gamma_hip_group* g) { return g && g->replicate ? 1 : 0; }

int gamma_hip_group_owner(const gamma_hip_group* g, int l) {
    return (g && l >= 0 && l < (int)g->owner.size()) ? g->owner[l] : -1;
}

int gamma_hip_group_ivfpq_add(gamma_hip_group* g, int64_t n, const float* vecs, int64_t first_vid) {
    if (!g || n < 0 || (n > 0 && !vecs)) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->owner.empty()) return gfail(g, GAMMA_HIP_EINVAL, "add: gamma_hip_group_set_owners first");
    const int W = (int)g->m.size(), nlist = (int)g->owner.size();
    // one encode for the batch (quantizer->assign + residual + pq.compute_codes, gamma_index_ivfpq.cc:424-512)
    const int e = g->next_enc++ % W;
    const int cs = gamma_hip_ivfpq_code_size(g->m[e]);
    if (cs <= 0) return gfail(g, GAMMA_HIP_EINVAL, "add: members not initialised");
    const int d = gamma_hip_ivfpq_dim(g->m[e]);
    const bool rows = g->raw_sharded && !g->replicate;   // every vector's row goes to the owner of its list, with its keys
    {
        const int rk = rows_storable(g, n, vecs);
        if (rk) return rk;
    }
    std::vector<float> gvecs;
    std::vector<int64_t> lno(n);
    std::vector<uint8_t> codes((size_t)n * cs);
    int rc = gamma_hip_ivfpq_encode(g->m[e], n, vecs, lno.data(), codes.data());
    if (rc) return member_fail(g, e, rc);
    // AddKeys at the owner, lists in ascending order, entries in batch order (the std::map of gamma_index_ivfpq.cc:428-494)
    std::vector<int64_t> order(n);
    for (int64_t i = 0; i < n; i++) {
        if (lno[i] < 0 || lno[i] >= nlist) lno[i] = (first_vid + i) % nlist;
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return lno[a] < lno[b]; });
    for (int o = 0; o < W; o++) {
        std::vector<int32_t> lists, counts;
        std::vector<int64_t> vids;
        std::vector<uint8_t> gcodes;
        gvecs.clear();
        for (int64_t i = 0; i < n; i++) {
            const int64_t src = order[i];
            if (!g->replicate && g->owner[lno[src]] != o) continue;
            if (rows) gvecs.insert(gvecs.end(), vecs + (size_t)src * d, vecs + (size_t)(src + 1) * d);
            if (lists.empty() || lists.back() != (int32_t)lno[src]) {
                lists.push_back((int32_t)lno[src]);
                counts.push_back(0);
            }
            counts.back()++;
            vids.push_back(first_vid + src);
            gcodes.insert(gcodes.end(), codes.begin() + (size_t)src * cs, codes.begin() + (size_t)(src + 1) * cs);
        }
        if (lists.empty()) continue;
        if (g->replicate) {   // the same grouped batch to every member
            for (int i = 0; i < W; i++) {
                rc = gamma_hip_ivfpq_add_keys_batch(g->m[i], (int)lists.size(), lists.data(), counts.data(), vids.data(), gcodes.data());
                if (rc) return member_fail(g, i, rc);
            }
            break;
        }
        if (rows) {   // the rows first: a vector is listed only once its row is in place
            rc = gamma_hip_raw_put(g->m[o], (int64_t)vids.size(), vids.data(), gvecs.data());
            if (rc) return member_fail(g, o, rc);
        }
        rc = gamma_hip_ivfpq_add_keys_batch(g->m[o], (int)lists.size(), lists.data(), counts.data(), vids.data(), gcodes.data());
        if (rc) return member_fail(g, o, rc);
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_group_ivfpq_add_keys(gamma_hip_group* g, int l, int n, const int64_t* vids, const uint8_t* codes) {
    if (!g) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (l < 0 || l >= (int)g->owner.size()) return gfail(g, GAMMA_HIP_EINVAL, "add_keys: bad list (or no owners yet)");
    const int o = g->owner[l];
    if (g->replicate) {
        for (size_t i = 0; i < g->m.size(); i++) {
            const int rc = gamma_hip_ivfpq_add_keys(g->m[i], l, n, vids, codes);
            if (rc) return member_fail(g, (int)i, rc);
        }
        return GAMMA_HIP_OK;
    }
    const int rc = gamma_hip_ivfpq_add_keys(g->m[o], l, n, vids, codes);
    return rc ? member_fail(g, o, rc) : GAMMA_HIP_OK;
}

int64_t gamma_hip_group_ivfpq_list_size(gamma_hip_group* g, int l) {
    if (!g) return -1;
    std::lock_guard<std::mutex> lk(g->mu);
    if (l < 0 || l >= (int)g->owner.size()) return -1;
    return gamma_hip_ivfpq_list_size(g->m[g->owner[l]], l);
}

int gamma_hip_group_ivfpq_get_list(gamma_hip_group* g, int l, int64_t* vids, uint8_t* codes) {
    if (!g) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (l < 0 || l >= (int)g->owner.size()) return gfail(g, GAMMA_HIP_EINVAL, "get_list: bad list (or no owners yet)");
    const int o = g->owner[l];
    const int rc = gamma_hip_ivfpq_get_list(g->m[o], l, vids, codes);
    return rc ? member_fail(g, o, rc) : GAMMA_HIP_OK;
}

int gamma_hip_group_ivfpq_update(gamma_hip_group* g, int n, const int64_t* vids, const float* vecs) {
    if (!g || n < 0 || (n > 0 && (!vids || !vecs))) return GAMMA_HIP_EINVAL;
    if (n == 0) return GAMMA_HIP_OK;
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->owner.empty()) return gfail(g, GAMMA_HIP_EINVAL, "update: gamma_hip_group_set_owners first");
    const int W = (int)g->m.size(), nlist = (int)g->owner.size();
    const int e = g->next_enc++ % W;
    const int cs = gamma_hip_ivfpq_code_size(g->m[e]);
    if (cs <= 0) return gfail(g, GAMMA_HIP_EINVAL, "update: bad code size");
    {
        const int rk = rows_storable(g, n, vecs);
        if (rk) return rk;
    }
    std::vector<int64_t> lno(n);
    std::vector<uint8_t> codes((size_t)n * cs);
    int rc = gamma_hip_ivfpq_encode_each(g->m[e], n, vecs, lno.data(), codes.data());
    if (rc) return member_fail(g, e, rc);
    if (g->replicate) {   // one encode, the same in-place Update at every member (a member ignores vids it never held)
        std::vector<int32_t> l32(n);
        for (int j = 0; j < n; j++) l32[j] = (int32_t)lno[j];
        for (int i = 0; i < W; i++) {
            rc = gamma_hip_ivfpq_apply_updates(g->m[i], n, l32.data(), vids, codes.data(), nullptr);
            if (rc) return member_fail(g, i, rc);
        }
        return GAMMA_HIP_OK;
    }
    // who holds each vid now (at most one member); kept current while the batch is routed, so that a vid named
    // twice is followed through its first move
    std::unordered_map<int64_t, int> holder;
    {
        std::vector<uint8_t> has(n);
        for (int i = 0; i < W; i++) {
            rc = gamma_hip_ivfpq_has_vid(g->m[i], vids, n, has.data());
            if (rc) return member_fail(g, i, rc);
            for (int j = 0; j < n; j++)
                if (has[j]) holder[vids[j]] = i;
        }
    }
    // RealTimeMemData::Update (realtime_mem_data.cc:305-327) when the list a vector leaves and the list it joins may
    // belong to different members: per member the entries that concern it, in batch order
    std::vector<std::vector<int>> idx(W);
    std::vector<std::vector<uint8_t>> ops(W);
    // sharded raw rows: where a vector's row was before the batch and the last entry of the batch that names it
    struct RowMove { int from, last; };
    std::unordered_map<int64_t, RowMove> moves;
    for (int j = 0; j < n; j++) {
        auto it = holder.find(vids[j]);
        if (it == holder.end()) continue;   // never added: Update ignores it (:307-311)
        if (g->raw_sharded) {
            auto mv = moves.find(vids[j]);
            if (mv == moves.end()) moves.emplace(vids[j], RowMove{it->second, j});
            else mv->second.last = j;
        }
        if (lno[j] < 0 || lno[j] >= nlist) continue;
        const int from = it->second, to = g->owner[lno[j]];
        if (from == to) {
            idx[to].push_back(j);
            ops[to].push_back(0);
        } else {
            idx[from].push_back(j);
            ops[from].push_back(2);   // leaves: flag the old entry
            idx[to].push_back(j);
            ops[to].push_back(1);     // the owner of the new list appends
            it->second = to;
        }
    }
    if (g->raw_sharded) {
        // The rows follow their vectors: the last vector a batch gives a vid is put at the member that lists it after the
        // batch (in place when it stayed, a new row when it moved), then the member that listed it before forgets its row.
        // Puts before drops, rows before lists: at no point is a listed vector without a row.
        const gamma_group_ext::RawOps* rops = raw_ops();
        if (!rops) return gfail(g, GAMMA_HIP_EUNSUPPORTED, "update: sharded raw rows are not built in");
        const int d = gamma_hip_ivfpq_dim(g->m[e]);
        std::vector<std::vector<int64_t>> pv(W), dv(W);
        std::vector<std::vector<float>> px(W);
        for (int j = 0; j < n; j++) {   // (batch order: the same sequence of puts on every run)
            auto mv = moves.find(vids[j]);
            if (mv == moves.end() || mv->second.last != j) continue;
            const int to = holder[vids[j]];
            pv[to].push_back(vids[j]);
            px[to].insert(px[to].end(), vecs + (size_t)j * d, vecs + (size_t)(j + 1) * d);
            if (mv->second.from != to) dv[mv->second.from].push_back(vids[j]);
        }
        for (int i = 0; i < W; i++) {
            if (pv[i].empty()) continue;
            rc = gamma_hip_raw_put(g->m[i], (int64_t)pv[i].size(), pv[i].data(), px[i].data());
            if (rc) return member_fail(g, i, rc);
        }
        for (int i = 0; i < W; i++) {
            if (dv[i].empty()) continue;
            rc = rops->raw_drop(g->m[i], (int64_t)dv[i].size(), dv[i].data());
            if (rc) return member_fail(g, i, rc);
        }
    }
    for (int i = 0; i < W; i++) {
        const int ni = (int)idx[i].size();
        if (ni == 0) continue;
        std::vector<int32_t> l32(ni);
        std::vector<int64_t> v(ni);
        std::vector<uint8_t> c((size_t)ni * cs);
        for (int t = 0; t < ni; t++) {
            const int j = idx[i][t];
            l32[t] = (int32_t)lno[j];
            v[t] = vids[j];
            memcpy(c.data() + (size_t)t * cs, codes.data() + (size_t)j * cs, cs);
        }
        rc = gamma_hip_ivfpq_apply_updates(g->m[i], ni, l32.data(), v.data(), c.data(), ops[i].data());
        if (rc) return member_fail(g, i, rc);
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_group_ivfpq_delete(gamma_hip_group* g, const int64_t* vids, int n) {
    if (!g || (n > 0 && !vids)) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    for (size_t i = 0; i < g->m.size(); i++) {   // a member counts the vids it holds and ignores the others
        const int rc = gamma_hip_ivfpq_delete(g->m[i], vids, n);
        if (rc) return member_fail(g, (int)i, rc);
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_group_ivfpq_compact_if_need(gamma_hip_group* g) {
    if (!g) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    for (size_t i = 0; i < g->m.size(); i++) {
        const int rc = gamma_hip_ivfpq_compact_if_need(g->m[i]);
        if (rc) return member_fail(g, (int)i, rc);
    }
    return GAMMA_HIP_OK;
}

int64_t gamma_hip_group_total_mem_bytes(gamma_hip_group* g) {
    if (!g) return 0;
    int64_t t = 0;
    for (auto* h : g->m) t += gamma_hip_total_mem_bytes(h);
    return t;
}

}  // extern "C"

// ---- search: ONE protocol for IVFPQ and IVFFLAT members (the sequence of meeting points: file header) ------------------------
// IVFPQ: gamma_index_ivfpq.cc search_preassigned + compute_dis per member; IVFFLAT: gamma_index_ivfflat.cc search_preassigned;
// faiss:IndexShards.cpp:283-345 for the merge.  What differs between the families is in their ShardFamily table
// (gamma_hip_group_ext.h); the sharded raw rows' entries (IVFPQ only) are called by name under Call::rs.
namespace {

using gamma_group_ext::ShardFamily;
typedef gamma_hip_group::Member Member;

const ShardFamily kIvfpqFamily = {
    "search", gamma_hip_ivfpq_search_device, gamma_hip_ivfpq_coarse_device, gamma_hip_ivfpq_search_shard_bounded,
    gamma_hip_ivfpq_shard_export_rows, gamma_hip_ivfpq_shard_export, gamma_hip_ivfpq_merge_rerank, gamma_hip_ivfpq_merge_replay,
    /*wide_tables*/ true, /*bounded_scan*/ true, /*tie_coarse_dis*/ true, /*raw_rows*/ true, /*rccl*/ true,
};

// one call, shared by the members' threads
struct Call {
    gamma_hip_group* g;
    const ShardFamily* f;
    gamma_hip_search_params pp;
    int nq, k, d, P, R, W, per;   // R: width of the candidate tables; per: rows of a slice
    // on_device: x / distances / labels live on member 0's device (the other members pull the batch over the fabric and push
    // their slice of the results back); the call still returns when the results are in place
    const float* x;
    float* distances;
    int64_t* labels;
    bool on_device;
    // raw rows sharded with the lists: the exact distances of compute_dis are computed where the rows are and travel with the
    // candidates (has_rank = 0: nothing is computed, nothing more is sent)
    bool rs;
    RcclApi* nccl;   // the exchanges go through RCCL; null: peer copies
    std::vector<int> rcs;
    std::vector<std::string> errs;
    std::vector<int64_t> rowmax;          // tie phase: every member's longest export row of the round
    std::vector<int> nfl;                 // flagged queries of every member's slice
    std::vector<const int32_t*> lists;    // and the device lists of their slice-local indices
    void slice(int i, int* q0, int* q1) const {
        *q0 = std::min(nq, i * per);
        *q1 = std::min(nq, *q0 + per);
    }
};

// one member's share of it: what its thread carries from phase to phase.  The first failure is kept (rc, the text in errs[i]);
// later steps still run or are skipped on ok(), but WHICH meeting points follow is never decided from it (Barrier::arrive).
struct Ctx {
    Call& c;
    const int i, dev;
    int q0, nql;
    Member& b;
    gamma_hip_index* const h;
    const hipStream_t s;
    int& rc;
    std::string& err;
    Ctx(Call& call, int member)
        : c(call), i(member), dev(call.g->dev[member]), b(call.g->mb[member]), h(call.g->m[member]),
          s((hipStream_t)gamma_hip_stream(call.g->m[member])), rc(call.rcs[member]), err(call.errs[member]) {
        int q1;
        c.slice(i, &q0, &q1);
        nql = q1 - q0;
    }
    bool ok() const { return rc == GAMMA_HIP_OK; }
    void hip(hipError_t e, const char* what) {
        if (e != hipSuccess && ok()) {
            rc = e == hipErrorOutOfMemory ? GAMMA_HIP_ENOMEM : GAMMA_HIP_EDEVICE;
            err = std::string(what) + ": " + hipGetErrorString(e);
        }
    }
    void abi(int r) {
        if (r != GAMMA_HIP_OK && ok()) {
            rc = r;
            err = std::string(gamma_hip_strerror(r)) + " (" + gamma_hip_last_error(h) + ")";
        }
    }
    void ncc(int e, const char* what) {
        if (e != 0 && ok()) {
            rc = GAMMA_HIP_EDEVICE;
            err = std::string(what) + ": " + (c.nccl && c.nccl->GetErrorString ? c.nccl->GetErrorString(e) : "RCCL error");
        }
    }
    void alloc(GBuf& buf, size_t bytes) { hip(buf.ensure(bytes), "alloc"); }
};

// One column of an exchange: rows of `width` elements of `elem` bytes travel from a member's `src` into this member's `dst`.
struct Col {
    GBuf Member::*src;
    GBuf Member::*dst;
    size_t elem, width;
    bool on;
    const char* what;
    size_t row() const { return elem * width; }
};
// rows [src_row, src_row + rows) of member j's column -> rows [dst_row, ...) of this member's, ordered on this member's stream
void pull(Ctx& m, const Col& col, int j, size_t dst_row, size_t src_row, size_t rows) {
    if (!col.on) return;
    gamma_hip_group* g = m.c.g;
    m.hip(copy_between((m.b.*col.dst).as<char>() + dst_row * col.row(), m.dev, (g->mb[j].*col.src).as<char>() + src_row * col.row(), g->dev[j],
                       rows * col.row(), m.s), col.what);
}

void upload(Ctx& m, const float* src, int rows) {
    const size_t bytes = (size_t)rows * m.c.d * sizeof(float);
    if (m.c.on_device) m.hip(copy_between(m.b.x.p, m.dev, src, m.c.g->dev[0], bytes, m.s), "queries to the member");
    else m.hip(hipMemcpyAsync(m.b.x.p, src, bytes, hipMemcpyHostToDevice, m.s), "H2D queries");
}

// the slice's rows (D, I) to the caller
void results_to_caller(Ctx& m) {
    Call& c = m.c;
    float* Ds = c.distances + (size_t)m.q0 * c.k;
    int64_t* Is = c.labels + (size_t)m.q0 * c.k;
    const size_t n = (size_t)m.nql * c.k;
    if (c.on_device) {
        m.hip(copy_between(Ds, c.g->dev[0], m.b.D.p, m.dev, n * sizeof(float), m.s), "results");
        m.hip(copy_between(Is, c.g->dev[0], m.b.I.p, m.dev, n * sizeof(int64_t), m.s), "results");
    } else {
        m.hip(hipMemcpyAsync(Ds, m.b.D.p, n * sizeof(float), hipMemcpyDeviceToHost, m.s), "D2H");
        m.hip(hipMemcpyAsync(Is, m.b.I.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, m.s), "D2H");
    }
}

// query-parallel over replicated lists: the member answers its slice with the ordinary single-handle search (exact ties and
// all); nothing is exchanged but the slice and its k results, and the members meet nowhere
void replicate_slice(Ctx& m) {
    Call& c = m.c;
    if (m.nql <= 0 || !m.ok()) return;
    const bool local = c.on_device && m.dev == c.g->dev[0];
    const float* xs = c.x + (size_t)m.q0 * c.d;
    if (!local) {
        m.alloc(m.b.x, (size_t)m.nql * c.d * sizeof(float));
        m.alloc(m.b.D, (size_t)m.nql * c.k * sizeof(float));
        m.alloc(m.b.I, (size_t)m.nql * c.k * sizeof(int64_t));
        if (!m.ok()) return;
        upload(m, xs, m.nql);
    }
    if (m.ok())
        m.abi(c.f->search_device(m.h, &c.pp, m.nql, local ? xs : m.b.x.as<float>(), c.k, local ? c.distances + (size_t)m.q0 * c.k : m.b.D.as<float>(),
                                 local ? c.labels + (size_t)m.q0 * c.k : m.b.I.as<int64_t>()));
    if (m.ok() && !local) results_to_caller(m);
    m.hip(hipStreamSynchronize(m.s), "sync");
}

// 0. the whole batch to every member (each scans its lists for all queries); coarse quantizer for the own slice
void upload_and_coarse(Ctx& m) {
    Call& c = m.c;
    Member& b = m.b;
    m.alloc(b.x, (size_t)c.nq * c.d * sizeof(float));
    // (W * per rows: the in-place all-gather moves whole slices, the last one's tail rows are never read)
    m.alloc(b.cdis, (size_t)c.W * c.per * c.P * sizeof(float));
    m.alloc(b.probe, (size_t)c.W * c.per * c.P * sizeof(int32_t));
    m.alloc(b.rdis, (size_t)c.nq * c.R * sizeof(float));
    m.alloc(b.rids, (size_t)c.nq * c.R * sizeof(int64_t));
    m.alloc(b.all_dis, (size_t)c.W * c.per * c.R * sizeof(float));
    m.alloc(b.all_ids, (size_t)c.W * c.per * c.R * sizeof(int64_t));
    m.alloc(b.D, (size_t)c.per * c.k * sizeof(float));
    m.alloc(b.I, (size_t)c.per * c.k * sizeof(int64_t));
    if (!m.ok()) return;
    upload(m, c.x, c.nq);
    if (m.nql > 0)
        m.abi(c.f->coarse_device(m.h, &c.pp, m.nql, b.x.as<float>() + (size_t)m.q0 * c.d, b.cdis.as<float>() + (size_t)m.q0 * c.P,
                                 b.probe.as<int32_t>() + (size_t)m.q0 * c.P));
    m.hip(hipEventRecord(b.ev_coarse, m.s), "record");
}

// 1a. the other slices of the assignment
void exchange_assignment(Ctx& m) {
    Call& c = m.c;
    const Col cols[] = {{&Member::cdis, &Member::cdis, sizeof(float), (size_t)c.P, true, "assignment exchange"},
                        {&Member::probe, &Member::probe, sizeof(int32_t), (size_t)c.P, true, "assignment exchange"}};
    if (c.nccl) {
        // RCCL: ONE all-gather of the assignment over xGMI (in place: this member's slice sits at its offset already)
        m.ncc(c.nccl->GroupStart(), "ncclGroupStart");
        for (const Col& col : cols)
            m.ncc(c.nccl->AllGather((m.b.*col.dst).as<char>() + (size_t)m.i * c.per * col.row(), (m.b.*col.dst).p, (size_t)c.per * col.row(),
                                    kNcclChar, c.g->comm[m.i], m.s), "ncclAllGather");
        m.ncc(c.nccl->GroupEnd(), "ncclGroupEnd");
        return;
    }
    for (int j = 0; j < c.W; j++) {
        if (j == m.i) continue;
        int a0, a1;
        c.slice(j, &a0, &a1);
        if (a1 <= a0) continue;
        m.hip(hipStreamWaitEvent(m.s, c.g->mb[j].ev_coarse, 0), "wait");
        for (const Col& col : cols) pull(m, col, j, a0, a0, a1 - a0);
    }
}

// The IVFPQ scan runs in TWO PHASES around a reduction of one float per query (gamma_hip_ivfpq_search_shard_bounded): every
// member bounds its own recall_num-th best from the query's nearest probes it owns, the minimum (L2) / maximum (IP) over the
// members bounds the GLOBAL one, and the members' other probes only keep what is within it.  The reduction: ncclAllReduce over
// xGMI, or -- peer copies -- every member publishes its bounds, the members meet, pull each other's and combine.  It is one more
// meeting point of the call: a member that does not get as far as its scan arrives there all the same (scan_owned_lists).
struct BoundMeeting {
    Ctx* m;
    bool arrived;
    bool arrive(bool my_ok) {
        arrived = true;
        return m->c.g->bar.arrive(my_ok);   // every member's bounds are on its stream (RCCL: all enter the collective, or none)
    }
};
int reduce_bounds(void* user, float* d_bound, int n, int take_max, void* stream) {
    BoundMeeting& at = *static_cast<BoundMeeting*>(user);
    Ctx& m = *at.m;
    Call& c = m.c;
    gamma_hip_group* g = c.g;
    Member& b = m.b;
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool ok = true;   // (the scan is entered by a member without an error only)
    if (!c.nccl)
        ok = b.bound_pub.ensure((size_t)n * sizeof(float)) == hipSuccess && b.bound_peer.ensure((size_t)n * sizeof(float)) == hipSuccess &&
             hipMemcpyAsync(b.bound_pub.p, d_bound, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess &&
             hipEventRecord(b.ev_bound, s) == hipSuccess;
    if (!at.arrive(ok)) return ok ? 0 : 1;   // (the bounds stay this member's own: still valid)
    if (c.nccl) {
        const int e = c.nccl->AllReduce(d_bound, d_bound, (size_t)n, kNcclFloat, take_max ? kNcclMax : kNcclMin, g->comm[m.i], s);
        if (e != 0) m.err = std::string("ncclAllReduce: ") + (c.nccl->GetErrorString ? c.nccl->GetErrorString(e) : "RCCL error");
        return e != 0;
    }
    for (int j = 0; j < c.W && ok; j++) {
        if (j == m.i) continue;
        ok = hipStreamWaitEvent(s, g->mb[j].ev_bound, 0) == hipSuccess &&
             copy_between(b.bound_peer.p, m.dev, g->mb[j].bound_pub.p, g->dev[j], (size_t)n * sizeof(float), s) == hipSuccess &&
             gamma_hip_bound_combine(stream, d_bound, b.bound_peer.as<float>(), n, take_max) == GAMMA_HIP_OK;
    }
    if (!ok) m.err = "bound reduction: peer copy failed";
    return ok ? 0 : 1;
}

// 1b. scan of the owned probed lists, local top-R of every query of the batch
void scan_owned_lists(Ctx& m) {
    Call& c = m.c;
    Member& b = m.b;
    BoundMeeting at{&m, false};
    if (c.f->bounded_scan) m.alloc(b.bound, (size_t)c.nq * sizeof(float));
    if (m.ok())
        m.abi(c.f->scan(m.h, &c.pp, c.nq, b.x.as<float>(), b.cdis.as<float>(), b.probe.as<int32_t>(), c.k, b.rdis.as<float>(),
                        b.rids.as<int64_t>(), c.f->bounded_scan ? b.bound.as<float>() : nullptr, c.f->bounded_scan ? reduce_bounds : nullptr, &at));
    if (c.f->bounded_scan && !at.arrived) (void)at.arrive(false);   // (this member never got to the reduction: its peers are waiting there)
    // did this member's own top-R cut of a query go through a tie?  (the merge at the query's owner asks)
    m.alloc(b.cutf, (size_t)c.nq);
    if (m.ok()) m.abi(gamma_hip_ivfpq_shard_cut_flags(m.h, c.nq, b.cutf.as<uint8_t>()));
    // (what the exchange below receives into is allocated on THIS side of the meeting point: a member that cannot get it says so
    //  in the go / no-go snapshot instead of leaving its peers inside a collective.  An RCCL error AFTER the meeting point is fatal
    //  for the group: nothing can call a member back out of ncclGroupEnd)
    m.alloc(b.cutall, (size_t)c.W * c.per);
    if (c.rs) {   // exact distances of the candidates this member is about to send, where it holds the row
        m.alloc(b.rex, (size_t)c.nq * c.R * sizeof(float));
        m.alloc(b.all_ex, (size_t)c.W * c.per * c.R * sizeof(float));
        if (m.ok()) m.abi(gamma_hip_ivfpq_shard_exact(m.h, &c.pp, c.nq, b.x.as<float>(), b.rids.as<int64_t>(), c.R, b.rex.as<float>()));
    }
    m.hip(hipEventRecord(b.ev_scan, m.s), "record");
}

// 2. the exchange of the path: the candidates of the own query slice from every member ([W][per][R]), their cut flags, and
//    their exact distances when the rows are sharded
void exchange_candidates(Ctx& m) {
    Call& c = m.c;
    const Col cols[] = {{&Member::rdis, &Member::all_dis, sizeof(float), (size_t)c.R, true, "candidate exchange"},
                        {&Member::rids, &Member::all_ids, sizeof(int64_t), (size_t)c.R, true, "candidate exchange"},
                        {&Member::cutf, &Member::cutall, 1, 1, true, "cut flags"},
                        {&Member::rex, &Member::all_ex, sizeof(float), (size_t)c.R, c.rs, "candidate exchange"}};
    if (c.nccl) {
        // RCCL: the per-shard tables of every owner's slice in one grouped exchange (every member sends slice j of its tables to
        // member j and receives its own slice of theirs -- an all-to-all over xGMI); members with an empty slice still take part
        m.ncc(c.nccl->GroupStart(), "ncclGroupStart");
        for (int j = 0; j < c.W; j++) {   // (never cut short: the other members' halves of the exchange are under way)
            int a0, a1;
            c.slice(j, &a0, &a1);
            for (const Col& col : cols)
                if (col.on && a1 > a0)
                    m.ncc(c.nccl->Send((m.b.*col.src).as<char>() + (size_t)a0 * col.row(), (size_t)(a1 - a0) * col.row(), kNcclChar, j,
                                       c.g->comm[m.i], m.s), "ncclSend");
            for (const Col& col : cols)
                if (col.on && m.nql > 0)
                    m.ncc(c.nccl->Recv((m.b.*col.dst).as<char>() + (size_t)j * c.per * col.row(), (size_t)m.nql * col.row(), kNcclChar, j,
                                       c.g->comm[m.i], m.s), "ncclRecv");
        }
        m.ncc(c.nccl->GroupEnd(), "ncclGroupEnd");
        return;
    }
    for (int j = 0; j < c.W && m.nql > 0; j++) {
        if (j != m.i) m.hip(hipStreamWaitEvent(m.s, c.g->mb[j].ev_scan, 0), "wait");
        for (const Col& col : cols) pull(m, col, j, (size_t)j * c.per, m.q0, m.nql);
    }
}

// 3. merge of the own slice to the global top-R, compute_dis (IVFPQ) / to the top-k (IVFFLAT)
void merge_slice(Ctx& m) {
    Call& c = m.c;
    Member& b = m.b;
    const float* xs = b.x.as<float>() + (size_t)m.q0 * c.d;
    if (m.ok()) m.abi(gamma_hip_ivfpq_merge_set_shard_flags(m.h, b.cutall.as<uint8_t>()));
    if (m.ok() && c.rs)
        m.abi(gamma_hip_ivfpq_merge_rerank_exact(m.h, &c.pp, c.W, c.per, xs, c.k, b.all_dis.as<float>(), b.all_ids.as<int64_t>(),
                                                 b.all_ex.as<float>(), 0, m.nql, b.D.as<float>(), b.I.as<int64_t>()));
    else if (m.ok())
        m.abi(c.f->merge(m.h, &c.pp, c.W, c.per, xs, c.k, b.all_dis.as<float>(), b.all_ids.as<int64_t>(), 0, m.nql, b.D.as<float>(),
                         b.I.as<int64_t>()));
}

// 4. exact ties across members (include/gamma_hip.h): the queries a tie can change, listed by their owner, get their candidate
//    streams exported by every member and replayed at the owner.  One round: nf flagged queries of owner o, from f0 of its list.
void tie_round(Ctx& m, int o, int f0, int nf) {
    Call& c = m.c;
    Member& b = m.b;
    Barrier& bar = c.g->bar;
    const int32_t* list = c.lists[o] + f0;
    // the flagged queries' vectors and assignment rows, compact (sharded rows: and their reduced bounds of the scan -- only exported
    // entries within them can be members of the recall_num-heap, only those get an exact distance)
    const Col in[] = {{&Member::fx, &Member::sx, sizeof(float), (size_t)c.d, true, "tie inputs"},
                      {&Member::fcd, &Member::scd, sizeof(float), (size_t)c.P, c.f->tie_coarse_dis, "tie inputs"},
                      {&Member::fpr, &Member::spr, sizeof(int32_t), (size_t)c.P, true, "tie inputs"},
                      {&Member::fbd, &Member::sbd, sizeof(float), 1, c.rs, "tie inputs"}};
    if (m.i == o) {
        for (const Col& col : in)
            if (col.on) m.alloc(b.*col.src, (size_t)nf * col.row());
        if (m.ok() && c.rs) m.abi(gamma_hip_gather_rows(m.h, b.bound.as<float>() + m.q0, 1, list, nf, b.fbd.p));
        if (m.ok()) {
            m.abi(gamma_hip_gather_rows(m.h, b.x.as<float>() + (size_t)m.q0 * c.d, c.d, list, nf, b.fx.p));
            if (c.f->tie_coarse_dis) m.abi(gamma_hip_gather_rows(m.h, b.cdis.as<float>() + (size_t)m.q0 * c.P, c.P, list, nf, b.fcd.p));
            m.abi(gamma_hip_gather_rows(m.h, b.probe.as<int32_t>() + (size_t)m.q0 * c.P, c.P, list, nf, b.fpr.p));
        }
        m.hip(hipEventRecord(b.ev_tie, m.s), "record");
    }
    bool go = bar.arrive(m.ok());   // the owner's compact inputs are on its stream
    for (const Col& col : in)
        if (col.on) m.alloc(b.*col.dst, (size_t)nf * col.row());
    m.alloc(b.ex_off, (size_t)nf * (c.P + 1) * sizeof(int32_t));
    c.rowmax[m.i] = 0;
    if (go && m.ok()) {
        if (m.i != o) m.hip(hipStreamWaitEvent(m.s, c.g->mb[o].ev_tie, 0), "wait");
        for (const Col& col : in) pull(m, col, o, 0, 0, nf);
        // how long this member's export rows get: the exports of all members share one row stride
        int64_t mine = 0;
        if (m.ok()) m.abi(c.f->shard_export_rows(m.h, &c.pp, nf, b.spr.as<int32_t>(), &mine));
        c.rowmax[m.i] = mine;
    }
    go = bar.arrive(m.ok());   // every member's longest row is known
    int64_t stride = 4;
    for (int j = 0; j < c.W; j++) stride = std::max<int64_t>(stride, (c.rowmax[j] + 3) & ~(int64_t)3);
    m.alloc(b.ex_vals, (size_t)nf * stride * sizeof(float));
    m.alloc(b.ex_ids, (size_t)nf * stride * sizeof(int64_t));
    if (go && m.ok())
        m.abi(c.f->shard_export(m.h, &c.pp, nf, b.sx.as<float>(), c.f->tie_coarse_dis ? b.scd.as<float>() : nullptr, b.spr.as<int32_t>(), stride,
                                b.ex_vals.as<float>(), b.ex_ids.as<int64_t>(), b.ex_off.as<int32_t>()));
    if (c.rs) m.alloc(b.ex_ex, (size_t)nf * stride * sizeof(float));
    if (c.rs && go && m.ok())
        m.abi(gamma_hip_ivfpq_shard_export_exact(m.h, &c.pp, nf, b.sx.as<float>(), b.ex_vals.as<float>(), b.ex_ids.as<int64_t>(),
                                                 b.ex_off.as<int32_t>(), stride, b.sbd.as<float>(), b.ex_ex.as<float>()));
    m.hip(hipStreamSynchronize(m.s), "sync");
    go = bar.arrive(m.ok());   // every member's export is complete
    if (m.i == o && go) {
        const Col out[] = {{&Member::ex_ex, &Member::ae, sizeof(float), (size_t)stride, c.rs, "exports"},
                           {&Member::ex_vals, &Member::av, sizeof(float), (size_t)stride, true, "exports"},
                           {&Member::ex_ids, &Member::ai, sizeof(int64_t), (size_t)stride, true, "exports"},
                           {&Member::ex_off, &Member::ao, sizeof(int32_t), (size_t)c.P + 1, true, "exports"}};
        for (const Col& col : out)
            if (col.on) m.alloc(b.*col.dst, (size_t)c.W * nf * col.row());
        for (int j = 0; j < c.W && m.ok(); j++)
            for (const Col& col : out) pull(m, col, j, (size_t)j * nf, 0, nf);
        const float* xs = b.x.as<float>() + (size_t)m.q0 * c.d;
        if (m.ok() && c.rs)
            m.abi(gamma_hip_ivfpq_merge_replay_exact(m.h, &c.pp, c.W, nf, xs, stride, b.av.as<float>(), b.ai.as<int64_t>(), b.ao.as<int32_t>(),
                                                     b.ae.as<float>(), c.k, list, b.D.as<float>(), b.I.as<int64_t>()));
        else if (m.ok())
            m.abi(c.f->merge_replay(m.h, &c.pp, c.W, nf, xs, stride, b.av.as<float>(), b.ai.as<int64_t>(), b.ao.as<int32_t>(), c.k, list,
                                    b.D.as<float>(), b.I.as<int64_t>()));
        m.hip(hipStreamSynchronize(m.s), "sync");
    }
    (void)bar.arrive(m.ok());   // the exports may be overwritten
}

// One member's thread through a call: the phases, and between them the meeting points every member reaches on every path.
// `go` is the snapshot of the last meeting point -- the same answer for all members; a member's own rc only gates its own work.
void member_search(Ctx& m) {
    Call& c = m.c;
    Barrier& bar = c.g->bar;
    m.hip(hipSetDevice(m.dev), "hipSetDevice");
    if (c.g->replicate) return replicate_slice(m);
    upload_and_coarse(m);
    bool go = bar.arrive(m.ok());   // every member's assignment is on its stream
    if (go) {
        exchange_assignment(m);
        scan_owned_lists(m);        // (IVFPQ: the meeting point of the bound reduction is in here)
    }
    go = bar.arrive(m.ok());        // every member's candidate tables are on its stream
    if (go) exchange_candidates(m);
    if (go && m.nql > 0) merge_slice(m);
    static const bool gdbg = getenv("GAMMA_HIP_GROUP_DBG") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    auto since = [&](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    int nf_i = 0;
    const int32_t* list_i = nullptr;
    if (go && m.nql > 0 && m.ok()) m.abi(gamma_hip_ivfpq_merge_flagged(m.h, &nf_i, &list_i));
    c.nfl[m.i] = m.ok() ? nf_i : 0;
    c.lists[m.i] = list_i;
    if (gdbg && m.i == 0) fprintf(stderr, "group: member 0 waited %.3f ms for its merge, %d flagged\n", since(tp0), nf_i);
    go = bar.arrive(m.ok());        // every owner's flagged queries are listed
    const int fcap = 256;           // flagged queries per round
    for (int o = 0; o < c.W && go; o++)
        for (int f0 = 0; f0 < c.nfl[o]; f0 += fcap) tie_round(m, o, f0, std::min(fcap, c.nfl[o] - f0));
    if (gdbg && m.i == 0) fprintf(stderr, "group: tie phase done %.3f ms after the merge was enqueued\n", since(tp0));
    // (go: the snapshot of the last meeting point outside the rounds -- the tie phase's own failures show in rc)
    if (go && m.nql > 0 && m.ok()) results_to_caller(m);
    m.hip(hipStreamSynchronize(m.s), "sync");
    (void)bar.arrive(m.ok());       // nobody is reading this member's tables any more
}

// transport of the exchanges: RCCL when asked for and a communicator of the members' distinct devices can be formed (tried once)
void form_communicator(gamma_hip_group* g) {
    const int W = (int)g->m.size();
    g->comm_tried = true;
    bool distinct = true;
    for (int i = 0; i < W; i++)
        for (int j = 0; j < i; j++) distinct = distinct && g->dev[i] != g->dev[j];
    RcclApi* api = rccl_api();
    if (!distinct) {
        g->transport_note = "RCCL asked for, but members share a device: peer copies";
    } else if (!api->ok()) {
        g->transport_note = "RCCL asked for, but librccl.so could not be loaded: peer copies";
    } else {
        g->comm.assign(W, nullptr);
        const int e = api->CommInitAll(g->comm.data(), W, g->dev.data());
        if (e != 0) {
            g->comm.clear();
            g->transport_note = std::string("ncclCommInitAll failed (") + (api->GetErrorString ? api->GetErrorString(e) : "?") + "): peer copies";
        } else {
            g->transport_note = "RCCL";
        }
    }
}

int group_search(gamma_hip_group* g, const ShardFamily* f, const gamma_hip_search_params* p, int nq, const float* x, int k, float* distances,
                 int64_t* labels, bool on_device) {
    if (!g || !p) return GAMMA_HIP_EINVAL;
    if (nq < 0) return GAMMA_HIP_EINVAL;
    if (k <= 0 || nq == 0) return GAMMA_HIP_OK;   // gamma_index_ivfpq.cc:753-756
    if (!x || !distances || !labels) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if (!f) return gfail(g, GAMMA_HIP_EUNSUPPORTED, "ivfflat_search: the IVFFLAT search of the group is not built in");
    const std::string name = f->name;
    if (g->owner.empty()) return gfail(g, GAMMA_HIP_EINVAL, name + ": gamma_hip_group_set_owners first");
    const int W = (int)g->m.size();
    const int d = gamma_hip_ivfpq_dim(g->m[0]);
    if (d <= 0) return gfail(g, GAMMA_HIP_EINVAL, name + ": members not initialised");
    if (p->nprobe <= 0) return gfail(g, GAMMA_HIP_EINVAL, name + ": nprobe out of range");
    Call c;
    c.g = g;
    c.f = f;
    // faiss chooses the coarse path from the size of the WHOLE call (faiss:utils/distances.cpp:346): the slices must agree
    c.pp = *p;
    if (c.pp.coarse_mode < 0) c.pp.coarse_mode = nq < 20 ? 0 : 1;
    // (gamma_hip_blas_form_not_restated: every member counts the shape of ITS slice -- a remainder block of the whole call
    //  that a slice boundary hides is not counted here)
    c.nq = nq, c.k = k, c.d = d, c.P = p->nprobe, c.W = W;
    c.R = f->wide_tables ? std::max(p->recall_num, k) : k;
    c.per = (nq + W - 1) / W;
    c.x = x, c.distances = distances, c.labels = labels, c.on_device = on_device;
    if (f->rccl && g->transport == 1 && !g->replicate && !g->comm_tried) form_communicator(g);
    if (!f->rccl && g->transport == 1 && !g->replicate && g->transport_note.find("IVFFLAT") == std::string::npos)
        g->transport_note += std::string(g->transport_note.empty() ? "" : "; ") + "IVFFLAT search: peer copies (RCCL serves the IVFPQ search only)";
    c.rs = f->raw_rows && g->raw_sharded && !g->replicate && c.pp.has_rank != 0;
    const bool use_rccl = f->rccl && g->transport == 1 && !g->replicate && (int)g->comm.size() == W;
    if (use_rccl) g->rccl_calls++;
    c.nccl = use_rccl ? rccl_api() : nullptr;
    c.rcs.assign(W, GAMMA_HIP_OK);
    c.errs.resize(W);
    c.rowmax.assign(W, 0);
    c.nfl.assign(W, 0);
    c.lists.assign(W, nullptr);
    g->run([&](int i) {
        Ctx m(c, i);
        member_search(m);
    });
    for (int i = 0; i < W; i++)
        if (c.rcs[i] != GAMMA_HIP_OK) return gfail(g, c.rcs[i], "member " + std::to_string(i) + ": " + c.errs[i]);
    return GAMMA_HIP_OK;
}

}  // namespace

extern "C" {

int gamma_hip_group_ivfpq_search(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* x, int k,
                                 float* distances, int64_t* labels) {
    return group_search(g, &kIvfpqFamily, p, nq, x, k, distances, labels, false);
}

int gamma_hip_group_ivfpq_search_device(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* d_x, int k,
                                        float* d_distances, int64_t* d_labels) {
    return group_search(g, &kIvfpqFamily, p, nq, d_x, k, d_distances, d_labels, true);
}

int gamma_hip_group_ivfflat_search(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* x, int k,
                                   float* distances, int64_t* labels) {
    return group_search(g, ivfflat_family(), p, nq, x, k, distances, labels, false);
}

int gamma_hip_group_ivfflat_search_device(gamma_hip_group* g, const gamma_hip_search_params* p, int nq, const float* d_x, int k,
                                          float* d_distances, int64_t* d_labels) {
    return group_search(g, ivfflat_family(), p, nq, d_x, k, d_distances, d_labels, true);
}

}  // extern "C"
