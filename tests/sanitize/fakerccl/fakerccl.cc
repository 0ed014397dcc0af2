// TEST INFRASTRUCTURE (fakerccl.h): the stand-in communicator.  What it holds its callers to, as NCCL documents it:
//   * a collective is a rendezvous: a rank blocks until ALL ranks of the communicator have called one, and kind, count, datatype
//     and reduction must agree across the ranks.  All checks of a collective are made at the rendezvous, so that EVERY rank
//     returns the error (a rank turned away at the door would leave its peers waiting);
//   * ncclAllGather fills nranks x sendcount at every rank; a send buffer inside the receive buffer must sit at
//     recvbuff + rank x sendcount (the in-place rule);
//   * ncclAllReduce: ncclFloat32 with ncclMin / ncclMax, the rest is refused;
//   * ncclSend / ncclRecv take effect at ncclGroupEnd: all sends of the group are posted first, every recv then takes the next
//     unconsumed send of its peer in posting order, the byte counts must be equal (both sides get the error), and the caller
//     returns when its sends have been consumed.  Sending to oneself is allowed.  A send or recv without a partner blocks;
//   * collectives inside a group are deferred to ncclGroupEnd too, and run in posting order before the group's sends and recvs;
//   * ncclCommInitAll refuses duplicate devices.
// Mutexes and condition variables only: ThreadSanitizer sees every ordering.  All copies are made under the communicator's
// mutex by a thread inside the call, into the buffers the callers named: AddressSanitizer sees every overrun.
#include "fakerccl.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../../gamma_amd/csrc/gamma_hip_group_rccl.h"

namespace {

enum Kind { ALL_GATHER = 1, ALL_REDUCE = 2, SEND = 3, RECV = 4 };
const char* const kKindName[] = {"?", "ncclAllGather", "ncclAllReduce", "ncclSend", "ncclRecv"};

struct Op {
    int kind = 0;
    const void* send = nullptr;
    void* recv = nullptr;
    size_t count = 0;
    int dtype = 0, op = 0, peer = 0;
    struct Comm* comm = nullptr;
};
struct Posted {   // a send waiting for its recv (owned by the sender, which stays inside ncclGroupEnd until it is consumed)
    const void* p;
    size_t bytes;
    bool consumed;
    int err;
};
struct World {   // what the ranks of one ncclCommInitAll share
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, alive = 0;
    std::vector<Op> slot;   // the collective under way: one per rank
    int arrived = 0;
    uint64_t gen = 0;
    int result[2] = {0, 0};
    std::vector<std::deque<Posted*>> box;   // [src * n + dst]
};
struct Comm {
    World* w;
    int rank;
    fakerccl_counts n;   // (under w->mu)
};

std::mutex g_mu;   // the registry and the switches below
std::vector<Comm*> g_live;
int64_t g_created = 0, g_inits = 0, g_messages = 0;
int g_fail_next_init = 0;

thread_local int tl_depth = 0;
thread_local std::vector<Op> tl_ops;

#define SAY(...)                                 \
    do {                                         \
        {                                        \
            std::lock_guard<std::mutex> lk_(g_mu); \
            g_messages++;                        \
        }                                        \
        fprintf(stderr, "FAKE RCCL: " __VA_ARGS__); \
        fputc('\n', stderr);                     \
    } while (0)

size_t type_size(int t) {
    static const size_t kSize[fakeNcclNumTypes] = {1, 1, 4, 4, 8, 8, 2, 4, 8, 2};
    return t >= 0 && t < fakeNcclNumTypes ? kSize[t] : 0;
}

// the last rank to arrive runs the collective for everybody (w.mu held; the other ranks wait inside their calls)
int run_collective(World& w) {
    const Op& a = w.slot[0];
    for (int r = 1; r < w.n; r++) {
        const Op& b = w.slot[r];
        if (b.kind != a.kind || b.count != a.count || b.dtype != a.dtype || b.op != a.op) {
            SAY("the ranks disagree in a collective: rank 0 called %s(count %zu, datatype %d, op %d), rank %d %s(count %zu, datatype %d, op %d)",
                kKindName[a.kind], a.count, a.dtype, a.op, r, kKindName[b.kind], b.count, b.dtype, b.op);
            return fakeNcclInvalidArgument;
        }
    }
    const size_t es = type_size(a.dtype);
    if (!es) {
        SAY("%s: unknown datatype %d", kKindName[a.kind], a.dtype);
        return fakeNcclInvalidArgument;
    }
    const size_t bytes = a.count * es;
    for (int r = 0; r < w.n; r++)
        if (bytes && (!w.slot[r].send || !w.slot[r].recv)) {
            SAY("%s: null buffer at rank %d", kKindName[a.kind], r);
            return fakeNcclInvalidArgument;
        }
    if (a.kind == ALL_GATHER) {
        for (int r = 0; r < w.n; r++) {   // in place: only at the rank's own offset
            const char *s = (const char*)w.slot[r].send, *d = (const char*)w.slot[r].recv;
            const bool overlaps = bytes && s < d + (size_t)w.n * bytes && s + bytes > d;
            if (overlaps && s != d + (size_t)r * bytes) {
                SAY("ncclAllGather: rank %d's send buffer lies inside its receive buffer at byte %td, not at rank x sendcount = %zu", r, s - d,
                    (size_t)r * bytes);
                return fakeNcclInvalidArgument;
            }
        }
        std::vector<char> all((size_t)w.n * bytes);
        for (int r = 0; r < w.n; r++)
            if (bytes) memcpy(all.data() + (size_t)r * bytes, w.slot[r].send, bytes);
        for (int r = 0; r < w.n; r++)
            if (bytes) memcpy(w.slot[r].recv, all.data(), all.size());
        return fakeNcclSuccess;
    }
    // ALL_REDUCE
    if (a.dtype != fakeNcclFloat32 || (a.op != fakeNcclMin && a.op != fakeNcclMax)) {
        SAY("ncclAllReduce: the stand-in reduces ncclFloat32 with ncclMin / ncclMax only (datatype %d, op %d)", a.dtype, a.op);
        return fakeNcclInvalidArgument;
    }
    std::vector<float> acc(a.count);
    if (bytes) memcpy(acc.data(), w.slot[0].send, bytes);
    for (int r = 1; r < w.n; r++) {
        const float* in = (const float*)w.slot[r].send;
        for (size_t t = 0; t < a.count; t++) acc[t] = a.op == fakeNcclMax ? std::max(acc[t], in[t]) : std::min(acc[t], in[t]);
    }
    for (int r = 0; r < w.n; r++)
        if (bytes) memcpy(w.slot[r].recv, acc.data(), bytes);
    return fakeNcclSuccess;
}

int collective(const Op& op) {
    World& w = *op.comm->w;
    std::unique_lock<std::mutex> lk(w.mu);
    const uint64_t g = w.gen;
    w.slot[op.comm->rank] = op;
    if (++w.arrived == w.n) {
        w.arrived = 0;
        w.result[g & 1] = run_collective(w);   // (a rank can be at most one generation ahead of the slowest reader)
        w.gen++;
        w.cv.notify_all();
    } else {
        w.cv.wait(lk, [&] { return w.gen != g; });
    }
    return w.result[g & 1];
}

// the sends and recvs of one group, all on communicators of one World
int exchange(const std::vector<Op>& ops) {
    if (ops.empty()) return fakeNcclSuccess;
    World& w = *ops[0].comm->w;
    int err = fakeNcclSuccess;
    std::deque<Posted> mine;   // (stable addresses)
    std::unique_lock<std::mutex> lk(w.mu);
    for (const Op& o : ops)
        if (o.kind == SEND) {
            mine.push_back({o.send, o.count * type_size(o.dtype), false, 0});
            w.box[(size_t)o.comm->rank * w.n + o.peer].push_back(&mine.back());
        }
    w.cv.notify_all();
    for (const Op& o : ops) {
        if (o.kind != RECV) continue;
        std::deque<Posted*>& q = w.box[(size_t)o.peer * w.n + o.comm->rank];
        w.cv.wait(lk, [&] { return !q.empty(); });
        Posted* s = q.front();
        q.pop_front();
        const size_t bytes = o.count * type_size(o.dtype);
        if (s->bytes != bytes) {
            lk.unlock();
            SAY("rank %d receives %zu bytes from rank %d, whose matching send has %zu", o.comm->rank, bytes, o.peer, s->bytes);
            lk.lock();
            err = s->err = fakeNcclInvalidArgument;
        } else if (bytes) {
            memcpy(o.recv, s->p, bytes);
        }
        s->consumed = true;
        w.cv.notify_all();
    }
    w.cv.wait(lk, [&] {
        for (const Posted& s : mine)
            if (!s.consumed) return false;
        return true;
    });
    for (const Posted& s : mine)
        if (s.err) err = s.err;
    return err;
}

int run_group(std::vector<Op>& ops) {
    int err = fakeNcclSuccess;
    std::vector<Op> p2p;
    for (const Op& o : ops) {
        if (o.comm->w != ops[0].comm->w) {
            SAY("one group over communicators of different ncclCommInitAll calls: not supported by the stand-in");
            return fakeNcclInvalidUsage;
        }
        if (o.kind == ALL_GATHER || o.kind == ALL_REDUCE) {
            const int e = collective(o);
            if (e && !err) err = e;
        } else {
            p2p.push_back(o);
        }
    }
    const int e = exchange(p2p);
    return err ? err : e;
}

int post(Op op, int64_t fakerccl_counts::*counter) {
    if (!op.comm) {
        SAY("%s: null communicator", kKindName[op.kind]);
        return fakeNcclInvalidArgument;
    }
    World& w = *op.comm->w;
    {
        std::lock_guard<std::mutex> lk(w.mu);
        op.comm->n.*counter += 1;
    }
    if (op.kind == SEND || op.kind == RECV) {
        if (op.peer < 0 || op.peer >= w.n || !type_size(op.dtype) || (op.count && !(op.kind == SEND ? op.send : op.recv))) {
            SAY("%s at rank %d: bad peer %d, datatype %d or null buffer", kKindName[op.kind], op.comm->rank, op.peer, op.dtype);
            return fakeNcclInvalidArgument;
        }
    }
    if (tl_depth > 0) {
        tl_ops.push_back(op);
        return fakeNcclSuccess;
    }
    std::vector<Op> one(1, op);
    return run_group(one);
}

}  // namespace

extern "C" {

int ncclCommInitAll(void** comm, int ndev, const int* devlist) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_inits++;
        if (g_fail_next_init) {   // (told to, by the test: no message)
            const int e = g_fail_next_init;
            g_fail_next_init = 0;
            return e;
        }
    }
    if (!comm || ndev <= 0) {
        SAY("ncclCommInitAll: bad arguments");
        return fakeNcclInvalidArgument;
    }
    for (int i = 0; devlist && i < ndev; i++)
        for (int j = 0; j < i; j++)
            if (devlist[i] == devlist[j]) {
                SAY("ncclCommInitAll: device %d named twice (ranks %d and %d)", devlist[i], j, i);
                return fakeNcclInvalidUsage;
            }
    World* w = new World();
    w->n = w->alive = ndev;
    w->slot.resize(ndev);
    w->box.resize((size_t)ndev * ndev);
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < ndev; i++) {
        Comm* c = new Comm{w, i, {0, 0, 0, 0, 0}};
        comm[i] = c;
        g_live.push_back(c);
        g_created++;
    }
    return fakeNcclSuccess;
}

int ncclCommDestroy(void* comm) {
    Comm* c = static_cast<Comm*>(comm);
    if (!c) return fakeNcclInvalidArgument;
    World* w = c->w;
    bool last;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), c), g_live.end());
    }
    {
        std::lock_guard<std::mutex> lk(w->mu);
        last = --w->alive == 0;
    }
    delete c;
    if (last) delete w;
    return fakeNcclSuccess;
}

int ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, int datatype, void* comm, hipStream_t) {
    Op op;
    op.kind = ALL_GATHER, op.send = sendbuff, op.recv = recvbuff, op.count = sendcount, op.dtype = datatype, op.comm = static_cast<Comm*>(comm);
    return post(op, &fakerccl_counts::all_gather);
}

int ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, int datatype, int rop, void* comm, hipStream_t) {
    Op op;
    op.kind = ALL_REDUCE, op.send = sendbuff, op.recv = recvbuff, op.count = count, op.dtype = datatype, op.op = rop, op.comm = static_cast<Comm*>(comm);
    return post(op, &fakerccl_counts::all_reduce);
}

int ncclSend(const void* sendbuff, size_t count, int datatype, int peer, void* comm, hipStream_t) {
    Op op;
    op.kind = SEND, op.send = sendbuff, op.count = count, op.dtype = datatype, op.peer = peer, op.comm = static_cast<Comm*>(comm);
    return post(op, &fakerccl_counts::send);
}

int ncclRecv(void* recvbuff, size_t count, int datatype, int peer, void* comm, hipStream_t) {
    Op op;
    op.kind = RECV, op.recv = recvbuff, op.count = count, op.dtype = datatype, op.peer = peer, op.comm = static_cast<Comm*>(comm);
    return post(op, &fakerccl_counts::recv);
}

int ncclGroupStart() {
    tl_depth++;
    return fakeNcclSuccess;
}

int ncclGroupEnd() {
    if (tl_depth <= 0) {
        SAY("ncclGroupEnd without ncclGroupStart");
        return fakeNcclInvalidUsage;
    }
    if (--tl_depth > 0) return fakeNcclSuccess;
    std::vector<Op> ops;
    ops.swap(tl_ops);
    if (ops.empty()) return fakeNcclSuccess;
    {
        std::lock_guard<std::mutex> lk(ops[0].comm->w->mu);
        ops[0].comm->n.group_end++;
    }
    return run_group(ops);
}

const char* ncclGetErrorString(int result) {
    switch (result) {
        case fakeNcclSuccess: return "no error";
        case fakeNcclInternalError: return "internal error (stand-in)";
        case fakeNcclInvalidArgument: return "invalid argument (stand-in)";
        case fakeNcclInvalidUsage: return "invalid usage (stand-in)";
        default: return "error (stand-in)";
    }
}

int fakerccl_get_counts(void* comm, fakerccl_counts* out) {
    Comm* c = static_cast<Comm*>(comm);
    if (!c || !out) return 1;
    std::lock_guard<std::mutex> lk(c->w->mu);
    *out = c->n;
    return 0;
}

void* fakerccl_live_comm(int nth) {
    std::lock_guard<std::mutex> lk(g_mu);
    return nth >= 0 && nth < (int)g_live.size() ? g_live[nth] : nullptr;
}

int fakerccl_comm_rank(void* comm) { return comm ? static_cast<Comm*>(comm)->rank : -1; }

int64_t fakerccl_comms_created(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_created;
}

int64_t fakerccl_init_calls(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_inits;
}

int64_t fakerccl_messages(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_messages;
}

void fakerccl_fail_next_init(int code) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_fail_next_init = code;
}

}  // extern "C"

// ---- the declarations above are what the group casts to (gamma_hip_group_rccl.h), and its enumerators are the ones used here ----
namespace {
using gamma_group_rccl::RcclApi;
#define SAME_AS_THE_GROUPS(entry, member) \
    static_assert(std::is_same<decltype(&entry), decltype(RcclApi::member)>::value, #entry ": not the pointer type of RcclApi::" #member)
SAME_AS_THE_GROUPS(ncclCommInitAll, CommInitAll);
SAME_AS_THE_GROUPS(ncclCommDestroy, CommDestroy);
SAME_AS_THE_GROUPS(ncclAllGather, AllGather);
SAME_AS_THE_GROUPS(ncclAllReduce, AllReduce);
SAME_AS_THE_GROUPS(ncclSend, Send);
SAME_AS_THE_GROUPS(ncclRecv, Recv);
SAME_AS_THE_GROUPS(ncclGroupStart, GroupStart);
SAME_AS_THE_GROUPS(ncclGroupEnd, GroupEnd);
SAME_AS_THE_GROUPS(ncclGetErrorString, GetErrorString);
static_assert(gamma_group_rccl::kNcclChar == fakeNcclInt8 && gamma_group_rccl::kNcclFloat == fakeNcclFloat32 &&
                  gamma_group_rccl::kNcclMax == fakeNcclMax && gamma_group_rccl::kNcclMin == fakeNcclMin,
              "the stand-in's enumerators are not the group's");
}  // namespace
