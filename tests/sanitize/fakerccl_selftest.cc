// fakerccl_selftest.cc -- TEST INFRASTRUCTURE: the stand-in communicator (fakerccl/) held to its own rules, W = 3 threads.  A
// correct all-gather (out of place and in place), min, max and grouped all-to-all must equal a plain loop bit for bit; a count
// that differs on one rank, an in-place all-gather at the wrong offset, a recv shorter than its send and a reduction outside
// min / max must each print "FAKE RCCL:" and return non-zero AT EVERY RANK, without hanging.  Without this a stand-in that
// checks nothing would make group_protocol.cc's RCCL cases vacuous.
#include <signal.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <functional>
#include <thread>
#include <vector>

#include "fakerccl/fakerccl.h"

namespace {

constexpr int W = 3;
void* g_comm[W];
const char* g_case = "setup";
int n_cases = 0, n_failures = 0;

void on_alarm(int) {
    const char a[] = "\nWATCHDOG: the stand-in did not return -- ";
    (void)!write(2, a, sizeof(a) - 1);
    (void)!write(2, g_case, strlen(g_case));
    (void)!write(2, "\n", 1);
    _exit(3);
}

// body(rank) on W threads; the ranks' return codes
std::vector<int> ranks(const std::function<int(int)>& body) {
    std::vector<int> rc(W, -1);
    std::vector<std::thread> th;
    alarm(30);
    for (int r = 0; r < W; r++) th.emplace_back([&, r] { rc[r] = body(r); });
    for (auto& t : th) t.join();
    alarm(0);
    return rc;
}

void report(const char* name, bool ok) {
    n_cases++;
    n_failures += !ok;
    printf("%-72s %s\n", name, ok ? "ok" : "FAILED");
}

// every rank returned 0 and `same` holds
void expect_ok(const char* name, const std::function<int(int)>& body, const std::function<bool()>& same) {
    g_case = name;
    const int64_t said = fakerccl_messages();
    const std::vector<int> rc = ranks(body);
    bool ok = fakerccl_messages() == said;
    for (int r = 0; r < W; r++) ok = ok && rc[r] == 0;
    report(name, ok && same());
}

// every rank returned non-zero, and the stand-in said why
void expect_refused(const char* name, const std::function<int(int)>& body) {
    g_case = name;
    const int64_t said = fakerccl_messages();
    const std::vector<int> rc = ranks(body);
    bool ok = fakerccl_messages() > said;
    for (int r = 0; r < W; r++) ok = ok && rc[r] != 0;
    report(name, ok);
}

float val(int r, int t) { return (float)((r * 7919 + t * 104729) % 1009) - 500.25f * (float)((r + t) % 3); }

}  // namespace

int main() {
    signal(SIGALRM, on_alarm);
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int devs[W] = {0, 1, 2}, twice[W] = {0, 1, 0};
    void* none[W] = {nullptr, nullptr, nullptr};

    // ---- ncclCommInitAll ----
    int64_t said = fakerccl_messages();
    report("ncclCommInitAll refuses a device named twice", ncclCommInitAll(none, W, twice) != 0 && fakerccl_messages() > said && !none[0]);
    fakerccl_fail_next_init(fakeNcclInternalError);
    said = fakerccl_messages();
    report("ncclCommInitAll fails once when told to, without a message",
           ncclCommInitAll(none, W, devs) == fakeNcclInternalError && fakerccl_messages() == said && !none[0] && fakerccl_comms_created() == 0);
    report("ncclCommInitAll forms a communicator per rank",
           ncclCommInitAll(g_comm, W, devs) == 0 && fakerccl_comms_created() == W && fakerccl_init_calls() == 3 && fakerccl_live_comm(2) == g_comm[2] &&
               fakerccl_comm_rank(g_comm[1]) == 1 && !fakerccl_live_comm(W));

    // ---- correct calls, against a plain loop ----
    const int N = 5;   // elements per rank
    std::vector<float> in[W], out[W], want;
    for (int r = 0; r < W; r++)
        for (int t = 0; t < N; t++) in[r].push_back(val(r, t));

    for (int r = 0; r < W; r++) out[r].assign(W * N, -1.f);
    want.clear();
    for (int r = 0; r < W; r++) want.insert(want.end(), in[r].begin(), in[r].end());
    expect_ok("ncclAllGather out of place", [&](int r) { return ncclAllGather(in[r].data(), out[r].data(), N, fakeNcclFloat32, g_comm[r], nullptr); },
              [&] { return out[0] == want && out[1] == want && out[2] == want; });

    for (int r = 0; r < W; r++) {
        out[r].assign(W * N, -1.f);
        std::copy(in[r].begin(), in[r].end(), out[r].begin() + r * N);
    }
    expect_ok("ncclAllGather in place, counted in bytes, inside a group",
              [&](int r) {
                  int e = ncclGroupStart();
                  e |= ncclAllGather((char*)out[r].data() + (size_t)r * N * 4, out[r].data(), (size_t)N * 4, fakeNcclInt8, g_comm[r], nullptr);
                  return e | ncclGroupEnd();
              },
              [&] { return out[0] == want && out[1] == want && out[2] == want; });

    for (int take_max = 0; take_max < 2; take_max++) {
        want.assign(in[0].begin(), in[0].end());
        for (int r = 1; r < W; r++)
            for (int t = 0; t < N; t++) want[t] = take_max ? (in[r][t] > want[t] ? in[r][t] : want[t]) : (in[r][t] < want[t] ? in[r][t] : want[t]);
        for (int r = 0; r < W; r++) out[r] = in[r];
        expect_ok(take_max ? "ncclAllReduce max, in place" : "ncclAllReduce min, in place",
                  [&](int r) { return ncclAllReduce(out[r].data(), out[r].data(), N, fakeNcclFloat32, take_max ? fakeNcclMax : fakeNcclMin, g_comm[r], nullptr); },
                  [&] { return out[0] == want && out[1] == want && out[2] == want; });
    }

    // all-to-all with rows of unequal length (rank j's slice has j + 1 elements), two columns per pair, self-sends included
    std::vector<float> a2a[W], b2a[W], wanta[W], wantb[W];
    for (int r = 0; r < W; r++) {
        a2a[r].assign((size_t)W * (r + 1), -1.f);
        b2a[r].assign((size_t)W * (r + 1), -1.f);
        for (int j = 0; j < W; j++)
            for (int t = 0; t < r + 1; t++) {
                wanta[r].push_back(val(j, 10 * r + t));
                wantb[r].push_back(val(j, 100 + 10 * r + t));
            }
    }
    expect_ok("grouped ncclSend / ncclRecv: an all-to-all of two columns",
              [&](int r) {
                  std::vector<float> sa[W], sb[W];
                  for (int j = 0; j < W; j++)
                      for (int t = 0; t < j + 1; t++) {
                          sa[j].push_back(val(r, 10 * j + t));
                          sb[j].push_back(val(r, 100 + 10 * j + t));
                      }
                  int e = ncclGroupStart();
                  for (int j = 0; j < W; j++) {
                      e |= ncclSend(sa[j].data(), (size_t)(j + 1) * 4, fakeNcclInt8, j, g_comm[r], nullptr);
                      e |= ncclSend(sb[j].data(), (size_t)(j + 1) * 4, fakeNcclInt8, j, g_comm[r], nullptr);
                      e |= ncclRecv(a2a[r].data() + (size_t)j * (r + 1), (size_t)(r + 1) * 4, fakeNcclInt8, j, g_comm[r], nullptr);
                      e |= ncclRecv(b2a[r].data() + (size_t)j * (r + 1), (size_t)(r + 1) * 4, fakeNcclInt8, j, g_comm[r], nullptr);
                  }
                  return e | ncclGroupEnd();
              },
              [&] {
                  bool ok = true;
                  for (int r = 0; r < W; r++) ok = ok && a2a[r] == wanta[r] && b2a[r] == wantb[r];
                  return ok;
              });
    fakerccl_counts n1;
    report("the counters saw those calls", fakerccl_get_counts(g_comm[1], &n1) == 0 && n1.all_gather == 2 && n1.all_reduce == 2 && n1.send == 2 * W &&
                                               n1.recv == 2 * W && n1.group_end == 2);

    // ---- what the stand-in must refuse: at every rank, with a message, without hanging ----
    for (int r = 0; r < W; r++) out[r].assign(W * N, -1.f);
    expect_refused("refused: a count that differs on one rank",
                   [&](int r) { return ncclAllGather(in[r].data(), out[r].data(), r == 2 ? N - 1 : N, fakeNcclFloat32, g_comm[r], nullptr); });
    expect_refused("refused: an all-reduce that one rank calls with the other reduction",
                   [&](int r) { return ncclAllReduce(out[r].data(), out[r].data(), N, fakeNcclFloat32, r == 1 ? fakeNcclMax : fakeNcclMin, g_comm[r], nullptr); });
    expect_refused("refused: an in-place all-gather at the wrong offset",
                   [&](int r) { return ncclAllGather(out[r].data() + (r == 2 ? 1 : r) * N, out[r].data(), N, fakeNcclFloat32, g_comm[r], nullptr); });
    expect_refused("refused: a recv shorter than its send", [&](int r) {
        int e = ncclGroupStart();
        for (int j = 0; j < W; j++) {
            e |= ncclSend(in[r].data(), (size_t)N * 4, fakeNcclInt8, j, g_comm[r], nullptr);
            e |= ncclRecv(out[r].data() + (size_t)j * N, (size_t)(r == 0 && j == 1 ? N - 1 : N) * 4, fakeNcclInt8, j, g_comm[r], nullptr);
        }
        e |= ncclGroupEnd();
        return r == 0 || r == 1 ? e : !e;   // the two ends of the pair get the error, rank 2's exchanges were fine
    });
    expect_refused("refused: a reduction outside min / max",
                   [&](int r) { return ncclAllReduce(out[r].data(), out[r].data(), N, fakeNcclFloat32, fakeNcclSum, g_comm[r], nullptr); });
    expect_refused("refused: a reduction of another datatype",
                   [&](int r) { return ncclAllReduce(out[r].data(), out[r].data(), N, fakeNcclInt32, fakeNcclMin, g_comm[r], nullptr); });

    // the communicator is still good after a refusal
    want.clear();
    for (int r = 0; r < W; r++) want.insert(want.end(), in[r].begin(), in[r].end());
    expect_ok("ncclAllGather after the refusals", [&](int r) { return ncclAllGather(in[r].data(), out[r].data(), N, fakeNcclFloat32, g_comm[r], nullptr); },
              [&] { return out[0] == want && out[1] == want && out[2] == want; });

    bool gone = true;
    for (int r = 0; r < W; r++) gone = ncclCommDestroy(g_comm[r]) == 0 && gone;
    report("ncclCommDestroy", gone && !fakerccl_live_comm(0));
    printf("fakerccl_selftest: %d cases, %d refusals said, %d failures\n", n_cases, (int)fakerccl_messages(), n_failures);
    return n_failures ? 1 : 0;
}
