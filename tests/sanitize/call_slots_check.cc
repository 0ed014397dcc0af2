// TEST: the completion slots of the _wait entries (gamma_amd/csrc/call_slots.h / .cpp) against the deferring streams of
// fakehip/hip/hip_deferred.h -- every waiter reads the overflow word of ITS call, however many calls are in flight and however
// late it looks.  This program plays the search: take a slot, enqueue the copy of the call's "device overflow word" (a plain int
// set per call) into the slot's pinned word, arm the slot behind it; later wait, read, give back.  Scripted cases a-f on one
// thread that steps the stream itself, then 8 waiter threads beside a "device" thread.  Links call_slots.cpp alone; built once
// with AddressSanitizer + UBSan and once with ThreadSanitizer by tests/test_call_slots.py.
#ifndef FAKEHIP_DEFERRED
#error "build this program and call_slots.cpp with -DFAKEHIP_DEFERRED (fakehip's deferring streams)"
#endif
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <mutex>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../../gamma_amd/csrc/call_slots.h"

using ghi::CallSlot;
using ghi::CallSlots;

namespace {

int g_failed = 0;        // EXPECTs that did not hold
long g_scripted = 0;     // calls made by the scripted cases
const char* g_case = "";

#define EXPECT(c)                                                                              \
    do {                                                                                       \
        if (!(c)) {                                                                            \
            fprintf(stderr, "case %s: %s:%d: EXPECT(%s) failed\n", g_case, __FILE__, __LINE__, #c); \
            g_failed++;                                                                        \
        }                                                                                      \
    } while (0)

// one stream, one pool, the calls enqueued on them
struct Sim {
    struct Call {
        CallSlot* s = nullptr;
        int dev = 0;         // the device overflow word of the call
        uint64_t mark = 0;   // the stream's position behind the call
    };
    CallSlots pool;
    hipStream_t st = nullptr;
    std::deque<Call> calls;   // (a deque: the queued copies hold addresses of its elements)
    Sim() { (void)hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    ~Sim() {
        fakehip::drain_all(st);
        pool.release();
        (void)hipStreamDestroy(st);
    }
    // take / copy / arm; -1 if the take failed
    int enqueue(int word) {
        CallSlot* s = nullptr;
        if (pool.take(&s) != hipSuccess) {
            EXPECT(s == nullptr);
            return -1;
        }
        EXPECT(*s->over == 0);
        calls.emplace_back();
        Call& c = calls.back();
        c.s = s, c.dev = word;
        EXPECT(hipMemcpyAsync(s->over, &c.dev, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess);
        EXPECT(CallSlots::arm(s, st) == hipSuccess);
        c.mark = fakehip::mark(st);
        g_scripted++;
        return (int)calls.size() - 1;
    }
    // wait / read / give back
    int finish(int i) {
        Call& c = calls[i];
        EXPECT(CallSlots::wait(c.s) == hipSuccess);
        const int w = CallSlots::word(c.s);
        pool.give_back(c.s);
        c.s = nullptr;
        return w;
    }
};

int word_of(uint64_t seq) {   // a call's word as a function of its sequence number: zero for about half, distinct otherwise
    const uint32_t h = (uint32_t)(seq + 1) * 2654435761u;
    return (h >> 13) & 1 ? (int)(seq + 1) : 0;
}

// a. four calls in flight with mixed words
void case_a() {
    g_case = "a";
    const int words[4] = {1, 0, 0, 1};
    for (int pre = 0; pre < 2; pre++) {   // the device ahead of the waiters / driven by them
        Sim m;
        for (int w : words) m.enqueue(w);
        if (pre) fakehip::drain_all(m.st);
        for (int i = 0; i < 4; i++) EXPECT(m.finish(i) == words[i]);
        EXPECT(m.pool.busy() == 0);
    }
}

// b / c. call 0 and call 4, one of them overflowing, three calls between them
void case_bc(const char* name, int w0, int w4) {
    const int words[5] = {w0, 0, 1, 0, w4};
    {   // variant 1: the device is through call 0 only when waiter 0 looks
        g_case = name;
        Sim m;
        for (int w : words) m.enqueue(w);
        fakehip::drain_to(m.st, m.calls[0].mark);
        EXPECT(m.finish(0) == w0);
        for (int i = 1; i < 5; i++) EXPECT(m.finish(i) == words[i]);
    }
    {   // variant 2: waiter 0 is late -- it starts its wait after call 4 was enqueued and everything has run
        Sim m;
        for (int w : words) m.enqueue(w);
        fakehip::drain_all(m.st);
        EXPECT(m.finish(0) == w0);
        EXPECT(m.finish(4) == w4);
        for (int i = 1; i < 4; i++) EXPECT(m.finish(i) == words[i]);
    }
}

// d. more calls in flight than any fixed number of slots, waited in three orders
void case_d() {
    g_case = "d";
    std::mt19937 rng(20240611);
    for (int n : {5, 8, 16, 33})
        for (int order = 0; order < 3; order++)
            for (int pre = 0; pre < 2; pre++) {
                Sim m;
                std::vector<int> words(n), idx(n);
                for (int i = 0; i < n; i++) words[i] = (rng() & 1) ? (int)(rng() % 1000) + 1 : 0;
                std::iota(idx.begin(), idx.end(), 0);
                if (order == 1) std::reverse(idx.begin(), idx.end());
                if (order == 2) std::shuffle(idx.begin(), idx.end(), rng);
                for (int w : words) m.enqueue(w);
                EXPECT(m.pool.busy() == (size_t)n);
                if (pre) fakehip::drain_all(m.st);
                for (int i : idx) EXPECT(m.finish(i) == words[i]);
                EXPECT(m.pool.busy() == 0);
                EXPECT(m.pool.slots() <= (size_t)n);
            }
}

// e. reuse: the pool holds no more slots than calls were ever in flight at one time (call_slots.h: the bound)
void case_e() {
    g_case = "e";
    Sim m;
    const int kInFlight = 3;
    for (int i = 0; i < 1000; i++) {
        m.enqueue(word_of(i));
        if (i >= kInFlight - 1) EXPECT(m.finish(i - (kInFlight - 1)) == word_of(i - (kInFlight - 1)));
        EXPECT(m.pool.busy() <= (size_t)kInFlight);
    }
    EXPECT(m.finish(998) == word_of(998));
    EXPECT(m.finish(999) == word_of(999));
    EXPECT(m.pool.slots() <= (size_t)kInFlight);
    EXPECT(m.pool.busy() == 0);
}

// f. the creation of the n-th take fails: the error comes back, nothing is leaked or left busy, the next take succeeds
void case_f() {
    g_case = "f";
    for (int kind = 0; kind < 2; kind++)
        for (int n = 1; n <= 6; n++) {
            fakehip::Knob& knob = kind ? fakehip::fail_host : fakehip::fail_event;
            {
                Sim m;
                knob.arm(n);   // every take below finds no free slot: the n-th creation is the n-th take's
                for (int i = 0; i < n - 1; i++) EXPECT(m.enqueue(word_of(i)) == i);
                const size_t slots = m.pool.slots(), busy = m.pool.busy();
                const long ev = fakehip::live_events, host = fakehip::live_host;
                EXPECT(m.enqueue(1) == -1);
                EXPECT(m.pool.slots() == slots && m.pool.busy() == busy);
                EXPECT(fakehip::live_events == ev && fakehip::live_host == host);
                knob.off();
                EXPECT(m.enqueue(word_of(n - 1)) == n - 1);
                EXPECT(m.pool.busy() == busy + 1);
                for (int i = 0; i < n; i++) EXPECT(m.finish(i) == word_of(i));
                EXPECT(m.pool.busy() == 0);
            }
            knob.off();
            EXPECT(fakehip::live_events == 0 && fakehip::live_host == 0 && fakehip::live_streams == 0);
        }
}

// threaded: 8 waiters x 200 calls under a mutex that stands for the search lock, beside a device thread that drains with pauses
long threaded(long* mismatches) {
    const int kThreads = 8, kCalls = 200;
    fakehip::self_drain = false;
    CallSlots pool;
    hipStream_t st = nullptr;
    (void)hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    std::mutex search_mu;
    uint64_t seq = 0;                                   // under search_mu
    std::vector<int> dev((size_t)kThreads * kCalls);    // the calls' device overflow words, by sequence number
    std::atomic<long> bad{0}, finished{0};
    std::atomic<bool> stop{false};
    std::thread device([&] {
        std::mt19937 rng(7);
        while (!stop.load()) {
            if (!fakehip::drain_one(st)) std::this_thread::yield();
            else if ((rng() & 3) == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 200));
        }
    });
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; t++)
        th.emplace_back([&] {
            for (int i = 0; i < kCalls; i++) {
                CallSlot* s = nullptr;
                uint64_t mine = 0;
                {
                    std::lock_guard<std::mutex> lk(search_mu);
                    mine = seq++;
                    if (pool.take(&s) != hipSuccess) {
                        bad++;
                        continue;
                    }
                    dev[mine] = word_of(mine);
                    if (hipMemcpyAsync(s->over, &dev[mine], sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) bad++;
                    if (CallSlots::arm(s, st) != hipSuccess) bad++;
                }
                if (CallSlots::wait(s) != hipSuccess) bad++;
                if (CallSlots::word(s) != word_of(mine)) bad++;
                pool.give_back(s);
                finished++;
            }
        });
    for (auto& x : th) x.join();
    stop = true;
    device.join();
    fakehip::drain_all(st);
    if (pool.busy() != 0 || pool.slots() > (size_t)kThreads) bad++;
    pool.release();
    (void)hipStreamDestroy(st);
    if (fakehip::live_events != 0 || fakehip::live_host != 0) bad++;
    *mismatches = bad;
    return finished;
}

}  // namespace

int main() {
    fakehip::self_drain = true;
    case_a();
    case_bc("b", 1, 0);
    case_bc("c", 0, 1);
    case_d();
    case_e();
    case_f();
    if (g_failed) {
        fprintf(stderr, "call slots: %d scripted expectations failed\n", g_failed);
        return 1;
    }
    long mismatches = 0;
    const long done = threaded(&mismatches);
    printf("call slots ok: %ld scripted, %ld threaded calls, %ld mismatches\n", g_scripted, done, mismatches);
    return mismatches == 0 && done == 1600 ? 0 : 1;
}
