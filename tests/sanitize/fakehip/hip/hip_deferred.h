// TEST INFRASTRUCTURE: streams that DEFER (hip_runtime.h includes this under FAKEHIP_DEFERRED) -- for code whose subject is
// the order of enqueue, completion and wait (gamma_amd/csrc/call_slots.cpp; tests/sanitize/call_slots_check.cc).
//   hipMemcpyAsync, hipEventRecord : append to the stream's queue; nothing happens until the program drains it
//                                    (fakehip::drain_one / drain_to / drain_all), from the scripting thread or a "device" thread.
//   hipEventRecord                 : the event captures the stream and its position; a re-record REPLACES the capture.
//   hipEventSynchronize            : waits for the capture that is current when it is called (what HIP documents); an event that
//                                    was never recorded does not wait.  fakehip::self_drain = true (a single scripting thread):
//                                    instead of blocking it drains the stream up to the capture, as a device left alone would.
//   hipHostMalloc, events          : counted (live_host, live_events); fail_host / fail_event make the n-th creation fail.
// Not a HIP implementation; never shipped.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <deque>

#define hipHostMallocDefault 0u
#define hipStreamNonBlocking 1u

namespace fakehip {
struct Item {
    void* dst;         // a copy; nullptr: an event record (a position marker)
    const void* src;
    size_t n;
};
inline std::mutex dmu;                  // every stream's queue and counts, every event's capture
inline std::condition_variable dcv;     // a stream moved on
inline bool self_drain = false;
inline Knob fail_event, fail_host;
inline std::atomic<long> live_events{0}, live_host{0}, live_streams{0};
}  // namespace fakehip

struct fake_stream {
    std::deque<fakehip::Item> q;
    uint64_t enq = 0, done = 0;   // items appended / executed
};
struct fake_event {
    fake_stream* st = nullptr;    // the capture: complete when st->done >= pos
    uint64_t pos = 0;
};

namespace fakehip {
// (under dmu) the oldest item of the stream, if it has one
inline bool step_locked(fake_stream* s) {
    if (s->q.empty()) return false;
    const Item it = s->q.front();
    s->q.pop_front();
    if (it.dst) memcpy(it.dst, it.src, it.n);
    s->done++;
    return true;
}
inline bool drain_one(hipStream_t s) {
    std::lock_guard<std::mutex> g(dmu);
    const bool did = step_locked(s);
    if (did) dcv.notify_all();
    return did;
}
inline uint64_t mark(hipStream_t s) {   // the position behind everything enqueued so far
    std::lock_guard<std::mutex> g(dmu);
    return s->enq;
}
inline void drain_to(hipStream_t s, uint64_t m) {
    std::lock_guard<std::mutex> g(dmu);
    while (s->done < m && step_locked(s)) {}
    dcv.notify_all();
}
inline void drain_all(hipStream_t s) { drain_to(s, UINT64_MAX); }
}  // namespace fakehip

static inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    *s = new fake_stream();
    fakehip::live_streams++;
    return hipSuccess;
}
static inline hipError_t hipStreamDestroy(hipStream_t s) {
    if (s && !s->q.empty()) fakehip::die("hipStreamDestroy of a stream with work in its queue");
    if (s) fakehip::live_streams--;
    delete s;
    return hipSuccess;
}
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
    if (fakehip::fail_copy.hit()) return hipErrorUnknown;
    std::lock_guard<std::mutex> g(fakehip::dmu);
    st->q.push_back({d, s, n});
    st->enq++;
    return hipSuccess;
}
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = nullptr;
    if (fakehip::fail_event.hit()) return hipErrorOutOfMemory;
    *e = new fake_event();
    fakehip::live_events++;
    return hipSuccess;
}
static inline hipError_t hipEventDestroy(hipEvent_t e) {
    if (e) fakehip::live_events--;
    delete e;
    return hipSuccess;
}
static inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    std::lock_guard<std::mutex> g(fakehip::dmu);
    st->q.push_back({nullptr, nullptr, 0});
    st->enq++;
    e->st = st, e->pos = st->enq;
    return hipSuccess;
}
static inline hipError_t hipEventSynchronize(hipEvent_t e) {
    std::unique_lock<std::mutex> g(fakehip::dmu);
    fake_stream* const st = e->st;   // the capture as of this call: a later re-record does not move the goal
    const uint64_t pos = e->pos;
    if (!st) return hipSuccess;
    if (fakehip::self_drain) {
        while (st->done < pos && fakehip::step_locked(st)) {}
        fakehip::dcv.notify_all();
        return st->done >= pos ? hipSuccess : hipErrorUnknown;
    }
    fakehip::dcv.wait(g, [&] { return st->done >= pos; });
    return hipSuccess;
}
static inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
    *p = nullptr;
    if (fakehip::fail_host.hit()) return hipErrorOutOfMemory;
    *p = malloc(n ? n : 1);
    if (*p) fakehip::live_host++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static inline hipError_t hipHostFree(void* p) {
    if (p) fakehip::live_host--;
    free(p);
    return hipSuccess;
}
