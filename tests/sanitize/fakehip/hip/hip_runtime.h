// TEST INFRASTRUCTURE: the handful of HIP runtime calls gamma_amd/csrc/gamma_hip_group.cpp makes (streams, events, device
// buffers, copies), with "device memory" = host memory and every copy done on the calling thread -- so that the group's OWN
// code (member threads, barriers, go / no-go snapshots, error paths) builds with g++ and runs under ThreadSanitizer in a
// container without a GPU (tests/sanitize/Makefile).  Not a HIP implementation; never shipped.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>

typedef int hipError_t;
#define hipSuccess 0
#define hipErrorOutOfMemory 2
#define hipErrorPeerAccessAlreadyEnabled 704
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
#define hipEventDisableTiming 2u
#define hipEventBlockingSync 1u

static inline hipError_t hipSetDevice(int) { return hipSuccess; }

// ---- knobs of the test programs (tests/sanitize/dev_mem_check.cc) ----------------------------------------------------
// fakehip::fail_*: "the n-th such call from now fails, and the count - 1 after it" -- fail_alloc counts hipMalloc and
// hipMemCreate (out of memory), fail_copy counts copies, fills and stream syncs, fail_map hipMemMap, fail_access
// hipMemSetAccess (hipErrorUnknown), fail_reserve hipMemAddressReserve.  fakehip::live_*: allocations not yet freed, memory handles not yet released, address
// ranges not yet given back.
#define hipErrorUnknown 999
namespace fakehip {
struct Knob {
    std::atomic<long> in{0}, count{0};
    void arm(long n, long cnt = 1) { count = cnt, in = n; }
    void off() { in = 0, count = 0; }
    bool hit() {   // true: this call fails
        if (count.load() <= 0) return false;
        if (in.load() > 1) {
            in--;
            return false;
        }
        count--;
        return true;
    }
};
inline Knob fail_alloc, fail_copy, fail_map, fail_access, fail_reserve;
inline std::atomic<long> live_allocs{0}, live_handles{0}, live_ranges{0};
}  // namespace fakehip

static inline hipError_t hipMalloc(void** p, size_t n) {
    *p = nullptr;
    if (fakehip::fail_alloc.hit()) return hipErrorOutOfMemory;
    *p = malloc(n ? n : 1);
    if (*p) fakehip::live_allocs++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static inline hipError_t hipFree(void* p) {
    if (p) fakehip::live_allocs--;
    free(p);
    return hipSuccess;
}
// (-DFAKEHIP_DEFERRED, the build of tests/sanitize/call_slots_check.cc alone: copies and event records wait in their stream's queue
//  until the program drains it -- hip_deferred.h, included at the end, has those calls then; everything else is as it is here)
#ifndef FAKEHIP_DEFERRED
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    if (fakehip::fail_copy.hit()) return hipErrorUnknown;
    memcpy(d, s, n);
    return hipSuccess;
}
#endif
static inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    if (fakehip::fail_copy.hit()) return hipErrorUnknown;
    memset(d, v, n);
    return hipSuccess;
}
static inline hipError_t hipMemcpyPeerAsync(void* d, int, const void* s, int, size_t n, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return fakehip::fail_copy.hit() ? hipErrorUnknown : hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
#ifndef FAKEHIP_DEFERRED
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
#endif
static inline hipError_t hipDeviceCanAccessPeer(int* can, int, int) { *can = 1; return hipSuccess; }
static inline hipError_t hipDeviceEnablePeerAccess(int, unsigned) { return hipSuccess; }
static inline hipError_t hipGetLastError(void) { return hipSuccess; }
static inline const char* hipGetErrorString(hipError_t) { return "fake hip error"; }

// ---- virtual memory management: an address range is ONE host allocation (hipMemGetInfo reports a small device), a mapped
// chunk an interval of it.  Strict about what the runtime leaves undefined: the process aborts with a message on a chunk
// mapped over a mapped interval, an unmap of something that is not mapped, a handle released twice and hipMemSetAccess over
// addresses that are not mapped.
typedef unsigned long long hipMemGenericAllocationHandle_t;
enum hipMemAllocationType { hipMemAllocationTypePinned = 1 };
enum hipMemLocationType { hipMemLocationTypeDevice = 1 };
enum hipMemAllocationGranularity_flags { hipMemAllocationGranularityMinimum = 0, hipMemAllocationGranularityRecommended = 1 };
enum hipMemAccessFlags { hipMemAccessFlagsProtNone = 0, hipMemAccessFlagsProtRead = 1, hipMemAccessFlagsProtReadWrite = 3 };
struct hipMemLocation { hipMemLocationType type; int id; };
struct hipMemAllocationProp { hipMemAllocationType type; hipMemLocation location; };
struct hipMemAccessDesc { hipMemLocation location; hipMemAccessFlags flags; };

namespace fakehip {
constexpr size_t kTotalBytes = (size_t)64 << 20;
struct Vm {
    std::mutex mu;
    std::map<char*, size_t> ranges;                                   // reserved: base -> bytes
    std::map<char*, size_t> maps;                                     // mapped: start -> bytes
    std::map<hipMemGenericAllocationHandle_t, size_t> handles;        // created, not yet released
    hipMemGenericAllocationHandle_t next = 1;
};
inline Vm vm;
[[noreturn]] inline void die(const char* what) {
    fprintf(stderr, "fakehip: %s\n", what);
    abort();
}
// (under vm.mu) is [at, at + n) covered by mapped intervals without a gap?
inline bool covered(char* at, size_t n) {
    char* end = at + n;
    while (at < end) {
        auto it = vm.maps.upper_bound(at);
        if (it == vm.maps.begin()) return false;
        --it;
        if (it->first + it->second <= at) return false;
        at = it->first + it->second;
    }
    return true;
}
}  // namespace fakehip

static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) {
    *free_b = *total_b = fakehip::kTotalBytes;
    return hipSuccess;
}
static inline hipError_t hipMemGetAllocationGranularity(size_t* g, const hipMemAllocationProp*, hipMemAllocationGranularity_flags) {
    *g = 4096;
    return hipSuccess;
}
static inline hipError_t hipMemAddressReserve(void** va, size_t bytes, size_t, void*, unsigned long long) {
    *va = fakehip::fail_reserve.hit() ? nullptr : malloc(bytes);
    if (!*va) return hipErrorOutOfMemory;
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    fakehip::vm.ranges[(char*)*va] = bytes;
    fakehip::live_ranges++;
    return hipSuccess;
}
static inline hipError_t hipMemAddressFree(void* va, size_t bytes) {
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    auto it = fakehip::vm.ranges.find((char*)va);
    if (it == fakehip::vm.ranges.end() || it->second != bytes) fakehip::die("hipMemAddressFree of a range that was not reserved");
    auto m = fakehip::vm.maps.lower_bound((char*)va);
    if (m != fakehip::vm.maps.end() && m->first < (char*)va + bytes) fakehip::die("hipMemAddressFree of a range with a mapped chunk");
    fakehip::vm.ranges.erase(it);
    fakehip::live_ranges--;
    free(va);
    return hipSuccess;
}
static inline hipError_t hipMemCreate(hipMemGenericAllocationHandle_t* h, size_t bytes, const hipMemAllocationProp*, unsigned long long) {
    if (fakehip::fail_alloc.hit()) return hipErrorOutOfMemory;
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    *h = fakehip::vm.next++;
    fakehip::vm.handles[*h] = bytes;
    fakehip::live_handles++;
    return hipSuccess;
}
static inline hipError_t hipMemRelease(hipMemGenericAllocationHandle_t h) {
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    if (!fakehip::vm.handles.erase(h)) fakehip::die("hipMemRelease of a handle that is not live (released twice?)");
    fakehip::live_handles--;
    return hipSuccess;
}
static inline hipError_t hipMemMap(void* at, size_t bytes, size_t, hipMemGenericAllocationHandle_t h, unsigned long long) {
    if (fakehip::fail_map.hit()) return hipErrorUnknown;
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    char* a = (char*)at;
    auto hit = fakehip::vm.handles.find(h);
    if (hit == fakehip::vm.handles.end() || hit->second != bytes) fakehip::die("hipMemMap of a handle that is not live, or of another size");
    auto r = fakehip::vm.ranges.upper_bound(a);
    if (r == fakehip::vm.ranges.begin()) fakehip::die("hipMemMap outside every reserved range");
    --r;
    if (a + bytes > r->first + r->second) fakehip::die("hipMemMap beyond the reserved range");
    auto m = fakehip::vm.maps.upper_bound(a);
    if (m != fakehip::vm.maps.end() && m->first < a + bytes) fakehip::die("hipMemMap over a mapped interval");
    if (m != fakehip::vm.maps.begin()) {
        --m;
        if (m->first + m->second > a) fakehip::die("hipMemMap over a mapped interval");
    }
    fakehip::vm.maps[a] = bytes;
    return hipSuccess;
}
static inline hipError_t hipMemUnmap(void* at, size_t bytes) {
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    auto m = fakehip::vm.maps.find((char*)at);
    if (m == fakehip::vm.maps.end() || m->second != bytes) fakehip::die("hipMemUnmap of something that is not mapped");
    fakehip::vm.maps.erase(m);
    return hipSuccess;
}
static inline hipError_t hipMemSetAccess(void* at, size_t bytes, const hipMemAccessDesc*, size_t) {
    std::lock_guard<std::mutex> g(fakehip::vm.mu);
    if (!fakehip::covered((char*)at, bytes)) fakehip::die("hipMemSetAccess over addresses that are not mapped");
    return fakehip::fail_access.hit() ? hipErrorUnknown : hipSuccess;
}

#ifdef FAKEHIP_DEFERRED
#include "hip_deferred.h"
#endif
