// dev_mem.h -- who owns device memory in libgamma_hip.so: DevBuf (a workspace), VmRange (an address range with physical
// chunks mapped behind what is in use), DevArray (the one growable array a search in flight may be reading) and DevColumns /
// ArenaSets (the arrays of the inverted-list arena, which grow together).  Host code over the HIP runtime API alone: no
// kernels, nothing of the handle -- tests/sanitize/dev_mem_check.cc runs it against a stand-in runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace ghi {

// A workspace: grows by being replaced, contents are not kept.  Owns its allocation (move-only).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

}  // namespace ghi

// A device array that grows in place: an address range reserved once (the device's whole memory -- addresses are free),
// physical chunks mapped behind what is in use.  Nothing moves, so readers of the mapped part go on while it grows.
struct VmRange {
    char* base = nullptr;
    size_t va_bytes = 0, mapped = 0, gran = 0;
    int device = 0;
    std::vector<hipMemGenericAllocationHandle_t> chunks;
    std::vector<size_t> chunk_bytes;
    bool tainted = false;   // unmapped without the fence (unmap_all): must not be mapped again
    bool on() const { return base != nullptr; }
    // false: the runtime does not offer it (nothing is left behind)
    bool reserve(int device_, size_t chunk_min);
    // mapped >= bytes afterwards; grows by at least 1/8 of what is mapped, in whole chunks.  On failure *what names the
    // step and nothing of the failed step stays mapped.
    hipError_t map_to(size_t bytes, const char** what);
    void release();
    // the physical memory goes back, the address range stays reserved (mapped = 0)
    void unmap_all();
};
// an ordinary allocation and release, behind every unmap (dev_mem.cpp says why); false: the device is out of memory
bool vm_unmap_fence();

namespace ghi {

// What DevArray::grow calls before it frees memory a search in flight may be reading: no search can start afterwards and
// the streams are drained (WriteLock is one).
struct DevExclusive {
    virtual hipError_t exclusive() = 0;

protected:
    ~DevExclusive() = default;
};

// The one growable device array: backed by a VmRange (reserve() succeeded: growth maps chunks in place) or by a plain
// allocation (growth reallocates).  grow() guarantees, whatever the backing:
//   capacity suffices : no runtime call, no exclusive.
//   mapped            : chunks are mapped behind the array; exclusive is never taken, nothing moves.
//   reallocating      : exclusive is taken before the old memory is freed; the live prefix moves on the writer stream, the
//                       stream is drained, then the old array is freed.
//   any failed step   : the new allocation is freed; pointer, capacity and contents are as before the call.
struct DevArray {
    void* p = nullptr;
    size_t cap = 0;         // bytes a reader or writer may touch
    bool mapped = false;    // backed by vm
    VmRange vm;
    int64_t regrows = 0;    // growths that moved the array (0 while mapped)
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() { release(); }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
    // an empty array takes an address range of the device's memory in chunks of at least chunk_min bytes; false: the runtime
    // does not offer it, the array reallocates
    bool reserve(int device, size_t chunk_min);
    // cap >= need afterwards.  want: the capacity of the reallocating path (the caller's growth law; >= need), 0 = this
    // array never reallocates.  keep: the live bytes carried over.  fill: 0..255 = the byte the new space [keep, cap) holds
    // (reallocating path only), < 0 = left as allocated.  A mapped array whose FIRST mapping fails while it holds nothing
    // (keep == 0) gives its range back and reallocates from then on, unless want == 0.  On failure *what names the step.
    hipError_t grow(size_t need, size_t want, size_t keep, int fill, hipStream_t wstream, DevExclusive& ex, const char** what);
    // the memory goes back (the caller holds exclusive); a mapped array keeps its range unless the unmap went without its
    // fence: such a range moves to *retired -- its addresses are not mapped again -- and the array reallocates from then on
    void clear(std::vector<VmRange>* retired);
    // clear(), and whatever range there is moves to *retired: the array is a plain one afterwards
    void leave_vm(std::vector<VmRange>* retired);
    void release();
    void swap(DevArray& o) {
        std::swap(p, o.p), std::swap(cap, o.cap), std::swap(mapped, o.mapped), std::swap(vm, o.vm), std::swap(regrows, o.regrows);
    }
};

// a DevArray of T as its readers name it: h->d_bitmap is still the pointer the kernels take
template <typename T>
struct DevArrayOf : DevArray {
    operator T*() const { return static_cast<T*>(p); }
    T* get() const { return static_cast<T*>(p); }
};

// The arrays of the inverted-list arena -- codes, ids and, where kept, code sums: one entry each per list slot -- which
// reserve, map, unmap and release together.  Capacity is the minimum over the columns.
struct DevColumns {
    static constexpr int NMAX = 3;
    DevArray col[NMAX];
    size_t esz[NMAX] = {0, 0, 0};
    int n = 0;
    void shape(size_t e0, size_t e1, size_t e2_or_0) {
        esz[0] = e0, esz[1] = e1, esz[2] = e2_or_0;
        n = e2_or_0 ? 3 : 2;
    }
    bool mapped() const { return n > 0 && col[0].mapped; }
    int64_t cap() const;   // entries
    // the first reservation: mapped ranges when the runtime offers them AND the first chunks map -- all or nothing (false
    // leaves nothing reserved in any column)
    bool start_mapped(int device, size_t chunk_min, int64_t entries);
    // cap() >= need afterwards, every column through DevArray::grow (want entries on the reallocating path, keep entries
    // carried over).  A failure at a later column leaves the earlier ones grown: cap() is the minimum.
    hipError_t grow(int64_t need, int64_t want, int64_t keep, hipStream_t wstream, DevExclusive& ex, const char** what);
    // an idle set becomes a mapped target of `entries`: tainted members go to *retired and are replaced, missing ranges are
    // reserved, then every column maps.  On failure the caller clear()s.
    hipError_t map_target(int device, size_t chunk_min, int64_t entries, std::vector<VmRange>* retired, const char** what);
    // ... a plain (hipMalloc) target: every range goes to *retired first
    hipError_t alloc_target(int64_t entries, hipStream_t wstream, DevExclusive& ex, std::vector<VmRange>* retired, const char** what);
    void taint();   // a mapped set whose contents did not read back: its addresses are not mapped again
    void clear(std::vector<VmRange>* retired);
    void release();
};

// current and alternate set (the repack moves the lists from one into the other and swaps them) and the ranges that may not
// be mapped again (address space only; freed with the sets).  The list is the handle's only one: a raw store or slot table
// that had to retire its range (DevArray::clear) hands it over here as well.
struct ArenaSets {
    DevColumns cur, alt;
    std::vector<VmRange> retired;
    ArenaSets() = default;
    ArenaSets(const ArenaSets&) = delete;
    ArenaSets& operator=(const ArenaSets&) = delete;
    ~ArenaSets();
    void swap_sets();
    // the readers' pointers and capacity = the current set's
    template <typename A, typename B, typename C>
    void adopt(A** c0, B** c1, C** c2, int64_t* cap) const {
        *c0 = cur.col[0].as<A>(), *c1 = cur.col[1].as<B>(), *c2 = cur.n > 2 ? cur.col[2].as<C>() : nullptr;
        *cap = cur.cap();
    }
};

}  // namespace ghi
using ghi::DevBuf;
