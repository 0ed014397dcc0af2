// dev_mem.cpp -- the owners of device memory (dev_mem.h): mapped ranges, the growable array, the arena's column sets.
#include "dev_mem.h"

#include <algorithm>

// ---- mapped ranges ------------------------------------------------------------------------
bool VmRange::reserve(int device_, size_t chunk_min) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device_;
    size_t g = 0, free_b = 0, total_b = 0;
    void* va = nullptr;
    if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || g == 0 ||
        hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) {
        (void)hipGetLastError();
        return false;
    }
    // whole chunks of at least 2 MB: hipMemSetAccess refuses chunk sizes that are only a multiple of the reported 4 KB
    // granularity (tools/exp/vmm_probe.cpp)
    const size_t chunk = std::max<size_t>(std::max<size_t>(g, chunk_min), (size_t)2 << 20) / g * g;
    const size_t want = (total_b + chunk - 1) / chunk * chunk;
    if (hipMemAddressReserve(&va, want, 0, nullptr, 0) != hipSuccess || !va) {
        (void)hipGetLastError();
        return false;
    }
    base = static_cast<char*>(va);
    va_bytes = want;
    mapped = 0;
    gran = chunk;
    device = device_;
    return true;
}
hipError_t VmRange::map_to(size_t bytes, const char** what) {
    *what = "";
    if (bytes <= mapped) return hipSuccess;
    size_t add = std::max(bytes - mapped, mapped / 8);   // fewer, larger chunks
    add = (add + gran - 1) / gran * gran;
    if (mapped + add > va_bytes) add = va_bytes - mapped;
    if (mapped + add < bytes) {
        *what = "beyond the reserved address range";
        return hipErrorOutOfMemory;
    }
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    hipMemGenericAllocationHandle_t hnd;
    hipError_t e = hipMemCreate(&hnd, add, &prop, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *what = "hipMemCreate";
        return e;
    }
    char* at = base + mapped;
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    // beside the kernels of the searches in flight: page-table updates of a range they do not read yet
    // (tools/exp/vmm_probe.cpp: mapping beside kernels on the range and beside a thread allocating and launching)
    e = hipMemMap(at, add, 0, hnd, 0);
    *what = "hipMemMap";
    if (e == hipSuccess) {
        e = hipMemSetAccess(at, add, &acc, 1);
        *what = "hipMemSetAccess";
        if (e != hipSuccess) {   // seen for chunks that are not a multiple of 2 MB: the whole mapped range is accepted
            (void)hipGetLastError();
            e = hipMemSetAccess(base, mapped + add, &acc, 1);
        }
        if (e != hipSuccess) {
            (void)hipMemUnmap(at, add);
            if (!vm_unmap_fence()) tainted = true;   // (the next map_to would hand out the same address)
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipMemRelease(hnd);
        return e;
    }
    chunks.push_back(hnd);
    chunk_bytes.push_back(add);
    mapped += add;
    *what = "";
    return hipSuccess;
}
// An address that was unmapped and is mapped again (to other physical memory) read back stale contents -- zeros -- now and then
// on this runtime when the GPU was shared with other processes (tests/test_gpu_fuzz.py::test_random_realtime_script under six
// processes: 10-18 % of the scripts, whether the range was freed and reserved again or merely unmapped and remapped;
// hipDeviceSynchronize does not help).  An ordinary allocation and release by the runtime in between does (0 of 400): it goes
// through the driver's page-table path and leaves no stale translation behind.  Every unmap ends with one.
bool vm_unmap_fence() {
    // (the runtime serves allocations below 2 MB from blocks it keeps: 1 MB and 4 KB fences changed nothing, 2 / 4 / 16 / 64 MB
    //  all cured it -- 0 of 600 scripts each)
    void* t = nullptr;
    for (size_t bytes : {(size_t)16 << 20, (size_t)2 << 20}) {
        if (hipMalloc(&t, bytes) == hipSuccess) {
            (void)hipFree(t);
            return true;
        }
        (void)hipGetLastError();
    }
    return false;   // the device is out of memory: the caller must not map these addresses again
}
void VmRange::unmap_all() {
    if (!base) return;
    size_t off = 0;
    for (size_t i = 0; i < chunks.size(); i++) {
        (void)hipMemUnmap(base + off, chunk_bytes[i]);
        (void)hipMemRelease(chunks[i]);
        off += chunk_bytes[i];
    }
    if (!chunks.empty() && !vm_unmap_fence()) tainted = true;
    chunks.clear();
    chunk_bytes.clear();
    mapped = 0;
}
void VmRange::release() {
    if (!base) return;
    size_t off = 0;
    for (size_t i = 0; i < chunks.size(); i++) {
        (void)hipMemUnmap(base + off, chunk_bytes[i]);
        (void)hipMemRelease(chunks[i]);
        off += chunk_bytes[i];
    }
    // (no fence: the address range is NOT given back -- whoever reserved it next would map addresses with stale
    //  translations; it stays reserved for the life of the process, address space only)
    if (chunks.empty() || vm_unmap_fence()) (void)hipMemAddressFree(base, va_bytes);
    chunks.clear();
    chunk_bytes.clear();
    base = nullptr;
    va_bytes = mapped = 0;
}

namespace ghi {

// ---- the growable array -------------------------------------------------------------------
bool DevArray::reserve(int device, size_t chunk_min) {
    if (p || mapped || !vm.reserve(device, chunk_min)) return false;
    mapped = true;
    p = vm.base;
    return true;
}

hipError_t DevArray::grow(size_t need, size_t want, size_t keep, int fill, hipStream_t wstream, DevExclusive& ex, const char** what) {
    *what = "";
    if (need <= cap) return hipSuccess;
    if (mapped) {
        const hipError_t e = vm.map_to(need, what);
        cap = vm.mapped;
        if (e == hipSuccess) return e;
        if (vm.mapped > 0 || keep > 0 || want == 0) return e;
        // nothing is mapped yet: the range is given back and the array reallocates from here on
        vm.release();
        mapped = false;
        p = nullptr;
    }
    if (want < need) want = need;
    *what = "exclusive";
    hipError_t e = ex.exclusive();   // the old array is freed below: no search may be reading it
    if (e != hipSuccess) return e;
    void* np = nullptr;
    *what = "hipMalloc";   // (the callers' grow_fail tells THIS step by its name -- "<store>: out of memory" -- so the name stays)
    e = hipMalloc(&np, want);
    if (e != hipSuccess) return e;
    *what = "copy";
    if (fill >= 0) e = hipMemsetAsync(static_cast<char*>(np) + keep, fill, want - keep, wstream);
    if (e == hipSuccess && keep > 0) e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, wstream);
    if (e == hipSuccess) e = hipStreamSynchronize(wstream);
    if (e != hipSuccess) {
        (void)hipFree(np);
        return e;
    }
    if (p) (void)hipFree(p);
    p = np;
    cap = want;
    regrows++;
    *what = "";
    return hipSuccess;
}

void DevArray::clear(std::vector<VmRange>* retired) {
    if (mapped) {
        vm.unmap_all();   // (the address range stays reserved)
        if (vm.tainted) {   // unmapped without a fence: these addresses are not mapped again
            retired->push_back(std::move(vm));
            vm = VmRange();
            mapped = false;
            p = nullptr;
        }
    } else if (p) {
        (void)hipFree(p);
        p = nullptr;
    }
    cap = 0;
}

void DevArray::leave_vm(std::vector<VmRange>* retired) {
    clear(retired);
    if (mapped) {
        retired->push_back(std::move(vm));
        vm = VmRange();
        mapped = false;
        p = nullptr;
    }
}

void DevArray::release() {
    if (mapped) vm.release();   // unmap the chunks, release them, free the range
    else if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    mapped = false;
}

// ---- the arena's columns ------------------------------------------------------------------
int64_t DevColumns::cap() const {
    int64_t c = n > 0 ? INT64_MAX : 0;
    for (int i = 0; i < n; i++) c = std::min<int64_t>(c, (int64_t)(col[i].cap / esz[i]));
    return c;
}

bool DevColumns::start_mapped(int device, size_t chunk_min, int64_t entries) {
    bool ok = true;
    for (int i = 0; i < n && ok; i++) ok = col[i].reserve(device, chunk_min);
    const char* what = "";
    for (int i = 0; i < n && ok; i++) ok = col[i].vm.map_to((size_t)entries * esz[i], &what) == hipSuccess;
    if (!ok) {
        release();
        (void)hipGetLastError();
        return false;
    }
    for (int i = 0; i < n; i++) col[i].cap = col[i].vm.mapped;
    return true;
}

hipError_t DevColumns::grow(int64_t need, int64_t want, int64_t keep, hipStream_t wstream, DevExclusive& ex, const char** what) {
    hipError_t e = hipSuccess;
    // a mapped set never reallocates (want 0): its columns leave their ranges together or not at all
    for (int i = 0; i < n && e == hipSuccess; i++)
        e = col[i].grow((size_t)need * esz[i], mapped() ? 0 : (size_t)want * esz[i], (size_t)keep * esz[i], -1, wstream, ex, what);
    return e;
}

hipError_t DevColumns::map_target(int device, size_t chunk_min, int64_t entries, std::vector<VmRange>* retired, const char** what) {
    for (int i = 0; i < n; i++) {
        if (col[i].mapped && col[i].vm.tainted) col[i].leave_vm(retired);   // unmapped without a fence, or failed a read-back
        if (!col[i].mapped && !col[i].reserve(device, chunk_min)) {
            *what = "address range";
            return hipErrorOutOfMemory;
        }
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++) {
        e = col[i].vm.map_to((size_t)entries * esz[i], what);
        col[i].cap = col[i].vm.mapped;
    }
    return e;
}

hipError_t DevColumns::alloc_target(int64_t entries, hipStream_t wstream, DevExclusive& ex, std::vector<VmRange>* retired, const char** what) {
    for (int i = 0; i < n; i++) col[i].leave_vm(retired);
    return grow(entries, entries, 0, wstream, ex, what);
}

void DevColumns::taint() {
    for (int i = 0; i < n; i++)
        if (col[i].mapped) col[i].vm.tainted = true;
}

void DevColumns::clear(std::vector<VmRange>* retired) {
    for (int i = 0; i < NMAX; i++) col[i].clear(retired);
}

void DevColumns::release() {
    for (int i = 0; i < NMAX; i++) col[i].release();
}

ArenaSets::~ArenaSets() {
    cur.release();
    alt.release();
    for (VmRange& r : retired) r.release();
}

void ArenaSets::swap_sets() {
    for (int i = 0; i < DevColumns::NMAX; i++) {
        cur.col[i].swap(alt.col[i]);
        std::swap(cur.esz[i], alt.esz[i]);
    }
    std::swap(cur.n, alt.n);
}

}  // namespace ghi
