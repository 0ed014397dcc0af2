// TEST: the owners of device memory (gamma_amd/csrc/dev_mem.h / .cpp) against the stand-in runtime of fakehip/ -- growth laws,
// mapped growth, a failure injected at every step, the fence rules of mapped ranges, the arena's column sets, DevBuf.  Links
// dev_mem.cpp alone; built with AddressSanitizer + UBSan by tests/test_dev_mem.py.  After every row the stand-in's live counts
// (allocations, memory handles, address ranges) are back to what the row started with.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../gamma_amd/csrc/dev_mem.h"

using ghi::ArenaSets;
using ghi::DevArray;
using ghi::DevColumns;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

namespace {

struct Ex final : ghi::DevExclusive {
    int calls = 0;
    hipError_t exclusive() override {
        calls++;
        return hipSuccess;
    }
};

struct Live {
    long a = fakehip::live_allocs, h = fakehip::live_handles, r = fakehip::live_ranges;
    bool same() const { return a == fakehip::live_allocs && h == fakehip::live_handles && r == fakehip::live_ranges; }
};

const size_t MB = (size_t)1 << 20;
uint8_t pat(size_t i) { return (uint8_t)(i * 7 + 3); }
void put(void* p, size_t from, size_t to) {
    for (size_t i = from; i < to; i++) static_cast<uint8_t*>(p)[i] = pat(i);
}
bool holds(const void* p, size_t from, size_t to) {
    for (size_t i = from; i < to; i++)
        if (static_cast<const uint8_t*>(p)[i] != pat(i)) return false;
    return true;
}
bool filled(const void* p, size_t from, size_t to, int v) {
    for (size_t i = from; i < to; i++)
        if (static_cast<const uint8_t*>(p)[i] != (uint8_t)v) return false;
    return true;
}
void knobs_off() {
    fakehip::fail_alloc.off(), fakehip::fail_copy.off(), fakehip::fail_map.off(), fakehip::fail_access.off(), fakehip::fail_reserve.off();
}
// VmRange::map_to's rule: at least 1/8 of what is mapped, in whole chunks, clipped to the range
size_t map_rule(size_t mapped, size_t bytes, size_t gran, size_t va) {
    if (bytes <= mapped) return mapped;
    size_t add = std::max(bytes - mapped, mapped / 8);
    add = (add + gran - 1) / gran * gran;
    if (mapped + add > va) add = va - mapped;
    return mapped + add;
}

// ---- row 1: the growth laws of the call sites, on the reallocating path ------------------------------------------------
// law(need, cap) in elements -> the capacity asked for.  keep_cap: the whole old array is carried over (the bitmap).
struct Law {
    const char* name;
    size_t es;
    std::function<int64_t(int64_t, int64_t)> want;
    int fill;
    bool keep_cap;
};
int64_t max3(int64_t a, int64_t b, int64_t c) { return std::max(a, std::max(b, c)); }

void law_row(const Law& L) {
    Live live;
    {
        DevArray a;
        Ex ex;
        const char* what = "";
        int64_t have = 0;
        int growths = 0;
        for (int step = 0; step < 3; step++) {
            const int64_t cap = (int64_t)(a.cap / L.es);
            // first append: grows from nothing; second: fits; third: one element more than there is room for
            const int64_t total = step == 0 ? 1000 : step == 1 ? have + (cap - have) / 2 : cap + 1;
            const bool grows = total > cap;
            const int64_t want = L.want(total, cap);
            const size_t keep = L.keep_cap ? a.cap : (size_t)have * L.es;
            const int before = ex.calls;
            CHECK(a.grow((size_t)total * L.es, (size_t)want * L.es, keep, L.fill, nullptr, ex, &what) == hipSuccess);
            CHECK(ex.calls == before + (grows ? 1 : 0));
            if (grows) {
                growths++;
                CHECK(a.cap == (size_t)want * L.es);   // exactly the law's
                if (L.fill >= 0) CHECK(filled(a.p, keep, a.cap, L.fill));
            }
            CHECK(a.regrows == growths && !a.mapped);
            CHECK(holds(a.p, 0, (size_t)have * L.es));   // the live prefix
            put(a.p, (size_t)have * L.es, (size_t)total * L.es);
            have = total;
        }
        CHECK(growths == 2);
    }
    if (!live.same()) fprintf(stderr, "law %s\n", L.name);
    CHECK(live.same());
}

void row1_realloc_growth() {
    const auto col = [](int64_t need, int64_t cap) { return max3(need, 1 << 16, cap * 2); };
    const Law laws[] = {
        {"scalar column", 4, col, -1, false},
        {"vid2docid", 4, col, -1, false},
        {"term rows", 8, col, -1, false},
        {"term items", 4, col, -1, false},
        {"raw store", 64, [](int64_t need, int64_t cap) { return max3(need, cap + cap / 2, 1024); }, -1, false},
        {"raw slot table", 4, [](int64_t need, int64_t) { return std::max<int64_t>(need + need / 2, 1 << 16); }, 0xff, false},
        {"bitmap", 1, [](int64_t need, int64_t cap) { return std::max(need, cap * 2); }, 0x00, true},
        {"binflat", 16, [](int64_t need, int64_t cap) { return max3(need, 1024, cap + cap / 2); }, -1, false},
    };
    for (const Law& L : laws) law_row(L);
    // the arena: max(2 * cap, used + need) * 9 / 8 entries, its columns in lockstep
    for (int ncol = 2; ncol <= 3; ncol++) {
        Live live;
        {
            DevColumns c;
            Ex ex;
            const char* what = "";
            c.shape(16, 8, ncol == 3 ? 4 : 0);
            int64_t used = 0;
            for (int step = 0; step < 3; step++) {
                const int64_t cap = c.cap();
                const int64_t total = step == 0 ? 1000 : step == 1 ? used + (cap - used) / 2 : cap + 1;
                int64_t want = std::max<int64_t>(cap * 2, total);
                want += want / 8;
                const int before = ex.calls;
                CHECK(c.grow(total, want, used, nullptr, ex, &what) == hipSuccess);
                CHECK(ex.calls == before + (total > cap ? ncol : 0));   // (once per array that moves)
                if (total > cap) CHECK(c.cap() == want);
                for (int i = 0; i < ncol; i++) {
                    CHECK(c.col[i].cap == (size_t)c.cap() * c.esz[i] && !c.col[i].mapped);
                    CHECK(holds(c.col[i].p, 0, (size_t)used * c.esz[i]));
                    put(c.col[i].p, (size_t)used * c.esz[i], (size_t)total * c.esz[i]);
                }
                used = total;
            }
            CHECK(c.col[0].regrows == 2 && (ncol == 3) == (c.col[2].p != nullptr));
        }
        CHECK(live.same());
    }
}

// ---- row 2: mapped growth ------------------------------------------------------------------------------------------
void row2_mapped_growth() {
    for (size_t chunk : {8 * MB, 64 * MB}) {
        Live live;
        {
            DevArray a;
            Ex ex;
            const char* what = "";
            CHECK(a.reserve(0, chunk) && a.mapped && a.p && a.cap == 0);
            CHECK(a.vm.gran == chunk && a.vm.va_bytes == fakehip::kTotalBytes);
            void* const base = a.p;
            size_t have = 0, expect = 0;
            for (size_t need : {(size_t)1, 9 * MB, 9 * MB + 1, 40 * MB, 41 * MB}) {
                expect = map_rule(expect, need, chunk, a.vm.va_bytes);
                CHECK(a.grow(need, need * 2, have, -1, nullptr, ex, &what) == hipSuccess);
                CHECK(a.p == base && a.mapped && a.cap == expect && a.vm.mapped == expect && expect >= need);
                CHECK(ex.calls == 0 && a.regrows == 0);
                CHECK(holds(a.p, 0, have));
                put(a.p, have, need);
                have = need;
            }
            const size_t mapped = a.cap;
            const long handles = fakehip::live_handles;
            CHECK(a.grow(fakehip::kTotalBytes + 1, 0, have, -1, nullptr, ex, &what) == hipErrorOutOfMemory);
            CHECK(!strcmp(what, "beyond the reserved address range"));
            CHECK(a.p == base && a.cap == mapped && a.vm.mapped == mapped && fakehip::live_handles == handles && ex.calls == 0);
            CHECK(holds(a.p, 0, have));
        }
        CHECK(live.same());
    }
}

// ---- row 3: a failure at every step of the reallocating path ---------------------------------------------------------
void row3_realloc_failures() {
    for (int step = 0; step < 3; step++) {   // the allocation, the copy, the sync
        Live live;
        {
            DevArray a;
            Ex ex;
            const char* what = "";
            CHECK(a.grow(4096, 4096, 0, -1, nullptr, ex, &what) == hipSuccess);
            put(a.p, 0, 1000);
            void* const p = a.p;
            const long allocs = fakehip::live_allocs;
            if (step == 0) fakehip::fail_alloc.arm(1);
            else fakehip::fail_copy.arm(step);   // (no fill: the copy is the first call of its kind, the sync the second)
            const hipError_t e = a.grow(8192, 8192, 1000, -1, nullptr, ex, &what);
            CHECK(e == (step == 0 ? hipErrorOutOfMemory : hipErrorUnknown));
            CHECK(!strcmp(what, step == 0 ? "hipMalloc" : "copy"));
            CHECK(a.p == p && a.cap == 4096 && a.regrows == 1 && holds(a.p, 0, 1000));
            CHECK(fakehip::live_allocs == allocs);   // the new allocation was given back
            knobs_off();
            CHECK(a.grow(8192, 8192, 1000, 0x5a, nullptr, ex, &what) == hipSuccess);
            CHECK(a.cap == 8192 && a.regrows == 2 && holds(a.p, 0, 1000) && filled(a.p, 1000, 8192, 0x5a));
            CHECK(fakehip::live_allocs == allocs);   // ... and the old array freed
        }
        CHECK(live.same());
    }
}

// ---- row 4: a failure at every step of the mapped path ---------------------------------------------------------------
void row4_mapped_failures() {
    Live live;
    {
        DevArray a;
        Ex ex;
        const char* what = "";
        CHECK(a.reserve(0, 8 * MB));
        CHECK(a.grow(1000, 2000, 0, -1, nullptr, ex, &what) == hipSuccess && a.cap == 8 * MB);
        put(a.p, 0, 1000);
        void* const base = a.p;
        const long handles = fakehip::live_handles;
        const size_t chunks = fakehip::vm.maps.size();
        const auto unchanged = [&]() {
            return a.p == base && a.mapped && a.cap == 8 * MB && a.vm.mapped == 8 * MB && fakehip::live_handles == handles &&
                   fakehip::vm.maps.size() == chunks && holds(a.p, 0, 1000) && ex.calls == 0 && !a.vm.tainted;
        };
        fakehip::fail_alloc.arm(1);
        CHECK(a.grow(9 * MB, 0, 1000, -1, nullptr, ex, &what) == hipErrorOutOfMemory && !strcmp(what, "hipMemCreate") && unchanged());
        knobs_off();
        fakehip::fail_map.arm(1);
        CHECK(a.grow(9 * MB, 0, 1000, -1, nullptr, ex, &what) == hipErrorUnknown && !strcmp(what, "hipMemMap") && unchanged());
        knobs_off();
        fakehip::fail_access.arm(1, 2);   // the chunk and the fallback over the whole mapped range
        CHECK(a.grow(9 * MB, 0, 1000, -1, nullptr, ex, &what) == hipErrorUnknown && !strcmp(what, "hipMemSetAccess") && unchanged());
        knobs_off();
        fakehip::fail_access.arm(1, 1);   // the chunk alone: the fallback over the whole mapped range is accepted
        CHECK(a.grow(9 * MB, 0, 1000, -1, nullptr, ex, &what) == hipSuccess);
        CHECK(fakehip::fail_access.count == 0 && a.p == base && a.cap == 16 * MB && fakehip::live_handles == handles + 1 && holds(a.p, 0, 1000));
        knobs_off();
    }
    CHECK(live.same());
    // the FIRST mapping of an array that holds nothing: the range is given back, the array reallocates from then on
    {
        DevArray a;
        Ex ex;
        const char* what = "";
        CHECK(a.reserve(0, 64 * MB) && fakehip::live_ranges == live.r + 1);
        fakehip::fail_alloc.arm(1);   // hipMemCreate
        CHECK(a.grow(1000, 4096, 0, -1, nullptr, ex, &what) == hipSuccess);
        CHECK(!a.mapped && !a.vm.on() && a.p && a.cap == 4096 && a.regrows == 1 && ex.calls == 1);
        CHECK(fakehip::live_ranges == live.r && fakehip::live_allocs == live.a + 1);
    }
    CHECK(live.same());
    // ... with rows present it is an error and the array stays mapped; so it is for an array that may not reallocate
    for (int variant = 0; variant < 2; variant++) {
        DevArray a;
        Ex ex;
        const char* what = "";
        CHECK(a.reserve(0, 64 * MB));
        fakehip::fail_alloc.arm(1);
        CHECK(a.grow(1000, variant ? 0 : 4096, variant ? 0 : 64, -1, nullptr, ex, &what) == hipErrorOutOfMemory && !strcmp(what, "hipMemCreate"));
        CHECK(a.mapped && a.vm.on() && a.cap == 0 && ex.calls == 0 && a.regrows == 0 && fakehip::live_allocs == live.a);
        knobs_off();
    }
    CHECK(live.same());
}

// ---- row 5: an unmap whose fence fails -------------------------------------------------------------------------------
void row5_fence_failures() {
    Live live;
    {
        std::vector<VmRange> retired;
        DevArray a;
        Ex ex;
        const char* what = "";
        CHECK(a.reserve(0, 8 * MB) && a.grow(9 * MB, 0, 0, -1, nullptr, ex, &what) == hipSuccess);
        // with one fence size left the unmap is clean: the array keeps its range
        fakehip::fail_alloc.arm(1, 1);
        a.clear(&retired);
        CHECK(retired.empty() && a.mapped && a.p && a.cap == 0 && !a.vm.tainted && fakehip::live_handles == live.h);
        knobs_off();
        CHECK(a.grow(9 * MB, 0, 0, -1, nullptr, ex, &what) == hipSuccess);
        // both fence allocations fail: tainted, and clear() hands the range to the retired list
        fakehip::fail_alloc.arm(1, 2);
        a.clear(&retired);
        knobs_off();
        CHECK(retired.size() == 1 && retired[0].tainted && retired[0].on() && retired[0].mapped == 0);
        CHECK(!a.mapped && !a.p && a.cap == 0 && !a.vm.on() && !a.vm.tainted);
        CHECK(fakehip::live_handles == live.h && fakehip::live_ranges == live.r + 1);   // address space only
        CHECK(a.grow(1000, 4096, 0, -1, nullptr, ex, &what) == hipSuccess && !a.mapped && a.cap == 4096 && ex.calls == 1);
        for (VmRange& r : retired) r.release();
    }
    CHECK(live.same());
    {   // VmRange::unmap_all itself
        VmRange r;
        const char* what = "";
        CHECK(r.reserve(0, 8 * MB) && r.map_to(1, &what) == hipSuccess);
        fakehip::fail_alloc.arm(1, 2);
        r.unmap_all();
        knobs_off();
        CHECK(r.tainted && r.on() && r.mapped == 0 && fakehip::live_handles == live.h);
        r.release();   // (nothing mapped: no fence is needed to give the range back)
    }
    CHECK(live.same());
    {   // release() with a failed fence does not free the address range
        VmRange r;
        const char* what = "";
        CHECK(r.reserve(0, 8 * MB) && r.map_to(1, &what) == hipSuccess);
        char* const base = r.base;
        const size_t bytes = r.va_bytes;
        fakehip::fail_alloc.arm(1, 2);
        r.release();
        knobs_off();
        CHECK(!r.on() && fakehip::live_handles == live.h && fakehip::live_ranges == live.r + 1);
        CHECK(hipMemAddressFree(base, bytes) == hipSuccess);   // (the test's own clean-up: the library keeps it for the life of the process)
    }
    CHECK(live.same());
    for (int ncol = 2; ncol <= 3; ncol++) {   // a tainted member of a column set is retired and replaced before the set maps again
        ArenaSets s;
        const char* what = "";
        s.alt.shape(16, 8, ncol == 3 ? 4 : 0);
        CHECK(s.alt.map_target(0, 8 * MB, 1000, &s.retired, &what) == hipSuccess);
        s.alt.clear(&s.retired);
        CHECK(s.retired.empty() && s.alt.col[1].mapped);
        char* const old = s.alt.col[1].vm.base;
        s.alt.col[1].vm.tainted = true;   // (as a failed read-back or a failed unmap inside map_to leaves it)
        CHECK(s.alt.map_target(0, 8 * MB, 1000, &s.retired, &what) == hipSuccess);
        CHECK(s.retired.size() == 1 && s.retired[0].base == old && s.retired[0].mapped == 0);
        CHECK(s.alt.col[1].mapped && s.alt.col[1].vm.base != old && !s.alt.col[1].vm.tainted && s.alt.cap() >= 1000);
        // a set that did not read back: taint(), and clear() retires every member
        s.alt.taint();
        s.alt.clear(&s.retired);
        CHECK((int)s.retired.size() == 1 + ncol && !s.alt.mapped() && !s.alt.col[0].p && s.alt.cap() == 0);
    }
    CHECK(live.same());
}

// ---- row 6: the arena's column sets ----------------------------------------------------------------------------------
void row6_column_sets() {
    for (int ncol = 2; ncol <= 3; ncol++) {
        const size_t e2 = ncol == 3 ? 4 : 0;
        Live live;
        // first start: a failure at any column, reserving or mapping, leaves nothing reserved in any of them
        for (int phase = 0; phase < 2; phase++)
            for (int c = 0; c < ncol; c++) {
                DevColumns s;
                s.shape(16, 8, e2);
                (phase ? fakehip::fail_alloc : fakehip::fail_reserve).arm(c + 1);
                CHECK(!s.start_mapped(0, 8 * MB, 1000));
                knobs_off();
                for (int i = 0; i < DevColumns::NMAX; i++) CHECK(!s.col[i].mapped && !s.col[i].p && !s.col[i].vm.on() && s.col[i].cap == 0);
                CHECK(live.same() && s.cap() == 0);
            }
        {
            DevColumns s;
            Ex ex;
            const char* what = "";
            s.shape(16, 8, e2);
            CHECK(s.start_mapped(0, 8 * MB, 1000) && s.mapped());
            const int64_t cap = s.cap();
            CHECK(cap == (int64_t)(8 * MB / 16));   // the minimum over the columns: the widest entry
            // a growth every column needs, failing at the second: the first keeps its extra mapping, the capacity is the minimum
            const int64_t need = 2200000;
            const size_t c0 = map_rule(8 * MB, (size_t)need * 16, 8 * MB, fakehip::kTotalBytes);
            int64_t least = std::min<int64_t>((int64_t)(c0 / 16), (int64_t)(8 * MB / 8));
            if (ncol == 3) least = std::min<int64_t>(least, (int64_t)(8 * MB / 4));
            fakehip::fail_alloc.arm(2);
            CHECK(s.grow(need, 2 * need, cap, nullptr, ex, &what) == hipErrorOutOfMemory && !strcmp(what, "hipMemCreate"));
            knobs_off();
            CHECK(s.col[0].cap == c0 && c0 > 8 * MB && s.col[1].cap == 8 * MB && s.cap() == least && least < need && s.mapped() && ex.calls == 0);
            CHECK(s.grow(need, 2 * need, cap, nullptr, ex, &what) == hipSuccess && s.cap() >= need && ex.calls == 0 && s.col[0].cap == c0);
            s.release();
        }
        CHECK(live.same());
        {   // the same on the reallocating path
            DevColumns s;
            Ex ex;
            const char* what = "";
            s.shape(16, 8, e2);
            CHECK(s.grow(1000, 1000, 0, nullptr, ex, &what) == hipSuccess && s.cap() == 1000 && !s.mapped());
            for (int i = 0; i < ncol; i++) put(s.col[i].p, 0, 1000 * s.esz[i]);
            fakehip::fail_alloc.arm(2);
            CHECK(s.grow(1001, 2000, 1000, nullptr, ex, &what) == hipErrorOutOfMemory && !strcmp(what, "hipMalloc"));
            knobs_off();
            CHECK(s.col[0].cap == 2000 * 16 && s.col[1].cap == 1000 * 8 && s.cap() == 1000);
            for (int i = 0; i < ncol; i++) CHECK(holds(s.col[i].p, 0, 1000 * s.esz[i]));
        }
        CHECK(live.same());
        {   // current and alternate set: a swap, the readers' pointers, the destructor
            ArenaSets sets;
            Ex ex;
            const char* what = "";
            sets.cur.shape(16, 8, e2);
            sets.alt.shape(16, 8, e2);
            CHECK(sets.cur.start_mapped(0, 8 * MB, 1000));
            uint8_t* d_codes = nullptr;
            int64_t* d_ids = nullptr;
            float* d_sums = nullptr;
            int64_t cap = 0;
            sets.adopt(&d_codes, &d_ids, &d_sums, &cap);
            CHECK((void*)d_codes == sets.cur.col[0].p && (void*)d_ids == sets.cur.col[1].p && cap == sets.cur.cap());
            CHECK(ncol == 3 ? (void*)d_sums == sets.cur.col[2].p : d_sums == nullptr);
            for (int mapped = 1; mapped >= 0; mapped--) {   // a mapped target, then a plain one (after a failed read-back)
                CHECK((mapped ? sets.alt.map_target(0, 8 * MB, 600000, &sets.retired, &what)
                              : sets.alt.alloc_target(600000, nullptr, ex, &sets.retired, &what)) == hipSuccess);
                void* const t0 = sets.alt.col[0].p;
                void* const t1 = sets.alt.col[1].p;
                void* const t2 = sets.alt.col[2].p;
                CHECK(t0 && t1 && (ncol == 3) == (t2 != nullptr) && sets.alt.mapped() == (mapped == 1));
                sets.swap_sets();
                sets.alt.clear(&sets.retired);
                sets.adopt(&d_codes, &d_ids, &d_sums, &cap);
                CHECK((void*)d_codes == t0 && (void*)d_ids == t1 && (void*)d_sums == t2 && cap == sets.cur.cap() && cap >= 600000);
                CHECK(sets.alt.cap() == 0 && sets.cur.mapped() == (mapped == 1));
            }
            CHECK((int)sets.retired.size() == ncol);   // the mapped set that became the alternate one, when it turned plain
            // (the destructor releases both sets and the retired list)
        }
        CHECK(live.same());
    }
}

// ---- row 7: DevBuf ---------------------------------------------------------------------------------------------------
void row7_devbuf() {
    Live live;
    {
        ghi::DevBuf a;
        CHECK(a.ensure(1000) == hipSuccess && a.cap == 1000 + 1000 / 8 + 256 && fakehip::live_allocs == live.a + 1);
        void* const p = a.p;
        CHECK(a.ensure(1000) == hipSuccess && a.p == p);
        ghi::DevBuf b(std::move(a));
        CHECK(!a.p && a.cap == 0 && b.p == p && fakehip::live_allocs == live.a + 1);   // a moved-from buffer owns nothing
        ghi::DevBuf c;
        CHECK(c.ensure(10) == hipSuccess);
        c = std::move(b);   // (what c held is freed)
        CHECK(!b.p && c.p == p && fakehip::live_allocs == live.a + 1);
        std::swap(a, c);
        CHECK(a.p == p && !c.p && fakehip::live_allocs == live.a + 1);
        // over capacity: the old buffer is freed BEFORE the new one is asked for -- a failed allocation leaves none
        fakehip::fail_alloc.arm(1);
        CHECK(a.ensure(100000) == hipErrorOutOfMemory && !a.p && a.cap == 0 && fakehip::live_allocs == live.a);
        knobs_off();
        CHECK(a.ensure(100000) == hipSuccess && a.as<char>() != nullptr);
    }
    CHECK(live.same());   // the destructor frees
}

}  // namespace

int main() {
    row1_realloc_growth();
    row2_mapped_growth();
    row3_realloc_failures();
    row4_mapped_failures();
    row5_fence_failures();
    row6_column_sets();
    row7_devbuf();
    CHECK(fakehip::live_allocs == 0 && fakehip::live_handles == 0 && fakehip::live_ranges == 0 && fakehip::vm.maps.empty());
    printf("dev mem ok\n");
    return 0;
}
