// call_slots.cpp -- the pool behind call_slots.h: a free list under its own mutex, a slot created only when the list is empty.
#include "call_slots.h"

namespace ghi {

hipError_t CallSlots::take(CallSlot** out) {
    *out = nullptr;
    CallSlot* s = nullptr;
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!free_.empty()) {
            s = free_.back();
            free_.pop_back();
        }
    }
    if (!s) {
        // built in full before the pool hears of it: a failure leaves the pool as it was
        hipEvent_t ev = nullptr;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        int* over = nullptr;
        e = hipHostMalloc((void**)&over, sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipEventDestroy(ev);
            return e;
        }
        s = new CallSlot();
        s->ev = ev, s->over = over;
        std::lock_guard<std::mutex> g(mu_);
        all_.push_back(s);
    }
    // (nobody waits on this slot and no copy into its word is in flight: its last owner read the word before giving it back)
    *s->over = 0;
    *out = s;
    return hipSuccess;
}

void CallSlots::give_back(CallSlot* s) {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(s);
}

size_t CallSlots::slots() {
    std::lock_guard<std::mutex> g(mu_);
    return all_.size();
}

size_t CallSlots::busy() {
    std::lock_guard<std::mutex> g(mu_);
    return all_.size() - free_.size();
}

void CallSlots::release() {
    std::lock_guard<std::mutex> g(mu_);
    for (CallSlot* s : all_) {
        (void)hipEventDestroy(s->ev);
        (void)hipHostFree(s->over);
        delete s;
    }
    all_.clear();
    free_.clear();
}

}  // namespace ghi
