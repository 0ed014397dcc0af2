// call_slots.h -- what a call of a _wait entry (gamma_hip_ivfpq_search_device_wait, gamma_hip_flat_search_device_wait) owns
// while its caller waits for it with the handle already free: a completion event and a pinned word (the flat call's "did a
// survivor list overflow").  Host code over the HIP runtime API alone: no kernels, nothing of the handle --
// tests/sanitize/call_slots_check.cc runs it against a stand-in runtime whose streams defer.
//
// The rule: a call owns its slot from take() -- under the search lock -- until its waiter gives it back, which needs no lock
// but the pool's own.  No later call arms the slot's event or writes its word before then, so any number of callers may
// overlap.  A slot is created only when none is free.  The bound: slots() never exceeds the largest number of calls that
// were between take() and give_back() at one time -- W callers settle at W slots, however many calls they make.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>
#include <vector>

namespace ghi {

struct CallSlot {
    hipEvent_t ev = nullptr;   // behind everything of the call that owns the slot, once armed
    int* over = nullptr;       // pinned; zero from take() on, until the call's own copy lands
};

class CallSlots {
  public:
    CallSlots() = default;
    CallSlots(const CallSlots&) = delete;
    CallSlots& operator=(const CallSlots&) = delete;
    ~CallSlots() { release(); }

    // a slot of the caller's own, its word zero.  On an error nothing is taken and nothing is left behind.
    hipError_t take(CallSlot** out);
    // the slot's event behind what stream `s` holds now: the call's last enqueue
    static hipError_t arm(CallSlot* s, hipStream_t st) { return hipEventRecord(s->ev, st); }
    // until the armed event has completed (a slot that was never armed does not wait)
    static hipError_t wait(CallSlot* s) { return hipEventSynchronize(s->ev); }
    // the word: the owner's after wait()
    static int word(const CallSlot* s) { return *static_cast<const volatile int*>(s->over); }
    // the slot goes to the next call; from any thread, without the search lock
    void give_back(CallSlot* s);

    size_t slots();   // created so far
    size_t busy();    // taken and not yet given back
    // destroys every event and frees every word (the device current, nobody waiting any more)
    void release();

  private:
    std::mutex mu_;
    std::vector<CallSlot*> all_, free_;   // every slot created / those that no call owns
};

// The slot of one call of a _wait entry: given back when the call leaves the entry, on whichever path.
class CallTicket {
  public:
    explicit CallTicket(CallSlots& pool) : pool_(pool) {}
    CallTicket(const CallTicket&) = delete;
    CallTicket& operator=(const CallTicket&) = delete;
    ~CallTicket() { done(); }
    hipError_t take() { return pool_.take(&s_); }
    CallSlot* slot() const { return s_; }
    void done() {
        if (s_) pool_.give_back(s_);
        s_ = nullptr;
    }

  private:
    CallSlots& pool_;
    CallSlot* s_ = nullptr;
};

}  // namespace ghi
