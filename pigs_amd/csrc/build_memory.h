// Binned path, host side: the slot table behind the library's memories of the last builds (build_choice.h: OrderState
// keyed by M, PointsState keyed by (N, M); instantiated in plan.hip, under its one mutex).  16 slots per table, least
// recently used first to go; per slot one pinned buffer, mapped into the device's address space, and one event.  A build
// first reserves its slot (reserve), then sends a few words home behind itself on its own stream: either its last
// kernel stores them into the slot's buffer where they come into being (home, then sent -- no launch of its own), or
// they are copied out of its workspace header (request -- a blit kernel in the build's stream); a later call of the
// same (device, key) looks whether they have landed (poll) and never waits.  Nothing here runs inside a stream capture:
// the callers see to that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pigs {

inline bool current_device(int* dev) {
    if (hipGetDevice(dev) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
inline bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// Key: operator==.  State: default-constructed for a new (device, key).  WORDS: 32-bit words of a copy.
template <class Key, class State, uint32_t WORDS>
struct BuildMemory {
    struct Slot {
        int device = -1;
        Key key{};
        State st{};
        bool pending = false;          // words are on their way (or about to be: reserved)
        bool recorded = false;         // ... and `ev` has been recorded behind them (poll looks at no other event)
        hipEvent_t ev = nullptr;
        uint32_t* host = nullptr;      // pinned and mapped, WORDS words; lives as long as the process
        uint32_t* dev = nullptr;       // the same words as the slot's device addresses them
        uint64_t stamp = 0;
    };
    void (*landed)(Slot&);             // what a completed copy means (host[0 .. WORDS) -> st)
    Slot slots[16];
    uint64_t clock = 0;

    void poll(Slot& s) {
        if (!s.pending || !s.recorded) return;
        const hipError_t q = hipEventQuery(s.ev);
        (void)hipGetLastError();          // hipErrorNotReady is an answer, not a failure
        if (q != hipSuccess) return;
        s.pending = false;
        landed(s);
    }
    Slot* peek(int device, const Key& key) {      // (no use counted)
        for (auto& s : slots)
            if (s.device == device && s.key == key) return &s;
        return nullptr;
    }
    // create: a new (device, key) takes the least recently used slot that waits for no copy
    Slot* find(int device, const Key& key, bool create = false) {
        Slot* lru = nullptr;
        for (auto& s : slots) {
            if (s.device == device && s.key == key) { s.stamp = ++clock; return &s; }
            if (!s.pending && (!lru || s.stamp < lru->stamp)) lru = &s;
        }
        if (!create) return nullptr;
        if (!lru) {
            // every slot waits for a copy (sizes that were built once and never came back): the copies have long
            // landed -- take note of them and give the least recently used slot away
            for (auto& s : slots) {
                poll(s);
                if (!s.pending && (!lru || s.stamp < lru->stamp)) lru = &s;
            }
            if (!lru) return nullptr;
        }
        if (lru->ev && lru->device != device) {      // an event belongs to the device it was created on
            (void)hipEventDestroy(lru->ev);
            lru->ev = nullptr;
            lru->dev = nullptr;
        }
        if (!lru->ev && hipEventCreateWithFlags(&lru->ev, hipEventDisableTiming) != hipSuccess) { lru->ev = nullptr; (void)hipGetLastError(); return nullptr; }
        if (!lru->host && hipHostMalloc((void**)&lru->host, WORDS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { lru->host = nullptr; (void)hipGetLastError(); return nullptr; }
        if (!lru->dev && hipHostGetDevicePointer((void**)&lru->dev, lru->host, 0) != hipSuccess) { lru->dev = nullptr; (void)hipGetLastError(); return nullptr; }
        lru->device = device; lru->key = key; lru->st = State{}; lru->pending = lru->recorded = false; lru->stamp = ++clock;
        return lru;
    }
    // The slot is this build's from here on: no other build sends words to it, nobody gives it away, and poll leaves it
    // alone until request or sent has recorded the event (release: the build failed to launch).
    void reserve(Slot& s) { s.pending = true; s.recorded = false; }
    void release(Slot& s) { s.pending = false; s.recorded = false; }
    // A reserved slot's words zeroed by the host (nothing on the device can be writing them: the slot was not pending)
    // and its device address, for the kernel that stores the words that are not zero.
    uint32_t* home(Slot& s) {
        for (uint32_t k = 0; k < WORDS; ++k) s.host[k] = 0u;
        return s.dev;
    }
    // ... behind that kernel's launch on `stream`
    void sent(Slot& s, hipStream_t stream) {
        s.recorded = hipEventRecord(s.ev, stream) == hipSuccess;
        if (!s.recorded) s.pending = false;
        (void)hipGetLastError();
    }
    // WORDS words from `src` (device memory) to the slot's pinned buffer, behind what `stream` holds
    void request(Slot& s, const void* src, hipStream_t stream) {
        s.pending = s.recorded = hipMemcpyAsync(s.host, src, WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                                 hipEventRecord(s.ev, stream) == hipSuccess;
        (void)hipGetLastError();
    }
};

}  // namespace pigs
