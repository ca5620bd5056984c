// Binned path, host side: the slot table behind the library's memories of the last builds (build_choice.h: OrderState
// keyed by M, PointsState keyed by (N, M); instantiated in plan.hip, under its one mutex).  16 slots per table, least
// recently used first to go; per slot one pinned buffer and one event.  A build asks for a few words of its workspace
// header to be copied behind it on its own stream (request); a later call of the same (device, key) looks whether the
// copy has landed (poll) and never waits.  Nothing here runs inside a stream capture: the callers see to that.
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
        bool pending = false;          // a copy is on its way
        hipEvent_t ev = nullptr;
        uint32_t* host = nullptr;      // pinned, WORDS words
        uint64_t stamp = 0;
    };
    void (*landed)(Slot&);             // what a completed copy means (host[0 .. WORDS) -> st)
    Slot slots[16];
    uint64_t clock = 0;

    void poll(Slot& s) {
        if (!s.pending) return;
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
        }
        if (!lru->ev && hipEventCreateWithFlags(&lru->ev, hipEventDisableTiming) != hipSuccess) { lru->ev = nullptr; (void)hipGetLastError(); return nullptr; }
        if (!lru->host && hipHostMalloc((void**)&lru->host, WORDS * sizeof(uint32_t), hipHostMallocPortable) != hipSuccess) { lru->host = nullptr; (void)hipGetLastError(); return nullptr; }
        lru->device = device; lru->key = key; lru->st = State{}; lru->pending = false; lru->stamp = ++clock;
        return lru;
    }
    // WORDS words from `src` (device memory) to the slot's pinned buffer, behind what `stream` holds
    void request(Slot& s, const void* src, hipStream_t stream) {
        if (hipMemcpyAsync(s.host, src, WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
            hipEventRecord(s.ev, stream) == hipSuccess)
            s.pending = true;
        (void)hipGetLastError();
    }
};

}  // namespace pigs
