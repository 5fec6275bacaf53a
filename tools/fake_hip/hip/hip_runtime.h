// A stand-in for <hip/hip_runtime.h> that covers what sorobn_amd/csrc/device_mem.h calls, for tools/device_mem_sim.cpp only (a host
// program: no GPU, no ROCm).  Every handle is backed by malloc and keeps its address until fake_hip::reset(), so a handle is never
// handed out twice and the ledger can say how often each one was created and released.  fail_at = N makes the N-th creating call
// (counted from 1 since the last reset) fail without creating anything.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <map>

typedef enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct fake_hip_event *hipEvent_t;
typedef struct fake_hip_stream *hipStream_t;
enum : unsigned { hipEventDefault = 0x0, hipEventDisableTiming = 0x2, hipHostMallocDefault = 0x0, hipStreamNonBlocking = 0x1 };

namespace fake_hip {
enum Kind { kDevice, kPinned, kEvent, kStream };
struct Handle {
    Kind kind;
    size_t bytes;     // device / pinned
    unsigned flags;   // pinned / event / stream
    int priority;     // stream (0 without)
    int created, released;
};
struct Ledger {
    std::map<void *, Handle> handles;  // every handle since the last reset, live or not
    long calls = 0;                    // backend calls of any kind
    long creates = 0;                  // creating calls, failed ones included
    long fail_at = 0;                  // 0: none
    long unknown_releases = 0;         // releases of something that was never handed out
};
inline Ledger &ledger() { static Ledger L; return L; }
inline void reset() {
    Ledger &L = ledger();
    for (auto &kv : L.handles) std::free(kv.first);
    L = Ledger{};
}
inline hipError_t create(void **out, Kind kind, size_t bytes, unsigned flags, int priority) {
    Ledger &L = ledger();
    ++L.calls;
    *out = nullptr;
    if (++L.creates == L.fail_at) return hipErrorOutOfMemory;
    void *p = std::malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    L.handles[p] = Handle{kind, bytes, flags, priority, 1, 0};
    *out = p;
    return hipSuccess;
}
inline hipError_t release(void *p, Kind kind) {
    Ledger &L = ledger();
    ++L.calls;
    if (!p) return hipSuccess;  // (hipFree(nullptr) is allowed; the owners never do it)
    auto it = L.handles.find(p);
    if (it == L.handles.end() || it->second.kind != kind) { ++L.unknown_releases; return hipErrorInvalidValue; }
    ++it->second.released;
    return hipSuccess;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void **p, size_t bytes) { return fake_hip::create(p, fake_hip::kDevice, bytes, 0, 0); }
inline hipError_t hipFree(void *p) { return fake_hip::release(p, fake_hip::kDevice); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { return fake_hip::create(p, fake_hip::kPinned, bytes, flags, 0); }
inline hipError_t hipHostFree(void *p) { return fake_hip::release(p, fake_hip::kPinned); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { return fake_hip::create((void **)e, fake_hip::kEvent, 0, flags, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::release(e, fake_hip::kEvent); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { return fake_hip::create((void **)s, fake_hip::kStream, 0, flags, 0); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority) { return fake_hip::create((void **)s, fake_hip::kStream, 0, flags, priority); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::release(s, fake_hip::kStream); }
