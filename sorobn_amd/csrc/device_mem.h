// Move-only owners of what the HIP runtime hands out: device buffers, pinned host buffers, events and streams.  Host-only.
// The only file of csrc/ that allocates or frees any of them.  Every operation returns hipError_t (the caller forms the message);
// an empty owner's destructor makes no HIP call, so a context that never touched the runtime never does.  Each owner converts to
// the handle it owns, so that launch code reads like it did with raw pointers.  (Each keeps its handle in a std::unique_ptr with a
// deleter of its own: moves, move assignment over a live owner and the deleted copies are unique_ptr's.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <type_traits>

namespace mibn {

// A device buffer and its capacity in elements.
template <class T>
class DevBuf {
public:
    // room for `need` elements, grown with half as much again of headroom; what the buffer held is not kept
    hipError_t ensure(size_t need) { return need <= cap() ? hipSuccess : reset(need + need / 2 + 1024); }
    // exactly n elements, whatever it held
    hipError_t reset(size_t n) {
        if (hipError_t e = release()) return e;
        void *p = nullptr;
        if (hipError_t e = hipMalloc(&p, n * sizeof(T))) return e;
        p_.reset(static_cast<T *>(p));
        cap_ = n;
        return hipSuccess;
    }
    // frees the buffer now (the owner is empty afterwards, whatever hipFree returned)
    hipError_t release() { T *p = p_.release(); return p ? hipFree(p) : hipSuccess; }
    T *get() const { return p_.get(); }
    operator T *() const { return p_.get(); }
    size_t cap() const { return p_ ? cap_ : 0; }  // (a moved-from buffer has none)

private:
    struct Free { void operator()(T *p) const { (void)hipFree(p); } };
    std::unique_ptr<T, Free> p_;
    size_t cap_ = 0;
};

// A pinned host buffer (sizes in bytes): a pageable source would make hipMemcpyAsync block on its stream.
class PinnedBuf {
public:
    // at least `bytes`, grown with a quarter of headroom; what the buffer held is not kept
    hipError_t ensure(size_t bytes) { return bytes <= cap() ? hipSuccess : reset(bytes + bytes / 4 + 4096); }
    hipError_t reset(size_t bytes) {
        if (hipError_t e = release()) return e;
        void *p = nullptr;
        if (hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault)) return e;
        p_.reset(static_cast<char *>(p));
        cap_ = bytes;
        return hipSuccess;
    }
    hipError_t release() { char *p = p_.release(); return p ? hipHostFree(p) : hipSuccess; }
    // for pinned memory that lives in a plain pointer between two calls (planner.h's ProgBuf::data): take it over / hand it out
    static PinnedBuf adopt(void *p) { PinnedBuf b; b.p_.reset(static_cast<char *>(p)); return b; }
    char *detach() { return p_.release(); }
    char *get() const { return p_.get(); }
    size_t cap() const { return p_ ? cap_ : 0; }

private:
    struct Free { void operator()(char *p) const { (void)hipHostFree(p); } };
    std::unique_ptr<char, Free> p_;
    size_t cap_ = 0;
};

// An event, created on first use: hipEventDefault takes times, hipEventDisableTiming only orders streams.
class Event {
public:
    hipError_t ensure(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) e_.reset(e);
        return r;
    }
    hipError_t release() { hipEvent_t e = e_.release(); return e ? hipEventDestroy(e) : hipSuccess; }
    hipEvent_t get() const { return e_.get(); }
    operator hipEvent_t() const { return e_.get(); }

private:
    struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
    std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> e_;
};

// A stream, created on first use: with flags, or with flags and a priority.
class Stream {
public:
    hipError_t ensure(unsigned flags) { hipStream_t s = nullptr; return s_ ? hipSuccess : keep(hipStreamCreateWithFlags(&s, flags), s); }
    hipError_t ensure(unsigned flags, int priority) { hipStream_t s = nullptr; return s_ ? hipSuccess : keep(hipStreamCreateWithPriority(&s, flags, priority), s); }
    hipError_t release() { hipStream_t s = s_.release(); return s ? hipStreamDestroy(s) : hipSuccess; }
    hipStream_t get() const { return s_.get(); }
    operator hipStream_t() const { return s_.get(); }

private:
    hipError_t keep(hipError_t r, const hipStream_t &s) { if (r == hipSuccess) s_.reset(s); return r; }  // (s is read after the create call wrote it)
    struct Destroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
    std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> s_;
};

}  // namespace mibn
