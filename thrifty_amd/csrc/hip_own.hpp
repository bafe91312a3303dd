// Owning types for what the host side takes from the HIP runtime: device buffers, pinned host buffers,
// streams and events.  Each kind is released in ONE place (detail::drop) and counted there: the number of
// live resources of each kind in the process is what thr_debug_live_resources() reports, so that "the
// handle gives back all it took" is a test and not a hope.  Host only: no kernel, no device function.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace thr {

enum Resource { kDeviceBuf = 0, kPinnedBuf = 1, kStream = 2, kEvent = 3 };
inline std::atomic<int64_t> g_live[4];      // thr_debug_live_resources

namespace detail {
inline hipError_t took(Resource kind, hipError_t e, const void* what) {
    if (e == hipSuccess && what) g_live[kind].fetch_add(1, std::memory_order_relaxed);
    return e;
}
// the only place a resource goes back to the runtime
inline void drop(Resource kind, void* what) {
    if (!what) return;
    switch (kind) {
        case kDeviceBuf: (void)hipFree(what); break;
        case kPinnedBuf: (void)hipHostFree(what); break;
        case kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(what)); break;
        case kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(what)); break;
    }
    g_live[kind].fetch_sub(1, std::memory_order_relaxed);
}
inline hipError_t take(Resource kind, void** p, size_t bytes) {
    const hipError_t e = kind == kDeviceBuf ? hipMalloc(p, bytes) : hipHostMalloc(p, bytes, hipHostMallocDefault);
    return took(kind, e, *p);
}
}  // namespace detail

// untyped device buffer of the post-detect cores (post_stages.hpp)
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        detail::drop(kDeviceBuf, p);
        p = nullptr;
    }
    hipError_t alloc(size_t bytes) {
        release();
        return detail::take(kDeviceBuf, &p, bytes ? bytes : 1);
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Typed array in device (Dev<T>) or pinned host (Pinned<T>) memory that reads as the T* it owns, so a
// launch takes `h->d_stats` as it took the raw pointer.  `bytes` is what was asked for, 0 when empty.
template <class T, Resource Kind>
struct Owned {
    T* p = nullptr;
    size_t bytes = 0;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { release(); }
    operator T*() const { return p; }
    void release() {
        detail::drop(Kind, p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n_bytes) {
        release();
        const hipError_t e = detail::take(Kind, reinterpret_cast<void**>(&p), n_bytes);
        if (e == hipSuccess) bytes = n_bytes;
        return e;
    }
    // at least `need` bytes; a buffer that is too small is replaced (contents lost) by one of need + slack
    hipError_t grow(size_t need, size_t slack = 0) { return bytes >= need ? hipSuccess : alloc(need + slack); }
};
template <class T>
using Dev = Owned<T, kDeviceBuf>;
template <class T>
using Pinned = Owned<T, kPinnedBuf>;

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { detail::drop(kStream, s); }
    operator hipStream_t() const { return s; }
    hipError_t create(unsigned flags) {
        detail::drop(kStream, std::exchange(s, nullptr));
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        return detail::took(kStream, e, s);
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        std::swap(e, o.e);
        return *this;
    }
    ~Event() { detail::drop(kEvent, e); }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags = hipEventDefault) {
        detail::drop(kEvent, std::exchange(e, nullptr));
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        return detail::took(kEvent, rc, e);
    }
};

}  // namespace thr
