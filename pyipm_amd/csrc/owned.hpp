// owned.hpp -- one owner per device resource of a handle: device and pinned-host buffers, events, streams.  Move-only; each
// releases what it holds in its destructor, so a handle is torn down by `delete` and an error path by leaving the scope.
// These are the only places of the library that create or release a HIP resource.  A conversion to the raw handle lets an
// owner stand wherever HIP or a kernel launch takes one; views into a buffer (WT into JT, the carved workspace) stay plain pointers.
//
// The rule for a free: hipFree waits for the whole device before it releases the memory, so no owner synchronises a stream
// in front of it -- whatever still reads the old storage, on any stream, is done when the memory goes.  Only a Stream
// synchronises explicitly (hipStreamDestroy returns at once and lets the stream drain behind it: a failure of that work
// would be reported to nobody).  A handle's teardown synchronises its streams up front all the same, so the order in
// which its members are destroyed does not matter.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>
#include <vector>

namespace pyipm {

// Device (Pinned = false) or pinned host memory: pointer + capacity in elements.
template <class T, bool Pinned = false>
class Buf {
    T* p_ = nullptr; size_t cap_ = 0; bool own_ = true; unsigned flags_ = 0;
public:
    Buf() = default;
    explicit Buf(unsigned host_flags) : flags_(host_flags) {}         // pinned: the hipHostMalloc flags of every allocation
    Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept { swap(o); }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~Buf() { reset(); }
    void swap(Buf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); std::swap(own_, o.own_); std::swap(flags_, o.flags_); }
    void reset() {
        if (p_ && own_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; cap_ = 0; own_ = true;
    }
    // Room for `count` elements.  Grows by free-then-allocate: the contents are NOT kept.  On failure the buffer is empty.
    hipError_t reserve(size_t count) {
        if (count <= cap_) return hipSuccess;
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, count * sizeof(T), flags_) : hipMalloc((void**)&p_, count * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = count;
        return hipSuccess;
    }
    void adopt(T* p, size_t count) { reset(); p_ = p; cap_ = count; own_ = false; }   // caller-supplied memory: used, never freed
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    operator T*() const { return p_; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// An event, created on first ensure() with the flags given there (hipEventDefault: a timing event).
class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~Event() { reset(); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipError_t ensure(unsigned flags) {
        if (e_) return hipSuccess;
        const hipError_t e = flags == hipEventDefault ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    operator hipEvent_t() const { return e_; }
};
// at least `n` events in `v`, the new ones created with `flags`
inline hipError_t ensure_events(std::vector<Event>& v, size_t n, unsigned flags) {
    while (v.size() < n) {
        Event e;
        const hipError_t rc = e.ensure(flags); if (rc != hipSuccess) return rc;
        v.push_back(std::move(e));
    }
    return hipSuccess;
}

// A stream, created on first ensure().  The destructor synchronises, then destroys.
class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    void reset() { if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); } s_ = nullptr; }
    hipError_t ensure(unsigned flags) {                  // default priority
        if (s_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    hipError_t ensure_highest(unsigned flags) {          // the top of the device's priority range
        if (s_) return hipSuccess;
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&s_, flags, hi);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    void sync() const { if (s_) (void)hipStreamSynchronize(s_); }
    operator hipStream_t() const { return s_; }
};

}  // namespace pyipm
