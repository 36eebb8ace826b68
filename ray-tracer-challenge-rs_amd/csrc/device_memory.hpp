// device_memory.hpp — move-only owners of the host layer's GPU resources:
// DeviceBuffer (device or pinned host memory), Event, Stream.
//
// DeviceBuffer<T, Alloc> itself names no HIP call: Alloc supplies
//   static int allocate(void** p, size_t bytes);  // RT_OK, or the code of an error already recorded
//   static void free(void* p);
// so tests/device_buffer.cpp builds it with g++ against a counting host
// allocator (RTC_DEVICE_MEMORY_NO_HIP leaves out everything below the class).
#pragma once

#include <cstddef>
#include <utility>

namespace rtc {

struct HipDeviceAlloc;

template <typename T, typename Alloc = HipDeviceAlloc>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return n_; }  // elements
    void reset() {
        if (p_) Alloc::free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // Room for n elements.  Nothing happens while capacity() >= n.  Otherwise
    // the old block is freed BEFORE the new one is allocated (the peak is
    // never old + new) and its contents are gone; *grew tells the caller so.
    // A failed allocation leaves the buffer empty and returns Alloc's code.
    int reserve(size_t n, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (n_ >= n) return 0;
        reset();
        if (grew) *grew = true;
        void* p = nullptr;
        if (int rc = Alloc::allocate(&p, n * sizeof(T))) return rc;
        p_ = static_cast<T*>(p);
        n_ = n;
        return 0;
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace rtc

#ifndef RTC_DEVICE_MEMORY_NO_HIP
#include <hip/hip_runtime.h>

#include <string>

#include "rtc_internal.hpp"

namespace rtc {

inline int hip_status(hipError_t e, const char* call) {
    return e == hipSuccess ? RT_OK : set_error(RT_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e));
}

struct HipDeviceAlloc {
    static int allocate(void** p, size_t bytes) { return hip_status(hipMalloc(p, bytes), "hipMalloc"); }
    static void free(void* p) { (void)hipFree(p); }
};
struct HipPinnedAlloc {
    static int allocate(void** p, size_t bytes) { return hip_status(hipHostMalloc(p, bytes), "hipHostMalloc"); }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <typename T>
using PinnedBuffer = DeviceBuffer<T, HipPinnedAlloc>;

// A default-constructed Event or Stream is null and destroys nothing.
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    int create(unsigned flags = hipEventDefault) {  // hipEventDisableTiming for ev_order
        return hip_status(hipEventCreateWithFlags(&e_, flags), "hipEventCreate");
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    int create(unsigned flags) {  // hipStreamNonBlocking for the context stream
        return hip_status(hipStreamCreateWithFlags(&s_, flags), "hipStreamCreateWithFlags");
    }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace rtc
#endif  // RTC_DEVICE_MEMORY_NO_HIP
