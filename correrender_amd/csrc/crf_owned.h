// crf_owned.h -- move-only owners of the HIP resources a crf_context holds (crf_context.h).  Host only.
// Each releases what it holds when it goes out of scope or is assigned a fresh value; the device it was created on must be
// the current one at that moment (crf_destroy and crf_set_grid bind it first).  Internal to libcorrfield.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace crf {

// `count` elements of T in device memory
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), count_(std::exchange(o.count_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            count_ = std::exchange(o.count_, 0);
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        count_ = 0;
    }
    // grow only: at least `count` elements afterwards.  Growing gives a new allocation (the contents are not kept); on
    // failure the buffer is empty.
    hipError_t reserve(size_t count) {
        if (count <= count_) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else count_ = count;
        return e;
    }
    T* get() const { return p_; }
    size_t count() const { return count_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t count_ = 0;
};

// `count` floats of pinned host memory that the device can address (hipHostMallocMapped)
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept
        : host_(std::exchange(o.host_, nullptr)), device_(std::exchange(o.device_, nullptr)) {}
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            host_ = std::exchange(o.host_, nullptr);
            device_ = std::exchange(o.device_, nullptr);
        }
        return *this;
    }
    ~PinnedBuffer() { reset(); }
    void reset() {
        if (host_) (void)hipHostFree(host_);
        host_ = device_ = nullptr;
    }
    hipError_t allocate(size_t count) {  // once: a buffer that is there stays as it is
        if (host_) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host_), count * sizeof(float), hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&device_), host_, 0);
        if (e != hipSuccess) reset();
        return e;
    }
    float* host() const { return host_; }
    float* device() const { return device_; }  // the same memory as the device addresses it

private:
    float* host_ = nullptr;
    float* device_ = nullptr;
};

// A non-blocking stream or an event, created at first use.  Both convert to the runtime's handle (null: not created).
class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        std::swap(s_, o.s_);
        return *this;
    }
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipError_t create() { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace crf
