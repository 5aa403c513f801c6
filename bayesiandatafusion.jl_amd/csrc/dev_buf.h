// dev_buf.h -- the one owner of the library's own device and pinned-host memory, and of its events.  A handle holds its buffers as
// DevBuf members: they free themselves when the handle is deleted, on every error path of the function that builds it included.
// Structs passed to kernels never hold one: they stay plain views filled with get().
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/bdf.h"

void bdf_set_error(const char *fmt, ...);

// blocks and bytes (as requested) currently held by DevBuf objects of this process: bdf_dev_live
inline std::atomic<int64_t> g_dev_live_blocks{0}, g_dev_live_bytes{0};

// the hipHostMalloc flags of the pinned flavour
constexpr unsigned kPinnedDefault = hipHostMallocDefault, kPinnedMapped = hipHostMallocMapped,
                   kPinnedMappedCoherent = hipHostMallocMapped | hipHostMallocCoherent;

template <typename T>
class DevBuf {
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    T *p_ = nullptr;
    size_t bytes_ = 0;
    int host_flags_ = -1;          // >= 0: pinned host memory allocated with these hipHostMalloc flags; -1: device memory
public:
    DevBuf() = default;
    static DevBuf pinned(unsigned flags) { DevBuf b; b.host_flags_ = (int)flags; return b; }
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_), host_flags_(o.host_flags_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; host_flags_ = o.host_flags_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }                // reads as the pointer it owns (a kernel launch still needs get(): no copies)
    explicit operator bool() const { return p_ != nullptr; }
    size_t bytes() const { return bytes_; }
    T *release()
    {
        T *p = p_;
        if (p) { g_dev_live_blocks.fetch_sub(1, std::memory_order_relaxed); g_dev_live_bytes.fetch_sub((int64_t)bytes_, std::memory_order_relaxed); }
        p_ = nullptr; bytes_ = 0;
        return p;
    }
    void reset()
    {
        if (void *p = (void *)release()) { if (host_flags_ >= 0) (void)hipHostFree(p); else (void)hipFree(p); }
    }
    // replaces what is held by a fresh block of exactly `bytes` bytes; empty after a failure
    int alloc_bytes(size_t bytes)
    {
        reset();
        void *p = nullptr;
        const hipError_t e = host_flags_ >= 0 ? hipHostMalloc(&p, bytes, (unsigned)host_flags_) : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            bdf_set_error("%s(%zu bytes) failed: %s (%s:%d)", host_flags_ >= 0 ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e), __FILE__, __LINE__);
            return BDF_ERR_HIP;
        }
        p_ = (T *)p; bytes_ = bytes;
        g_dev_live_blocks.fetch_add(1, std::memory_order_relaxed); g_dev_live_bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed);
        return BDF_OK;
    }
    int alloc(size_t count) { return alloc_bytes(count * kElem); }
    // a device copy of a host vector (at least 16 bytes: an empty vector still gets an address)
    template <typename U>
    int upload(const std::vector<U> &src)
    {
        static_assert(std::is_same<U, std::remove_cv_t<T>>::value, "upload: element types differ");
        if (int rc = alloc_bytes(std::max<size_t>(src.size() * sizeof(U), 16))) return rc;
        if (!src.empty()) {
            const hipError_t e = hipMemcpy((void *)p_, src.data(), src.size() * sizeof(U), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                bdf_set_error("hipMemcpy(%zu bytes) failed: %s (%s:%d)", src.size() * sizeof(U), hipGetErrorString(e), __FILE__, __LINE__);
                reset();
                return BDF_ERR_HIP;
            }
        }
        return BDF_OK;
    }
    // grow on demand: nothing when `bytes` (the caller's own rounding) fit already; else the old block goes -- after the work on
    // `wait_on` that may still read it, where one is given -- and a block of `bytes` takes its place
    int grow(size_t bytes) { return bytes <= bytes_ && p_ ? BDF_OK : alloc_bytes(bytes); }
    int grow(size_t bytes, hipStream_t wait_on)
    {
        if (bytes <= bytes_ && p_) return BDF_OK;
        const hipError_t e = hipStreamSynchronize(wait_on);
        if (e != hipSuccess) {
            bdf_set_error("hipStreamSynchronize failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
            return BDF_ERR_HIP;
        }
        return alloc_bytes(bytes);
    }
};

// an event the library owns; created with the flags its site needs
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags)
    {
        const hipError_t err = hipEventCreateWithFlags(&e, flags);
        if (err != hipSuccess) {
            e = nullptr;
            bdf_set_error("hipEventCreateWithFlags failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
            return BDF_ERR_HIP;
        }
        return BDF_OK;
    }
    operator hipEvent_t() const { return e; }
};
