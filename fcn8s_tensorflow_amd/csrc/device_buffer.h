// Owners of the host side's HIP allocations (model.hip): a buffer belongs to exactly one Buf, which frees it when it goes out of scope, is
// erased from its map, or is told to.  What is NOT owned stays a raw pointer: views into the arena, sub-pointers of another buffer, memory
// the caller handed in.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace fcn8s {

// device bytes all DeviceBuf of the process hold right now (option "device_bytes_live")
inline std::atomic<long long> g_device_bytes_live{0};

// kPinned: page-locked host memory (hipHostMalloc / hipHostFree) instead of device memory; not counted in g_device_bytes_live
template <class T, bool kPinned = false>
class Buf {
    T* p_ = nullptr;
    size_t bytes_ = 0;
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    ~Buf() { reset(); }

    operator T*() const { return p_; }          // a Buf reads like the pointer it owns
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    size_t elems() const { return bytes_ / sizeof(T); }

    // free now; the caller has made sure nothing in flight still uses the buffer
    void reset()
    {
        if (!p_) return;
        if (kPinned) hipHostFree(p_); else { hipFree(p_); g_device_bytes_live -= (long long)bytes_; }
        p_ = nullptr; bytes_ = 0;
    }
    // At least `bytes` (grown, never shrunk; a regrown buffer keeps nothing of the old one).  A live buffer that is too small is freed behind
    // everything queued on `stream`.  true: the buffer is there.  false: out of memory -- the Buf is empty, the HIP error is cleared, and whether
    // that is an error or a fallback is the caller's business.  *regrown says whether this call allocated (what depends on the old contents is
    // invalidated by the caller), *count is bumped per allocation (the "workspace_allocations" statistic), zero: clear the new buffer on `stream`.
    bool grow(size_t bytes, hipStream_t stream, int64_t* count = nullptr, bool zero = false, bool* regrown = nullptr)
    {
        if (regrown) *regrown = false;
        if (p_ && bytes_ >= bytes) return true;
        if (p_) { hipStreamSynchronize(stream); reset(); }
        const hipError_t e = kPinned ? hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault) : hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return false; }
        bytes_ = bytes;
        if (!kPinned) g_device_bytes_live += (long long)bytes;
        if (count) ++*count;
        if (zero) hipMemsetAsync(p_, 0, bytes, stream);
        if (regrown) *regrown = true;
        return true;
    }
};
template <class T> using DeviceBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

}  // namespace fcn8s
