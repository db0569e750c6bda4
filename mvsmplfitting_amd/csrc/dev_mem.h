// Owners of the library's device and pinned-host memory (host only).  Every allocation of a ctx belongs to one of them, so
// that a lifetime ends in one place: a DevPool frees what it handed out when it is released or destroyed, a DevBuf /
// PinnedBuf holds one buffer that only grows.  Both are move-only.  Neither synchronises: a caller that frees memory the
// GPU may still read waits for its stream first.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace mvfit {

// the allocations of one lifetime
class DevPool {
public:
    DevPool() = default;
    DevPool(DevPool&& o) noexcept : ptrs_(std::move(o.ptrs_)) { o.ptrs_.clear(); }
    DevPool& operator=(DevPool&& o) noexcept {
        if (this != &o) { release(); ptrs_ = std::move(o.ptrs_); o.ptrs_.clear(); }
        return *this;
    }
    ~DevPool() { release(); }
    // bytes of device memory, zero-filled on request; *out is null on failure (what was handed out before stays owned)
    template <typename T>
    hipError_t alloc(T** out, size_t bytes, bool zero = false) {
        void* p = nullptr;
        *out = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        ptrs_.push_back(p);
        *out = static_cast<T*>(p);
        return zero ? hipMemset(p, 0, bytes) : hipSuccess;
    }
    void release() {
        for (void* p : ptrs_) (void)hipFree(p);
        ptrs_.clear();
    }

private:
    std::vector<void*> ptrs_;
};

// one buffer that grows to the largest size asked for; Pinned: host memory of hipHostMalloc
template <bool Pinned>
class GrowBuf {
public:
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), size_(std::exchange(o.size_, 0)) {}
    GrowBuf& operator=(GrowBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); size_ = std::exchange(o.size_, 0); }
        return *this;
    }
    ~GrowBuf() { reset(); }
    // large enough: nothing (the address stays).  Else the old buffer is freed BEFORE the new one is allocated (peak memory is
    // the larger of the two, and the contents are lost); on failure the buffer is empty.
    hipError_t reserve(size_t bytes) {
        if (bytes <= size_) return hipSuccess;
        reset();
        const hipError_t e = Pinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else size_ = bytes;
        return e;
    }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        size_ = 0;
    }
    void* get() const { return p_; }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    size_t size() const { return size_; }

private:
    void* p_ = nullptr;
    size_t size_ = 0;
};
using DevBuf = GrowBuf<false>;
using PinnedBuf = GrowBuf<true>;

}  // namespace mvfit
