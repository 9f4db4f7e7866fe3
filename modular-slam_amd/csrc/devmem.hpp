// devmem.hpp — who owns device and page-locked memory: DevBuf<T> (one hipMalloc block) and PinnedBuf<T> (one hipHostMalloc
// block), both move-only, and the two ways a block grows.  Everything else (kernel argument structs, QuadArgs, views
// handed through the C ABI) holds plain pointers INTO these blocks and frees nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <utility>

namespace mslam
{
template <typename T>
class DevBuf
{
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~DevBuf() { reset(); }
    // frees what it holds, then max(n, 1) elements; empty on failure
    hipError_t alloc(size_t n)
    {
        reset();
        n = std::max<size_t>(n, 1);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
        if(e == hipSuccess)
            n_ = n;
        else
            p_ = nullptr;
        return e;
    }
    void reset()
    {
        if(p_)
            (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; } // elements
};

// The same over page-locked host memory; get() is the host address, dev() the device's address of a mapped block
// (nullptr for one allocated with mapped = false: plain staging for copies).
template <typename T>
class PinnedBuf
{
    T *p_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;
    bool mapped_;

public:
    explicit PinnedBuf(bool mapped = true) : mapped_(mapped) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t n)
    {
        reset();
        n = std::max<size_t>(n, 1);
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), mapped_ ? hipHostMallocMapped : hipHostMallocDefault);
        if(e != hipSuccess)
        {
            p_ = nullptr;
            return e;
        }
        n_ = n;
        if(mapped_ && (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_), p_, 0)) != hipSuccess)
            reset();
        return e;
    }
    void reset()
    {
        if(p_)
            (void)hipHostFree(p_);
        p_ = dev_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* dev() const { return dev_; }
    size_t size() const { return n_; }
};

// Grow, contents not kept: nothing when n <= size(); otherwise waits for `s` (whatever reads the old block has finished
// before it is freed) and reallocates.
template <typename Buf>
hipError_t grow(Buf& b, size_t n, hipStream_t s)
{
    if(n <= b.size())
        return hipSuccess;
    const hipError_t e = hipStreamSynchronize(s);
    return e != hipSuccess ? e : b.alloc(n);
}

// Grow, live prefix kept, first half: `fresh` becomes a block of n elements (zeroed first when asked) with the first old_n
// elements of `b` copied across, all enqueued on `s`.  The caller waits for `s` and move-assigns fresh to b — several
// blocks that must grow together share one wait, and a failure before the swap leaves every one of them as it was.
template <typename T>
hipError_t grown_copy(DevBuf<T>& fresh, const DevBuf<T>& b, size_t n, size_t old_n, bool zero, hipStream_t s)
{
    hipError_t e = fresh.alloc(n);
    if(e == hipSuccess && zero)
        e = hipMemsetAsync(fresh, 0, n * sizeof(T), s);
    if(e == hipSuccess && old_n && b)
        e = hipMemcpyAsync(fresh, b, old_n * sizeof(T), hipMemcpyDeviceToDevice, s);
    return e;
}
} // namespace mslam
