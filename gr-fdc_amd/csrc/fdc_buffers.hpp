// Owning device and pinned-host buffers: a pointer, a capacity in elements, freed by the destructor.  Move-only.
//   alloc(n)                 a fixed table: max(16, n * sizeof(T)) bytes
//   reserve(need, grow_to)   a buffer that follows the demand: nothing when need <= capacity, otherwise the old block goes FIRST
//                            (pointer null, capacity 0) and grow_to elements are allocated — a failed allocation leaves an empty
//                            buffer behind, never a dangling pointer with a capacity.  The caller names the new size (its growth rule).
//   upload(vec)              DevBuf: alloc(vec.size()) and a blocking copy of the vector
// The conversion to T * lets a buffer stand where the raw pointer stood (kernel launches, copies, pointer arithmetic).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace fdc {

struct DevMem {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { (void)hipFree(p); }
};
struct PinMem {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { (void)hipHostFree(p); }
};
struct MappedMem {                       // pinned AND mapped into the device's address space (hipHostGetDevicePointer): kernels read it in place
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped); }
    static void put(void *p) { (void)hipHostFree(p); }
};

template <typename T, typename Mem>
class Buf {
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf &operator=(Buf &&o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~Buf() { release(); }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void release() { if (p_) Mem::put(p_); p_ = nullptr; cap_ = 0; }
    hipError_t alloc(size_t n) { return grab(n, std::max<size_t>(16, n * sizeof(T))); }
    hipError_t reserve(size_t need, size_t grow_to) { return need <= cap_ ? hipSuccess : grab(grow_to, grow_to * sizeof(T)); }
protected:
    hipError_t grab(size_t n, size_t bytes)
    {
        release();
        const hipError_t e = Mem::get(reinterpret_cast<void **>(&p_), bytes);
        if (e == hipSuccess) cap_ = n; else p_ = nullptr;
        return e;
    }
    T *p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T>
struct DevBuf : Buf<T, DevMem> {
    hipError_t upload(const std::vector<T> &v)
    {
        const hipError_t e = this->alloc(v.size());
        return e != hipSuccess ? e : hipMemcpy(this->p_, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    }
};
template <typename T>
using PinBuf = Buf<T, PinMem>;
template <typename T>
using MappedBuf = Buf<T, MappedMem>;

}  // namespace fdc
