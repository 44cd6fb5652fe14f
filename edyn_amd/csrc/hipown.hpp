// Move-only owners of what the HIP runtime hands out - device memory (of one size, or growing), pinned host memory, an event, a stream.
// Each releases what it holds in its destructor, so a function may return from anywhere and a context needs no list of what to free.
// (They release on the device that is current: edynhip_destroy sets the context's device before the context - and with it its owners -
// goes; a multi-device world's free_shard does the same for a shard's.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace eh {

template <typename H, hipError_t (*Release)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset() { if (h) (void)Release(h); h = nullptr; }
    explicit operator bool() const { return h != nullptr; }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    operator hipEvent_t() const { return h; }
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&h, flags); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    operator hipStream_t() const { return h; }
    hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&h, flags); }
};
template <typename T>
struct DeviceBuf : Owned<void *, hipFree> {
    operator T *() const { return (T *)h; }
    hipError_t alloc(size_t count) { reset(); return hipMalloc(&h, count * sizeof(T)); }   // (not cleared)
};
template <typename T>
struct PinnedBuf : Owned<void *, hipHostFree> {
    operator T *() const { return (T *)h; }
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) { reset(); return hipHostMalloc(&h, count * sizeof(T), flags); }
};
// Device memory that only grows, in bytes: by free and allocate, so the contents are not kept; it holds nothing after a failed growth.
struct GrowBuf : Owned<void *, hipFree> {
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(GrowBuf &&o) noexcept : Owned(std::move(o)), cap(o.cap) { o.cap = 0; }
    GrowBuf &operator=(GrowBuf &&o) noexcept { if (this != &o) { Owned::operator=(std::move(o)); cap = o.cap; o.cap = 0; } return *this; }
    void reset() { Owned::reset(); cap = 0; }
    hipError_t grow(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc(&h, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
};

}  // namespace eh
