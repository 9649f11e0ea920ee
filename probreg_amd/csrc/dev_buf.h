// Owning buffers of the handles: one pointer, one capacity, never apart.  `p == nullptr <=> cap == 0` holds after every
// call, failed ones included - a failed allocation leaves the buffer EMPTY, never a freed pointer or a stale capacity that a
// later launch would trust.  The owner still decides when a buffer is re-created and how large (hipFree drains the device,
// so the growth policies stay at the call sites); all calls return hipError_t, so call sites read PRG_HIP(buf.ensure(..)).
// Host-compilable: depends on the HIP runtime API only (tests/host/dev_buf_check.cpp runs it against a fake allocator).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

namespace prg {

template <class T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;  // elements

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // free, then allocate exactly `count` elements (the old contents are gone either way)
    hipError_t reset(int64_t count) {
        release();
        if (count <= 0) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (size_t)count * sizeof(T));
        if (e != hipSuccess || !q) return e != hipSuccess ? e : hipErrorOutOfMemory;
        p = static_cast<T*>(q);
        cap = count;
        return hipSuccess;
    }
    // exchange the blocks of two buffers (a finished local buffer is handed to its owner this way; the other goes with the local)
    void swap(DevBuf& o) {
        T* const q = p; p = o.p; o.p = q;
        const int64_t c = cap; cap = o.cap; o.cap = c;
    }
    // cap >= need: nothing happens; else reset(max(need, want)).  *grown: the buffer was re-created (contents undefined)
    hipError_t ensure(int64_t need, int64_t want, bool* grown = nullptr) {
        if (grown) *grown = false;
        if (cap >= need) return hipSuccess;
        const hipError_t e = reset(need > want ? need : want);
        if (grown) *grown = e == hipSuccess;
        return e;
    }
};

// Buffers that are sized together, of any element types: reset_group(a, na, b, nb, ...) releases all of them, then allocates
// them in the order given, each exactly its count.  All-or-nothing: the first error is returned and EVERY listed buffer is
// empty then, so one pointer of a group answers for the rest.  The owner writes whatever describes the group (a point count, a
// capacity, "have" flags) after it has succeeded, and clears it otherwise.  release_all(a, b, ...) is the one way to drop
// several buffers at once (a later step of the owner failed).
template <class... Bufs>
void release_all(Bufs&... bufs) {
    (bufs.release(), ...);
}
namespace detail {  // the two passes of reset_group over its (buffer, count) pairs
inline void release_pairs() {}
template <class T, class... Rest>
void release_pairs(DevBuf<T>& b, int64_t, Rest&&... rest) {
    b.release();
    release_pairs(rest...);
}
inline hipError_t reset_pairs() { return hipSuccess; }
template <class T, class... Rest>
hipError_t reset_pairs(DevBuf<T>& b, int64_t count, Rest&&... rest) {
    hipError_t e = b.reset(count);
    if (e == hipSuccess) e = reset_pairs(rest...);
    if (e != hipSuccess) b.release();
    return e;
}
}  // namespace detail
template <class... Pairs>
hipError_t reset_group(Pairs&&... pairs) {
    detail::release_pairs(pairs...);
    return detail::reset_pairs(pairs...);
}

// Pinned host memory, allocated once and zero-filled; with hipHostMallocMapped in `flags`, `dev` is the address the device
// reaches it by.
template <class T>
struct HostBuf {
    T* p = nullptr;
    T* dev = nullptr;

    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }

    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        dev = nullptr;
    }
    hipError_t ensure(int64_t count, unsigned flags = hipHostMallocDefault) {
        if (p) return hipSuccess;
        void* q = nullptr;
        hipError_t e = hipHostMalloc(&q, (size_t)count * sizeof(T), flags);
        if (e != hipSuccess || !q) return e != hipSuccess ? e : hipErrorOutOfMemory;
        p = static_cast<T*>(q);
        memset(q, 0, (size_t)count * sizeof(T));
        if (flags & hipHostMallocMapped) {
            void* d = nullptr;
            e = hipHostGetDevicePointer(&d, q, 0);
            if (e != hipSuccess) {
                release();
                return e;
            }
            dev = static_cast<T*>(d);
        }
        return hipSuccess;
    }
};

}  // namespace prg
