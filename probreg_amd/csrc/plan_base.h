// The host side that every opaque handle of the library shares: the checked device selection of an entry point, create,
// destroy, and the copies between a handle's buffers and the caller ("The handle pattern").  Host-compilable against the HIP
// runtime API alone, as dev_buf.h is (tests/host/plan_base_check.cpp runs it against fakes).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <memory>
#include <new>
#include <type_traits>

#include "../../include/probreg_hip.h"
#include "dev_buf.h"

namespace prg {

void set_error(const char* fmt, ...);

#define PRG_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            prg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                           __LINE__);                                                          \
            return PRG_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

#define PRG_REQUIRE(cond, status, ...)                                                         \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            prg::set_error(__VA_ARGS__);                                                       \
            return (status);                                                                   \
        }                                                                                      \
    } while (0)

#define PRG_TRY(expr)                                                                          \
    do {                                                                                       \
        int _s = (expr);                                                                       \
        if (_s != PRG_OK) return _s;                                                           \
    } while (0)

// RAII device selection; constructed by PRG_ENTER only, which tests `ok`.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// The first statement of an entry point after its argument checks: selects `dev` until the enclosing scope ends (every return
// path restores the caller's device) and returns PRG_ERR_HIP, before anything is launched, if it cannot.  PRG_ENTER names the
// enclosing function in the message; a helper that serves several entry points passes the name it was given.
#define PRG_ENTER_AS(who, dev)                                                                 \
    prg::DeviceGuard _prg_guard(dev);                                                          \
    PRG_REQUIRE(_prg_guard.ok, PRG_ERR_HIP, "%s: hipSetDevice(%d) failed", (who), (int)(dev))
#define PRG_ENTER(dev) PRG_ENTER_AS(__func__, dev)

// Where a handle keeps its device and stream: in itself, or in what its ctx() returns (the lattice of prg_ph and prg_filterreg).
template <class H, class = void>
struct HandleCtx {
    static H& of(H& h) { return h; }
};
template <class H>
struct HandleCtx<H, std::void_t<decltype(std::declval<H&>().ctx())>> {
    static auto& of(H& h) { return h.ctx(); }
};

// prg_*_create(out, device, stream): checks, selects the device, constructs the handle, then runs init(handle), which may fail:
// the handle is deleted then (on its device) and *out stays as it was.
template <class H, class Init>
int create_handle(const char* who, H** out, int device, void* hip_stream, Init&& init) {
    PRG_REQUIRE(out != nullptr, PRG_ERR_INVALID, "%s: out is NULL", who);
    int count = 0;
    PRG_HIP(hipGetDeviceCount(&count));
    PRG_REQUIRE(device >= 0 && device < count, PRG_ERR_INVALID, "%s: device %d out of range", who, device);
    PRG_ENTER_AS(who, device);
    std::unique_ptr<H> h(new (std::nothrow) H());
    PRG_REQUIRE(h != nullptr, PRG_ERR_NOMEM, "%s: out of host memory", who);
    auto& ctx = HandleCtx<H>::of(*h);
    ctx.device = device;
    ctx.stream = (hipStream_t)hip_stream;
    PRG_TRY(init(h.get()));
    *out = h.release();
    return PRG_OK;
}
template <class H>
int create_handle(const char* who, H** out, int device, void* hip_stream) {
    return create_handle(who, out, device, hip_stream, [](H*) -> int { return PRG_OK; });
}

// prg_*_destroy(h): NULL is fine; the stream is drained (its result does not matter: the handle goes either way), before_delete
// runs what the members' destructors do not, and the buffers are released on the handle's device.
template <class H, class Pre>
int destroy_handle(H* h, Pre&& before_delete) {
    if (!h) return PRG_OK;
    auto& ctx = HandleCtx<H>::of(*h);
    DeviceGuard guard(ctx.device);  // (unchecked on purpose: a handle whose device cannot be selected is still deleted)
    (void)hipStreamSynchronize(ctx.stream);
    before_delete(h);
    delete h;
    return PRG_OK;
}
template <class H>
int destroy_handle(H* h) {
    return destroy_handle(h, [](H*) {});
}

// The one way results leave a handle: drain the stream, then a blocking copy of elements [first, first + count) of `buf` to the
// host.  An output the entry point documents as optional may be NULL and is skipped.
template <class T>
int copy_out(T* host, const DevBuf<T>& buf, int64_t count, hipStream_t stream, int64_t first = 0) {
    if (!host) return PRG_OK;
    PRG_REQUIRE(first >= 0 && count >= 0 && first + count <= buf.cap, PRG_ERR_STATE,
                "copy_out: %lld elements from %lld of a buffer of %lld", (long long)count, (long long)first, (long long)buf.cap);
    PRG_HIP(hipStreamSynchronize(stream));
    PRG_HIP(hipMemcpy(host, buf.p + first, (size_t)count * sizeof(T), hipMemcpyDeviceToHost));
    return PRG_OK;
}

// ... and its counterpart for `_hd` inputs (host or device memory): the copy is over when this returns, so the caller's memory
// may go and whatever is launched next sees the elements.
template <class T>
int copy_in(DevBuf<T>& buf, const T* src_hd, int64_t count, hipStream_t stream, int64_t first = 0) {
    PRG_REQUIRE(src_hd && first >= 0 && count >= 0 && first + count <= buf.cap, PRG_ERR_STATE,
                "copy_in: %lld elements to %lld of a buffer of %lld", (long long)count, (long long)first, (long long)buf.cap);
    PRG_HIP(hipStreamSynchronize(stream));
    PRG_HIP(hipMemcpy(buf.p + first, src_hd, (size_t)count * sizeof(T), hipMemcpyDefault));
    return PRG_OK;
}

}  // namespace prg
