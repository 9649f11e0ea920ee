// Host check of probreg_amd/csrc/plan_base.h: the checked device selection of an entry point (PRG_ENTER), the create and
// destroy templates of the handles, and the copies between a handle's buffers and the caller - against fakes of the HIP
// runtime (tests/test_plan_base_host.py builds this with the host compiler under AddressSanitizer / UBSan and runs it; it is
// not linked against the HIP runtime).  The fakes keep a current device, count the stream synchronisations and the copies,
// allocate with malloc and can be told to fail: the device count, the device selection, and a handle's own init step.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>

#include "../../probreg_amd/csrc/plan_base.h"

static std::set<void*> g_live;
static int g_bad_frees = 0;
static int g_current = 0, g_devices = 4, g_set_calls = 0;
static bool g_fail_set = false, g_fail_count = false, g_fail_sync = false;
static int g_syncs = 0, g_copies = 0, g_syncs_at_first_copy = -1;
static size_t g_last_copy_bytes = 0;
static std::string g_error;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_live.erase(p)) {
        ++g_bad_frees;
        return hipErrorInvalidValue;
    }
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
    *dev = host;
    return hipSuccess;
}
hipError_t hipGetDeviceCount(int* count) {
    if (g_fail_count) return hipErrorNoDevice;
    *count = g_devices;
    return hipSuccess;
}
hipError_t hipGetDevice(int* dev) {
    *dev = g_current;
    return hipSuccess;
}
hipError_t hipSetDevice(int dev) {
    ++g_set_calls;
    if (g_fail_set || dev < 0 || dev >= g_devices) return hipErrorInvalidDevice;
    g_current = dev;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_syncs;
    return g_fail_sync ? hipErrorUnknown : hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (g_copies++ == 0) g_syncs_at_first_copy = g_syncs;
    g_last_copy_bytes = bytes;
    memcpy(dst, src, bytes);  // (the sanitizer checks both extents)
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake error"; }
}

namespace prg {
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace prg

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

// a handle that keeps device and stream itself, owns a buffer and counts its constructions
struct Toy {
    static int live, made, gone, device_at_delete;
    int device = -1;
    hipStream_t stream = nullptr;
    prg::DevBuf<double> buf;
    Toy() { ++live, ++made; }
    ~Toy() {
        --live, ++gone;
        device_at_delete = g_current;
    }
};
int Toy::live = 0, Toy::made = 0, Toy::gone = 0, Toy::device_at_delete = -1;

// ... and one that keeps them in a member, as the lattice's owners do
struct Nested {
    struct Ctx {
        int device = -1;
        hipStream_t stream = nullptr;
    } L;
    Ctx& ctx() { return L; }
};

static int g_body_runs = 0, g_device_in_body = -1;
static int toy_entry(int dev, int result) {
    PRG_ENTER(dev);
    ++g_body_runs;
    g_device_in_body = g_current;
    return result;
}

static hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x40);

static void check_create() {
    Toy* const sentinel = reinterpret_cast<Toy*>(0x10);
    // 1. bad arguments: PRG_ERR_INVALID, nothing constructed, *out untouched
    CHECK(prg::create_handle<Toy>("toy_create", nullptr, 0, kStream) == PRG_ERR_INVALID && g_error == "toy_create: out is NULL");
    for (int device : {-1, g_devices}) {
        Toy* out = sentinel;
        CHECK(prg::create_handle("toy_create", &out, device, kStream) == PRG_ERR_INVALID && out == sentinel);
        CHECK(g_error == "toy_create: device " + std::to_string(device) + " out of range");
    }
    g_fail_count = true;
    Toy* out = sentinel;
    CHECK(prg::create_handle("toy_create", &out, 1, kStream) == PRG_ERR_HIP && out == sentinel);
    g_fail_count = false;
    CHECK(Toy::made == 0 && g_set_calls == 0);
    // 2. the device cannot be selected: PRG_ERR_HIP, nothing live
    g_current = 2;
    g_fail_set = true;
    CHECK(prg::create_handle("toy_create", &out, 1, kStream) == PRG_ERR_HIP && out == sentinel);
    CHECK(g_error == "toy_create: hipSetDevice(1) failed");
    g_fail_set = false;
    CHECK(Toy::made == 0 && Toy::live == 0 && g_live.empty() && g_current == 2);
    // 3. the handle's own init fails after it has allocated: its status comes back, one destruction (on the handle's
    //    device), nothing live, *out untouched, the caller's device restored
    int device_in_init = -1;
    CHECK(prg::create_handle("toy_create", &out, 1, kStream, [&](Toy* h) -> int {
              device_in_init = g_current;
              PRG_HIP(h->buf.reset(8));
              return PRG_ERR_STATE;
          }) == PRG_ERR_STATE);
    CHECK(out == sentinel && device_in_init == 1 && Toy::made == 1 && Toy::gone == 1 && Toy::live == 0 && g_live.empty());
    CHECK(Toy::device_at_delete == 1 && g_current == 2 && g_bad_frees == 0);
    // ... and the good path: device and stream set before init runs, the handle released into *out
    CHECK(prg::create_handle("toy_create", &out, 3, kStream, [](Toy* h) -> int {
              CHECK(h->device == 3 && h->stream == kStream && g_current == 3);
              PRG_HIP(h->buf.reset(8));
              return PRG_OK;
          }) == PRG_OK);
    CHECK(out != sentinel && out->device == 3 && out->stream == kStream && out->buf.cap == 8 && Toy::live == 1 && g_current == 2);
    // 4. destroy: NULL is fine; the handle goes on its own device and the caller's comes back; a failing drain still deletes
    CHECK(prg::destroy_handle(static_cast<Toy*>(nullptr)) == PRG_OK);
    int pre_runs = 0;
    const int syncs = g_syncs;
    g_fail_sync = true;
    CHECK(prg::destroy_handle(out, [&](Toy* h) {
              ++pre_runs;
              CHECK(h->buf.p != nullptr && g_current == 3 && g_syncs == syncs + 1);  // before the delete, after the drain
          }) == PRG_OK);
    g_fail_sync = false;
    CHECK(pre_runs == 1 && Toy::live == 0 && Toy::gone == 2 && Toy::device_at_delete == 3 && g_current == 2 && g_live.empty());
    // a handle whose device and stream live in a member
    Nested* n = nullptr;
    CHECK(prg::create_handle("nested_create", &n, 1, kStream) == PRG_OK && n && n->L.device == 1 && n->L.stream == kStream);
    CHECK(prg::destroy_handle(n) == PRG_OK && g_current == 2);
    CHECK(g_bad_frees == 0);
}

// 5. the checked entry
static void check_entry() {
    g_current = 2;
    CHECK(toy_entry(3, PRG_OK) == PRG_OK && g_body_runs == 1 && g_device_in_body == 3 && g_current == 2);
    CHECK(toy_entry(0, PRG_ERR_STATE) == PRG_ERR_STATE && g_body_runs == 2 && g_device_in_body == 0 && g_current == 2);
    const int calls = g_set_calls;
    CHECK(toy_entry(2, PRG_OK) == PRG_OK && g_body_runs == 3 && g_current == 2 && g_set_calls == calls + 1);  // (only the restore)
    g_fail_set = true;
    CHECK(toy_entry(3, PRG_OK) == PRG_ERR_HIP && g_body_runs == 3 && g_current == 2);
    CHECK(g_error == "toy_entry: hipSetDevice(3) failed");
    g_fail_set = false;
    CHECK(toy_entry(7, PRG_OK) == PRG_ERR_HIP && g_body_runs == 3 && g_current == 2);  // no such device
}

// 6. the copies
static void check_copies() {
    prg::DevBuf<double> buf;
    CHECK(buf.reset(10) == hipSuccess);
    for (int i = 0; i < 10; ++i) buf.p[i] = 100.0 + i;
    g_syncs = g_copies = 0;
    g_syncs_at_first_copy = -1;
    CHECK(prg::copy_out(static_cast<double*>(nullptr), buf, 10, kStream) == PRG_OK && g_copies == 0 && g_syncs == 0);  // optional
    double* host = static_cast<double*>(malloc(7 * sizeof(double)));  // exactly count elements: an overrun is the sanitizer's
    CHECK(prg::copy_out(host, buf, 7, kStream) == PRG_OK && g_copies == 1 && g_syncs_at_first_copy == 1);
    CHECK(g_last_copy_bytes == 7 * sizeof(double) && host[0] == 100.0 && host[6] == 106.0);
    CHECK(prg::copy_out(host, buf, 7, kStream, 3) == PRG_OK && host[0] == 103.0 && host[6] == 109.0);
    // more than the buffer holds: refused before anything is copied
    const int copies = g_copies;
    CHECK(prg::copy_out(host, buf, 11, kStream) == PRG_ERR_STATE && g_copies == copies);
    CHECK(prg::copy_out(host, buf, 7, kStream, 4) == PRG_ERR_STATE && g_copies == copies);
    // a failing drain: its status, no copy
    g_fail_sync = true;
    CHECK(prg::copy_out(host, buf, 7, kStream) == PRG_ERR_HIP && g_copies == copies);
    g_fail_sync = false;
    // the way in
    for (int i = 0; i < 7; ++i) host[i] = (double)i;
    const int syncs = g_syncs;
    CHECK(prg::copy_in(buf, host, 7, kStream, 3) == PRG_OK && g_syncs == syncs + 1 && g_last_copy_bytes == 7 * sizeof(double));
    CHECK(buf.p[2] == 102.0 && buf.p[3] == 0.0 && buf.p[9] == 6.0);
    CHECK(prg::copy_in(buf, host, 8, kStream, 3) == PRG_ERR_STATE && prg::copy_in(buf, static_cast<const double*>(nullptr), 1, kStream) == PRG_ERR_STATE);
    free(host);
}

int main() {
    check_create();
    check_entry();
    check_copies();
    CHECK(g_live.empty() && g_bad_frees == 0 && Toy::live == 0);
    if (g_failed) return 1;
    printf("plan_base_check ok: %d handles made, %d destroyed\n", Toy::made, Toy::gone);
    return 0;
}
