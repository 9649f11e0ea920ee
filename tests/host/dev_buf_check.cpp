// Host check of probreg_amd/csrc/dev_buf.h against a fake allocator (tests/test_dev_buf_host.py builds this with the host
// compiler under AddressSanitizer / UBSan and runs it; it is not linked against the HIP runtime).  The fakes sit on malloc /
// free, count what is live and fail the k-th allocation on request, so a double free, a leak or a buffer that keeps a freed
// pointer or a stale capacity shows either in the counters or in the sanitizer's report.
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "../../probreg_amd/csrc/dev_buf.h"

static std::set<void*> g_live;
static int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
static int g_fail_in = 0;  // > 0: the g_fail_in-th allocation from now on fails
static size_t g_last_bytes = 0;

static hipError_t fake_alloc(void** p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    ++g_allocs;
    g_last_bytes = bytes;
    return hipSuccess;
}
static hipError_t fake_free(void* p) {
    if (!g_live.erase(p)) {
        ++g_bad_frees;  // not live: a double free or a pointer the allocator never gave out
        return hipErrorInvalidValue;
    }
    ++g_frees;
    free(p);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_alloc(p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
    if (g_fail_in > 0 && --g_fail_in == 0) return hipErrorInvalidValue;
    *dev = host;
    return hipSuccess;
}
}

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

template <class B>
static bool empty(const B& b) { return b.p == nullptr && b.cap == 0; }

int main() {
    using prg::DevBuf;
    using prg::HostBuf;
    {
        DevBuf<double> b;
        CHECK(empty(b));
        // reset allocates exactly `count`
        CHECK(b.reset(100) == hipSuccess && b.p && b.cap == 100 && g_last_bytes == 100 * sizeof(double));
        CHECK(g_live.size() == 1);
        b.p[99] = 1.0;  // (the sanitizer checks the extent)
        // ensure below or at the capacity: no allocation, same pointer
        bool grown = true;
        double* before = b.p;
        int allocs = g_allocs;
        CHECK(b.ensure(100, 400, &grown) == hipSuccess && !grown && b.p == before && b.cap == 100 && g_allocs == allocs);
        CHECK(b.ensure(7, 7) == hipSuccess && b.p == before && g_allocs == allocs);
        // ensure above the capacity: max(need, want), the old block freed exactly once
        int frees = g_frees;
        CHECK(b.ensure(101, 400, &grown) == hipSuccess && grown && b.cap == 400 && g_last_bytes == 400 * sizeof(double));
        CHECK(g_frees == frees + 1 && g_live.size() == 1);
        CHECK(b.ensure(1000, 500, &grown) == hipSuccess && grown && b.cap == 1000);
        CHECK(g_live.size() == 1);
        // a failed ensure: empty, the previous block freed exactly once, nothing live
        frees = g_frees;
        g_fail_in = 1;
        grown = true;
        CHECK(b.ensure(2000, 2000, &grown) == hipErrorOutOfMemory && !grown && empty(b));
        CHECK(g_frees == frees + 1 && g_live.empty() && g_bad_frees == 0);
        // ... and the buffer works again afterwards
        CHECK(b.ensure(10, 10, &grown) == hipSuccess && grown && b.cap == 10 && g_live.size() == 1);
        // a failed reset: the same
        frees = g_frees;
        g_fail_in = 1;
        CHECK(b.reset(50) == hipErrorOutOfMemory && empty(b) && g_frees == frees + 1 && g_live.empty());
        // releasing or failing on an empty buffer frees nothing
        frees = g_frees;
        b.release();
        g_fail_in = 1;
        CHECK(b.reset(50) == hipErrorOutOfMemory && empty(b) && g_frees == frees);
        CHECK(b.reset(0) == hipSuccess && empty(b));
        CHECK(b.reset(3) == hipSuccess && b.cap == 3);
        b.release();
        CHECK(empty(b) && g_live.empty());
        CHECK(b.reset(5) == hipSuccess);
    }  // destruction of a live buffer
    CHECK(g_live.empty() && g_bad_frees == 0);
    {
        // the failure in the middle of a group of buffers that the old code got wrong: the second of three fails
        DevBuf<int> a, b, c;
        CHECK(a.reset(8) == hipSuccess && b.reset(8) == hipSuccess && c.reset(8) == hipSuccess);
        a.release(); b.release(); c.release();
        g_fail_in = 2;
        CHECK(a.reset(16) == hipSuccess && b.reset(16) == hipErrorOutOfMemory);
        CHECK(a.cap == 16 && empty(b) && empty(c) && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
    {
        HostBuf<double> pinned;
        CHECK(pinned.ensure(64, hipHostMallocDefault) == hipSuccess && pinned.p && !pinned.dev);
        CHECK(pinned.p[0] == 0.0 && pinned.p[63] == 0.0);
        double* before = pinned.p;
        int allocs = g_allocs;
        CHECK(pinned.ensure(64, hipHostMallocDefault) == hipSuccess && pinned.p == before && g_allocs == allocs);
        HostBuf<int> mapped;
        g_fail_in = 1;  // the allocation fails
        CHECK(mapped.ensure(8, hipHostMallocMapped) == hipErrorOutOfMemory && !mapped.p && !mapped.dev);
        g_fail_in = 2;  // the allocation succeeds, the device address does not: nothing is kept
        CHECK(mapped.ensure(8, hipHostMallocMapped) != hipSuccess && !mapped.p && !mapped.dev && g_live.size() == 1);
        CHECK(mapped.ensure(8, hipHostMallocMapped) == hipSuccess && mapped.p && mapped.dev == mapped.p);
        CHECK(g_live.size() == 2);
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
    if (g_failed) return 1;
    printf("dev_buf_check ok: %d allocations, %d frees\n", g_allocs, g_frees);
    return 0;
}
