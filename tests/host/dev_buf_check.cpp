// Host check of probreg_amd/csrc/dev_buf.h and cpd_buffers.h (the CPD plan's buffer groups) against a fake allocator (tests/test_dev_buf_host.py builds this with the host
// compiler under AddressSanitizer / UBSan and runs it; it is not linked against the HIP runtime).  The fakes sit on malloc /
// free, count what is live and fail the k-th allocation on request, so a double free, a leak or a buffer that keeps a freed
// pointer or a stale capacity shows either in the counters or in the sanitizer's report.
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "../../probreg_amd/csrc/cpd_buffers.h"
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

static bool source_empty(const prg::SourceBuffers& s) {
    return empty(s.src4) && empty(s.z4) && empty(s.rowacc) && empty(s.zmeta) && empty(s.rorig) && empty(s.zchunk) && s.Mcap == 0;
}
static bool target_empty(const prg::TargetBuffers& t) {
    return empty(t.tgt4) && empty(t.pt1) && empty(t.tmeta) && empty(t.tchunk) && empty(t.corig) && empty(t.colmin) && t.Ncap == 0;
}
static bool queue_empty(const prg::SweepQueue& q) {
    return empty(q.masks) && empty(q.chunk) && empty(q.units) && empty(q.ctrl) && empty(q.ucount) && q.cap_blocks == 0 &&
           q.cap_chunk == 0 && q.cap_units == 0 && q.nblocks == 0 && q.nchunk == 0 && q.cap_soft == 0;
}

// The three all-or-nothing groups of the CPD plan: for every position k of a group's allocations, the k-th one fails on a group
// that already holds buffers of another size.
static void check_groups() {
    const int64_t capA = 19456, capB = 20480;
    for (int k = 1; k <= 6; ++k) {
        prg::SourceBuffers s;
        CHECK(s.size_source(capA) == hipSuccess && s.Mcap == capA && g_live.size() == 6);
        CHECK(s.src4.cap == capA && s.z4.cap == capA && s.rowacc.cap == 4 * capA && s.zmeta.cap == capA / 32 * 8 &&
              s.rorig.cap == capA / 512 + 4 && s.zchunk.cap == capA / 256 * 8);
        const int allocs = g_allocs, frees = g_frees;
        CHECK(s.size_source(capA) == hipSuccess && g_allocs == allocs && g_frees == frees);  // unchanged extents: nothing happens
        g_fail_in = k;
        CHECK(s.size_source(capB) == hipErrorOutOfMemory && source_empty(s));
        CHECK(g_allocs == allocs + k - 1 && g_frees == g_allocs && g_live.empty() && g_bad_frees == 0);
        CHECK(s.size_source(capB) == hipSuccess && s.Mcap == capB && g_live.size() == 6);  // ... and the group works again
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
    for (int k = 1; k <= 6; ++k) {
        prg::TargetBuffers t;
        bool fresh = false;
        CHECK(t.size_target(capA, &fresh) == hipSuccess && fresh && t.Ncap == capA && g_live.size() == 6);
        CHECK(t.tgt4.cap == capA && t.pt1.cap == capA && t.tmeta.cap == capA / 32 * 8 && t.tchunk.cap == capA / 256 * 8 &&
              t.corig.cap == capA / 512 + 4 && t.colmin.cap == capA + capA / 32);
        const int allocs = g_allocs, frees = g_frees;
        CHECK(t.size_target(capA, &fresh) == hipSuccess && !fresh && g_allocs == allocs && g_frees == frees);
        g_fail_in = k;
        fresh = true;
        CHECK(t.size_target(capB, &fresh) == hipErrorOutOfMemory && !fresh && target_empty(t));
        CHECK(g_allocs == allocs + k - 1 && g_frees == g_allocs && g_live.empty() && g_bad_frees == 0);
        CHECK(t.size_target(capB, &fresh) == hipSuccess && fresh && t.Ncap == capB && g_live.size() == 6);
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
    for (int k = 1; k <= 5; ++k) {
        prg::SweepQueue q;
        bool fresh = false;
        CHECK(q.size(10, 3, 500, &fresh) == hipSuccess && fresh && g_live.size() == 5);
        CHECK(q.masks.cap == 10 * 3 * 8 && q.chunk.cap == 10 * 3 && q.units.cap == 500 && q.ctrl.cap == 16 && q.ucount.cap == 500);
        q.nblocks = 10, q.nchunk = 3, q.cap_soft = 100;  // (what a sweep built into it leaves)
        const int allocs = g_allocs, frees = g_frees;
        CHECK(q.size(10, 3, 500, &fresh) == hipSuccess && !fresh && g_allocs == allocs && g_frees == frees);
        CHECK(q.size(4, 1, 20, &fresh) == hipSuccess && !fresh && g_allocs == allocs && q.cap_blocks == 10);  // smaller: kept
        g_fail_in = k;
        fresh = true;
        CHECK(q.size(11, 3, 500, &fresh) == hipErrorOutOfMemory && !fresh && queue_empty(q));
        CHECK(g_allocs == allocs + k - 1 && g_frees == g_allocs && g_live.empty() && g_bad_frees == 0);
    }
    // larger in any ONE of the three extents: all five arrays are new, at the extents asked for, and the caller is told
    const int64_t grow[3][3] = {{11, 3, 500}, {10, 4, 500}, {10, 3, 501}};
    for (const auto& g : grow) {
        prg::SweepQueue q;
        bool fresh = false;
        CHECK(q.size(10, 3, 500, &fresh) == hipSuccess && fresh);
        const int allocs = g_allocs, frees = g_frees;
        CHECK(q.size(g[0], (int)g[1], g[2], &fresh) == hipSuccess && fresh && g_allocs == allocs + 5 && g_frees == frees + 5);
        CHECK(q.cap_blocks == g[0] && q.cap_chunk == g[1] && q.cap_units == g[2] && q.masks.cap == g[0] * g[1] * 8 &&
              q.chunk.cap == g[0] * g[1] && q.units.cap == g[2] && q.ucount.cap == g[2] && g_live.size() == 5);
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
}

// reset_group (dev_buf.h): buffers of different element types that are sized together.  For every position k of the failing
// allocation, on a group that already holds blocks of another size: the first error comes back, every buffer is empty, the old
// blocks were freed exactly once, nothing is live - and the same call succeeds afterwards.
static void check_reset_group() {
    using prg::DevBuf;
    for (int k = 1; k <= 4; ++k) {
        DevBuf<double> a;
        DevBuf<int> b;
        DevBuf<float4> c;
        DevBuf<char> d;
        CHECK(prg::reset_group(a, 10, b, 20, c, 30, d, 40) == hipSuccess && g_live.size() == 4 && g_last_bytes == 40);
        CHECK(a.p && b.p && c.p && d.p && a.cap == 10 && b.cap == 20 && c.cap == 30 && d.cap == 40);
        a.p[9] = 1.0, b.p[19] = 1, c.p[29].w = 1.f, d.p[39] = 1;  // (the sanitizer checks the extents)
        const int allocs = g_allocs, frees = g_frees;
        g_fail_in = k;
        CHECK(prg::reset_group(a, 11, b, 21, c, 31, d, 41) == hipErrorOutOfMemory);
        CHECK(empty(a) && empty(b) && empty(c) && empty(d));
        // the four old blocks and the k - 1 new ones, each freed once
        CHECK(g_allocs == allocs + k - 1 && g_frees == frees + 4 + k - 1 && g_live.empty() && g_bad_frees == 0);
        CHECK(prg::reset_group(a, 11, b, 21, c, 31, d, 41) == hipSuccess && g_live.size() == 4);
        CHECK(a.cap == 11 && b.cap == 21 && c.cap == 31 && d.cap == 41 && g_last_bytes == 41);
        c.p[30].x = 1.f;
    }
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
    {
        // a count of 0 inside a group: that buffer is empty, which is no failure, and allocates nothing
        DevBuf<double> a;
        DevBuf<int> b;
        DevBuf<float4> c;
        CHECK(prg::reset_group(a, 5, b, 5, c, 5) == hipSuccess && g_live.size() == 3);
        const int allocs = g_allocs;
        CHECK(prg::reset_group(a, 7, b, 0, c, 9) == hipSuccess && a.cap == 7 && empty(b) && c.cap == 9);
        CHECK(g_allocs == allocs + 2 && g_live.size() == 2);
        g_fail_in = 2;  // c's allocation, the second one
        CHECK(prg::reset_group(a, 8, b, 0, c, 10) == hipErrorOutOfMemory && empty(a) && empty(b) && empty(c) && g_live.empty());
        CHECK(prg::reset_group(a, 8, b, 0, c, 10) == hipSuccess && a.cap == 8 && empty(b) && c.cap == 10 && g_live.size() == 2);
        prg::release_all(a, b, c);
        CHECK(empty(a) && empty(b) && empty(c) && g_live.empty());
    }
    CHECK(g_bad_frees == 0 && g_allocs == g_frees);
}

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
        // swap: a finished local buffer goes to its (empty) owner, the local leaves with nothing to free
        DevBuf<double> owner;
        {
            DevBuf<double> local;
            CHECK(local.reset(12) == hipSuccess);
            double* const block = local.p;
            owner.swap(local);
            CHECK(owner.p == block && owner.cap == 12 && empty(local));
        }
        CHECK(g_live.size() == 1 && owner.cap == 12);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
    check_groups();
    check_reset_group();
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
