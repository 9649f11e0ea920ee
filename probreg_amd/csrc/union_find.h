// A union-find that never waits: `parent` is an int array over vertices that is only ever lowered, by 32-bit
// atomic minimum and compare-and-swap.  The invariant is parent[x] <= x, and every value ever stored in parent[x] is a vertex
// of x's component.  A larger root is always hooked under a smaller vertex, so when all unions are done the root of a
// component is its smallest vertex, whatever the schedule was.
//
// Templated on the atomic primitive, so that the host compiles it too (tests/host/union_find_check.cpp drives it with a plain
// array and with std::atomic<int> under eight threads); csrc/icp_cluster.hip gives it the device's atomics.  An Atomics has
//   int load(int x)                        parent[x], read atomically (any value parent[x] has held may come back)
//   int fetch_min(int x, int v)            parent[x] = min(parent[x], v), returns the value before
//   int compare_swap(int x, int e, int v)  if parent[x] == e then parent[x] = v; returns the value before
// No loop here ends on what another lane or thread does: each has a bound of its own, written next to it.
#pragma once

#ifndef PRG_UF_FN
#if defined(__HIPCC__)
#define PRG_UF_FN __host__ __device__ inline
#else
#define PRG_UF_FN inline
#endif
#endif

namespace prg {

// The root above x, of the moment.  Bound: at most x steps - every step goes to p = parent[x] with p < x (parent[x] <= x always,
// and p == x ends the loop), so the vertex strictly decreases and is never below 0.  On the way parent[x] is lowered to its
// grandparent (path halving): a value of x's component and <= p, so the invariant holds.  A stale read only returns an older,
// larger parent, which is in the component and <= x just the same.
template <class Atomics>
PRG_UF_FN int uf_find(Atomics& a, int x) {
    for (;;) {
        const int p = a.load(x);
        if (p == x) return x;
        const int g = a.load(p);
        if (g < p) a.fetch_min(x, g);
        x = p;
    }
}

// Joins the components of u and v.  Bound: at most max(u, v) + 1 rounds - a round ends the call (one root for both, or the
// larger root hooked under the smaller), or its compare-and-swap finds that the larger root `hi` is a root no more and returns
// its new parent `now` < hi; the next round starts from (now, lo) with both below hi, so the larger member of the pair
// strictly decreases.  Nothing is awaited: a failed hook carries on from the value that made it fail.
template <class Atomics>
PRG_UF_FN void uf_hook(Atomics& a, int u, int v) {
    for (;;) {
        u = uf_find(a, u);
        v = uf_find(a, v);
        if (u == v) return;
        const int hi = u > v ? u : v, lo = u > v ? v : u;
        const int now = a.compare_swap(hi, hi, lo);
        if (now == hi) return;  // hi was a root and hangs under lo now
        u = now;
        v = lo;
    }
}

}  // namespace prg
