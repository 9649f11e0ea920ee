// Plane segmentation, the part every decision is taken by: the draw of a hypothesis, its validity test, the
// plane of a triple, the sign rule, the anchored distance, the inlier predicate and the ranking of two scores.  Everything is
// fp64 and every operation is rounded once, so that a plain IEEE restatement gets the same bits.
//
// Host-compilable, as grid_search.h and union_find.h are: csrc/plane_seg.hip compiles it for the device, where the library's
// -ffp-contract=on would fuse a * b + c and the single roundings are therefore spelled __dmul_rn / __dadd_rn / __dsub_rn;
// tests/host/plane_seg_check.cpp compiles it with the host compiler under -ffp-contract=off, where the plain operators are
// the same operations.  Kernel and host check share this one text.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef PRG_PS_FN
#if defined(__HIPCC__)
#define PRG_PS_FN __host__ __device__ __forceinline__
#else
#define PRG_PS_FN inline
#endif
#endif

namespace prg {
namespace plane {

constexpr int kScorePiece = 1024;   // points per piece of a hypothesis' ordered sum (part of the definition)
constexpr int kRefitRun = 64;       // points per run of the refit's sums (part of the definition)
constexpr double kDegenerate = 0.05;  // |e1 x e2| >= kDegenerate |e1| |e2|: the constant of global_reg.hip

#if defined(__HIP_DEVICE_COMPILE__)
PRG_PS_FN double mul(double a, double b) { return __dmul_rn(a, b); }
PRG_PS_FN double add(double a, double b) { return __dadd_rn(a, b); }
PRG_PS_FN double sub(double a, double b) { return __dsub_rn(a, b); }
PRG_PS_FN double quot(double a, double b) { return __ddiv_rn(a, b); }
PRG_PS_FN double root(double a) { return __dsqrt_rn(a); }
#else
PRG_PS_FN double mul(double a, double b) { return a * b; }
PRG_PS_FN double add(double a, double b) { return a + b; }
PRG_PS_FN double sub(double a, double b) { return a - b; }
PRG_PS_FN double quot(double a, double b) { return a / b; }
PRG_PS_FN double root(double a) { return sqrt(a); }
#endif

PRG_PS_FN uint64_t splitmix64(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// point index j (0, 1, 2) of hypothesis `h` (offset included) among n points: < n
PRG_PS_FN uint32_t draw(uint64_t seed, uint64_t h, int j, uint32_t n) {
    const uint64_t z = splitmix64(seed, 3ull * h + (uint64_t)j + 1ull);
    return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);
}

// (x x + y y) + z z, then the root
PRG_PS_FN double norm3(double x, double y, double z) { return root(add(add(mul(x, x), mul(y, y)), mul(z, z))); }

// n <- -n unless the component of largest magnitude is positive; ties go to the lowest axis (the rule of the FPFH normals)
PRG_PS_FN void fix_sign(double n[3]) {
    const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
    const double lead = (a0 >= a1 && a0 >= a2) ? n[0] : (a1 >= a2 ? n[1] : n[2]);
    if (lead < 0.0) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
}

// The plane through p0, p1, p2 as pl = (n_x, n_y, n_z, a_x, a_y, a_z), anchored at p0.  Returns whether the triangle passes
// the degeneracy test (distinct indices are the caller's to check); pl is all zero when it does not.
PRG_PS_FN bool plane_of_triple(const double p0[3], const double p1[3], const double p2[3], double pl[6]) {
    const double e1[3] = {sub(p1[0], p0[0]), sub(p1[1], p0[1]), sub(p1[2], p0[2])};
    const double e2[3] = {sub(p2[0], p0[0]), sub(p2[1], p0[1]), sub(p2[2], p0[2])};
    const double cx = sub(mul(e1[1], e2[2]), mul(e1[2], e2[1]));
    const double cy = sub(mul(e1[2], e2[0]), mul(e1[0], e2[2]));
    const double cz = sub(mul(e1[0], e2[1]), mul(e1[1], e2[0]));
    const double len = norm3(cx, cy, cz);
    const double lim = mul(mul(kDegenerate, norm3(e1[0], e1[1], e1[2])), norm3(e2[0], e2[1], e2[2]));
    const bool ok = len >= lim && len > 0.0;
    double n[3] = {0.0, 0.0, 0.0};
    if (ok) {
        n[0] = quot(cx, len);
        n[1] = quot(cy, len);
        n[2] = quot(cz, len);
        fix_sign(n);
    }
    for (int k = 0; k < 3; ++k) {
        pl[k] = n[k];
        pl[3 + k] = ok ? p0[k] : 0.0;
    }
    return ok;
}

// signed distance of x from the plane pl: (n_x (x - a_x) + n_y (y - a_y)) + n_z (z - a_z); never n . x + d
PRG_PS_FN double distance(const double pl[6], double x, double y, double z) {
    return add(add(mul(pl[0], sub(x, pl[3])), mul(pl[1], sub(y, pl[4]))), mul(pl[2], sub(z, pl[5])));
}

// |dist| <= tau: a point exactly at tau is inside
PRG_PS_FN bool within(double dist, double tau) { return fabs(dist) <= tau; }

// the normal test of a point with normal m of length len (taken once at upload): |n . m| >= cos_theta len, never for m = 0
PRG_PS_FN bool normal_agrees(const double pl[6], double mx, double my, double mz, double len, double cos_theta) {
    const double dot = add(add(mul(pl[0], mx), mul(pl[1], my)), mul(pl[2], mz));
    return len > 0.0 && fabs(dot) >= mul(cos_theta, len);
}

// (count descending, sum ascending, h ascending) is a strict total order, so the winner does not depend on how a reduction
// is shaped
PRG_PS_FN bool ranks_ahead(int ca, double sa, int64_t ha, int cb, double sb, int64_t hb) {
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa < sb;
    return ha < hb;
}

// The refit's covariance from the ten raw sums t = (k, s_x, s_y, s_z, xx, xy, xz, yy, yz, zz) of q = x - a over the inliers:
// c = s / k, C_ab = S_ab / k - c_a c_b, in (xx, xy, xz, yy, yz, zz) order.
PRG_PS_FN void covariance(const double t[10], double c[3], double cov[6]) {
    for (int a = 0; a < 3; ++a) c[a] = quot(t[1 + a], t[0]);
    cov[0] = sub(quot(t[4], t[0]), mul(c[0], c[0]));
    cov[1] = sub(quot(t[5], t[0]), mul(c[0], c[1]));
    cov[2] = sub(quot(t[6], t[0]), mul(c[0], c[2]));
    cov[3] = sub(quot(t[7], t[0]), mul(c[1], c[1]));
    cov[4] = sub(quot(t[8], t[0]), mul(c[1], c[2]));
    cov[5] = sub(quot(t[9], t[0]), mul(c[2], c[2]));
}

}  // namespace plane
}  // namespace prg
