// Fast global registration, the part every number is defined by: the normalised point, the edge test of a
// trial, the line-process weight, what one pair adds to the 27 sums of the normal equations and to the objective, the
// schedule of mu and the way back to the caller's units.  Everything is fp64 and every operation is rounded once, so that a
// plain IEEE restatement gets the same bits.
//
// Host-compilable, as plane_seg.h is (whose single-rounded operations and counter-based draw it takes over): csrc/fgr.hip
// compiles it for the device, tests/host/fgr_check.cpp with the host compiler under -ffp-contract=off.
#pragma once
#include "plane_seg.h"

namespace prg {
namespace fgr {

using plane::add;
using plane::mul;
using plane::quot;
using plane::root;
using plane::sub;

constexpr int kRun = 64;           // rows per run of every ordered sum (part of the definition)
constexpr int kSums = 28;          // A's upper triangle row-major (21), g (6), the objective
constexpr int kTrialsPerPair = 100;  // the tuple test looks at trials t < kTrialsPerPair C

// correspondence index j (0, 1, 2) of trial t among C correspondences: the draw of section 3.13
PRG_PS_FN uint32_t draw(uint64_t seed, uint64_t t, int j, uint32_t C) { return plane::draw(seed, t, j, C); }

// component of a normalised point: (x - mean) / scale_global
PRG_PS_FN double normalised(double x, double mean, double scale_global) { return quot(sub(x, mean), scale_global); }

// |a - b|: the differences, then (dx dx + dy dy) + dz dz, then the root
PRG_PS_FN double edge(const double a[3], const double b[3]) {
    return plane::norm3(sub(a[0], b[0]), sub(a[1], b[1]), sub(a[2], b[2]));
}

// one edge of a tuple: li s < lj and lj s < li, both strict (li = lj = 0, a repeated correspondence, fails)
PRG_PS_FN bool edge_agrees(double li, double lj, double s) { return mul(li, s) < lj && mul(lj, s) < li; }

// the tuple test of three pairs (p_j, q_j) on the edges (0, 1), (1, 2), (2, 0)
PRG_PS_FN bool tuple_passes(const double p[3][3], const double q[3][3], double s) {
    bool ok = true;
    for (int e = 0; e < 3; ++e) {
        const int a = e, b = (e + 1) % 3;
        ok = ok && edge_agrees(edge(p[a], p[b]), edge(q[a], q[b]), s);
    }
    return ok;
}

// s = R p + t, component a: ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a (pose: rotation row-major, then the shift)
PRG_PS_FN void moved(const double pose[12], const double p[3], double s[3]) {
    for (int a = 0; a < 3; ++a)
        s[a] = add(add(add(mul(pose[3 * a], p[0]), mul(pose[3 * a + 1], p[1])), mul(pose[3 * a + 2], p[2])), pose[9 + a]);
}

// l = (mu / (mu + r2))^2
PRG_PS_FN double weight(double mu, double r2) {
    const double w = quot(mu, add(mu, r2));
    return mul(w, w);
}

// the line-process value of the pair (p, q) at `pose` and `mu`
PRG_PS_FN double pair_weight(const double pose[12], double mu, const double p[3], const double q[3]) {
    double s[3];
    moved(pose, p, s);
    const double r[3] = {sub(s[0], q[0]), sub(s[1], q[1]), sub(s[2], q[2])};
    return weight(mu, add(add(mul(r[0], r[0]), mul(r[1], r[1])), mul(r[2], r[2])));
}

// What the pair (p, q) adds at `pose` and `mu`: c[0 .. 21) = l J^T J (upper triangle, row-major), c[21 .. 27) = l J^T r,
// c[27] = l r2 + mu (1 - sqrt l)^2, with J = (-[s]x | I), r = s - q, r2 = (r_x r_x + r_y r_y) + r_z r_z.  An entry of J^T J or
// J^T r is its three products added in ascending row order; the products with J's zeros and ones are exact and left out,
// which changes no bit.  Returns l.
PRG_PS_FN double pair_terms(const double pose[12], double mu, const double p[3], const double q[3], double c[kSums]) {
    double s[3];
    moved(pose, p, s);
    const double r[3] = {sub(s[0], q[0]), sub(s[1], q[1]), sub(s[2], q[2])};
    const double r2 = add(add(mul(r[0], r[0]), mul(r[1], r[1])), mul(r[2], r[2]));
    const double l = weight(mu, r2);
    const double s00 = mul(s[0], s[0]), s11 = mul(s[1], s[1]), s22 = mul(s[2], s[2]);
    c[0] = mul(l, add(s22, s11));
    c[1] = mul(l, -mul(s[1], s[0]));
    c[2] = mul(l, -mul(s[2], s[0]));
    c[3] = 0.0;
    c[4] = mul(l, -s[2]);
    c[5] = mul(l, s[1]);
    c[6] = mul(l, add(s22, s00));
    c[7] = mul(l, -mul(s[2], s[1]));
    c[8] = mul(l, s[2]);
    c[9] = 0.0;
    c[10] = mul(l, -s[0]);
    c[11] = mul(l, add(s11, s00));
    c[12] = mul(l, -s[1]);
    c[13] = mul(l, s[0]);
    c[14] = 0.0;
    c[15] = l;
    c[16] = 0.0;
    c[17] = 0.0;
    c[18] = l;
    c[19] = 0.0;
    c[20] = l;
    c[21] = mul(l, sub(mul(s[1], r[2]), mul(s[2], r[1])));
    c[22] = mul(l, sub(mul(s[2], r[0]), mul(s[0], r[2])));
    c[23] = mul(l, sub(mul(s[0], r[1]), mul(s[1], r[0])));
    c[24] = mul(l, r[0]);
    c[25] = mul(l, r[1]);
    c[26] = mul(l, r[2]);
    const double k = sub(1.0, root(l));
    c[27] = add(mul(l, r2), mul(mu, mul(k, k)));
    return l;
}

// mu after iteration i (counted from 0)
PRG_PS_FN double next_mu(double mu, int64_t i, bool decrease_mu, double division_factor, double maximum_correspondence_distance) {
    return (decrease_mu && i % 4 == 0 && mu > maximum_correspondence_distance) ? quot(mu, division_factor) : mu;
}

// The pose in the caller's units: R stays, t_out = (scale_global t + mean_q) - R mean_p with R mean_p as in moved().
PRG_PS_FN void denormalise(const double pose[12], const double mean_p[3], const double mean_q[3], double scale_global,
                           double out[12]) {
    for (int k = 0; k < 9; ++k) out[k] = pose[k];
    for (int a = 0; a < 3; ++a) {
        const double rm = add(add(mul(pose[3 * a], mean_p[0]), mul(pose[3 * a + 1], mean_p[1])), mul(pose[3 * a + 2], mean_p[2]));
        out[9 + a] = sub(add(mul(scale_global, pose[9 + a]), mean_q[a]), rm);
    }
}

}  // namespace fgr
}  // namespace prg
