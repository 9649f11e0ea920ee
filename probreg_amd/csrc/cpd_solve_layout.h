// Sizes and carving of the M-step / BCPD solve workspace (prg_cpd::nr_solve), host arithmetic only: a driver sizes the block
// with `total` and takes every pointer from the same object's offsets (all in doubles).  The pivot flag is the first int of
// the 16 doubles at the end.  tests/host/solve_layout_check.cpp states the totals and the region order as formulas.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace prg {
constexpr int kSolveNB = 128;       // block edge of the factorisation (== kSpdBlock)
constexpr int kSolveThreads = 256;  // workgroup of the drivers' row kernels: k_traces leaves two partials per workgroup
constexpr int kGramTile = 64;       // k_lr_gram: tile edge
constexpr int kGramSlab = 32;       // ... points per LDS slab

namespace layout {
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t rup(int64_t v, int64_t q) { return cdiv(v, q) * q; }
struct Carver {  // c(n): the offset of the next n doubles
    size_t at = 0;
    size_t operator()(size_t n) { return (at += n) - n; }
};
}  // namespace layout

// The reduced r x r system of a plan that holds the factor F [rank][ld] of its kernel matrix.
struct LowRankLayout {
    int64_t rp, chunk;  // rank in whole blocks; points per part of the sum over the points
    int ntile, nsplit;  // lower-triangle tiles of F^T D F; parts
    bool small;         // (beyond 1024 the MFMA panel solves of the look-ahead factorisation pay for their inverses)
    size_t n_s, n_linv, n_vec, n_gram, n_u;  // S | block inverses | one [ld][3] vector | tile partials | F^T B partials
};
inline LowRankLayout make_lowrank_layout(int64_t m, int64_t ld, int rank) {
    using namespace layout;
    LowRankLayout L;
    L.rp = rup(rank, kSolveNB);
    const int tiles1 = (int)cdiv(rank, kGramTile);
    L.ntile = tiles1 * (tiles1 + 1) / 2;
    // split the sum over the points so that the chip is full (~512 workgroups of >= 8 slabs), in whole slabs
    const int64_t want = 512 / L.ntile > 1 ? 512 / L.ntile : 1, most = cdiv(m, 8 * kGramSlab);
    L.chunk = rup(cdiv(m, want < most ? want : most), kGramSlab);
    L.nsplit = (int)cdiv(m, L.chunk);
    L.small = L.rp <= 1024;
    L.n_s = (size_t)L.rp * L.rp, L.n_linv = (size_t)L.rp * kSolveNB, L.n_vec = (size_t)ld * 3;
    L.n_gram = (size_t)L.nsplit * L.ntile * kGramTile * kGramTile, L.n_u = (size_t)L.nsplit * rank * 3;
    return L;
}

// ---- one carving per driver: offsets in the order of the regions, then the size of the block -------------------------------
struct NonrigidDenseWs { size_t S, linv, b3, gb, v, sp, r3, dw, trpart, info, total; };
inline NonrigidDenseWs nonrigid_dense_ws(int64_t m) {
    const size_t mp = (size_t)layout::rup(m, kSolveNB), n_vec = mp * 3;
    layout::Carver c;
    NonrigidDenseWs w;
    w.S = c(mp * mp), w.linv = c(mp * kSolveNB);
    w.b3 = c(n_vec), w.gb = c(n_vec), w.v = c(n_vec), w.sp = c(n_vec), w.r3 = c(n_vec), w.dw = c(n_vec);
    w.trpart = c(2 * (size_t)layout::cdiv(m, kSolveThreads)), w.info = c(16), w.total = c.at;
    return w;
}
struct NonrigidLowrankWs { size_t S, linv, part, upart, b3, sp, fz, gb, r3, dw, z, trpart, info, total; };
inline NonrigidLowrankWs nonrigid_lowrank_ws(const LowRankLayout& L, int64_t m) {
    layout::Carver c;
    NonrigidLowrankWs w;
    w.S = c(L.n_s), w.linv = c(L.n_linv), w.part = c(L.n_gram), w.upart = c(L.n_u);
    w.b3 = c(L.n_vec), w.sp = c(L.n_vec), w.fz = c(L.n_vec), w.gb = c(L.n_vec), w.r3 = c(L.n_vec), w.dw = c(L.n_vec);
    w.z = c((size_t)L.rp * 3), w.trpart = c(2 * (size_t)layout::cdiv(m, kSolveThreads)), w.info = c(16), w.total = c.at;
    return w;
}
// (X = L^-1; linv is used by the look-ahead Cholesky only)
struct BcpdLowrankWs { size_t S, X, linv, part, upart, b3, sp, nu, diag, z, info, total; };
inline BcpdLowrankWs bcpd_lowrank_ws(const LowRankLayout& L) {
    layout::Carver c;
    BcpdLowrankWs w;
    w.S = c(L.n_s), w.X = c(L.n_s), w.linv = c(L.n_linv), w.part = c(L.n_gram), w.upart = c(L.n_u);
    w.b3 = c(L.n_vec), w.sp = c(L.n_vec), w.nu = c(L.n_vec), w.diag = c(L.n_vec);
    w.z = c((size_t)L.rp * 3), w.info = c(16), w.total = c.at;
    return w;
}
struct BcpdDenseWs { size_t S, wt, linv, b3, gb, v, sp, gt, tv, diag, info, total; };
inline BcpdDenseWs bcpd_dense_ws(int64_t m) {
    const size_t mp = (size_t)layout::rup(m, kSolveNB), n_vec = mp * 3;
    layout::Carver c;
    BcpdDenseWs w;
    w.S = c(mp * mp), w.wt = c(mp * mp), w.linv = c(mp * kSolveNB);
    w.b3 = c(n_vec), w.gb = c(n_vec), w.v = c(n_vec), w.sp = c(n_vec), w.gt = c(n_vec), w.tv = c(n_vec);
    w.diag = c(mp), w.info = c(16), w.total = c.at;
    return w;
}
}  // namespace prg
