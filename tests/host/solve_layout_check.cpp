// Host check of probreg_amd/csrc/cpd_solve_layout.h (tests/test_solve_layout_host.py builds this with the host compiler under
// AddressSanitizer / UBSan and runs it; no HIP).  The workspace of each solve driver is one block of doubles; its size and the
// order of its regions are written out here as the formulas the drivers used before the layout had a file of its own:
//   non-rigid dense     S mp^2 | linv nblk 128^2 | b3 gb v sp r3 dw (3 mp each) | trpart 2 ceil(m / 256) | 16 (info first)
//   non-rigid low-rank  S rp^2 | linv | part | upart | b3 sp fz gb r3 dw (3 ld each) | z 3 rp | trpart | 16
//   BCPD low-rank       S rp^2 | X rp^2 | linv | part | upart | b3 sp nu diag (3 ld each) | z 3 rp | 16
//   BCPD dense          S mp^2 | wt mp^2 | linv | b3 gb v sp gt tv (3 mp each) | diag mp | 16
// with mp = round_up(m, 128), rp = round_up(rank, 128), part = nsplit ntile 64^2, upart = nsplit rank 3, and ld the leading
// dimension of the kernel factor, which build_lowrank_factor (cpd_nonrigid.hip) sets to round_up(m, 256) + 32.
#include <stdint.h>
#include <stdio.h>

#include "../../probreg_amd/csrc/cpd_solve_layout.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t rup(int64_t a, int64_t b) { return cdiv(a, b) * b; }

// off[0 .. n) are the regions in the order they must have, off[n - 1] is info; len[i] is what region i must hold
static void check_regions(const size_t* off, const size_t* len, int n, size_t total, size_t want_total) {
    CHECK(off[0] == 0);
    for (int i = 0; i + 1 < n; ++i) CHECK(off[i] + len[i] == off[i + 1]);  // today's order, nothing overlaps, no holes
    for (int i = 0; i < n; ++i) CHECK(off[i] * sizeof(double) % 8 == 0);
    CHECK(off[n - 1] * sizeof(double) + sizeof(int) <= total * sizeof(double));  // info lies inside the block ...
    CHECK(off[n - 1] + 16 == total);                                             // ... at the head of the 16-double tail
    CHECK(total == want_total);
}

int main() {
    using namespace prg;
    const int64_t dense_m[7] = {1, 127, 128, 129, 1100, 2177, 20000};
    for (int64_t m : dense_m) {
        const size_t mp = (size_t)rup(m, 128), n_s = mp * mp, n_linv = mp / 128 * 128 * 128, n_vec = 3 * mp;
        const size_t tr = 2 * (size_t)cdiv(m, 256);
        {
            const NonrigidDenseWs w = nonrigid_dense_ws(m);
            const size_t off[] = {w.S, w.linv, w.b3, w.gb, w.v, w.sp, w.r3, w.dw, w.trpart, w.info};
            const size_t len[] = {n_s, n_linv, n_vec, n_vec, n_vec, n_vec, n_vec, n_vec, tr, 16};
            check_regions(off, len, 10, w.total, n_s + n_linv + 6 * n_vec + tr + 16);
        }
        {
            const BcpdDenseWs w = bcpd_dense_ws(m);
            const size_t off[] = {w.S, w.wt, w.linv, w.b3, w.gb, w.v, w.sp, w.gt, w.tv, w.diag, w.info};
            const size_t len[] = {n_s, n_s, n_linv, n_vec, n_vec, n_vec, n_vec, n_vec, n_vec, mp, 16};
            check_regions(off, len, 11, w.total, 2 * n_s + n_linv + 6 * n_vec + mp + 16);
        }
    }

    const int64_t lr_m[3] = {300, 6000, 100000};
    const int ranks[6] = {1, 128, 129, 1024, 1025, 2048};
    for (int64_t m : lr_m)
        for (int rank : ranks) {
            const int64_t ld = rup(m, 256) + 32;  // f_ld (cpd_nonrigid.hip, build_lowrank_factor)
            const LowRankLayout L = make_lowrank_layout(m, ld, rank);
            CHECK(L.rp == rup(rank, 128));
            const int tiles1 = (int)cdiv(rank, 64);
            CHECK(L.ntile == tiles1 * (tiles1 + 1) / 2);
            CHECK(L.small == (rank <= 1024));
            CHECK(L.nsplit >= 1);
            CHECK(L.chunk % 32 == 0);  // whole slabs
            CHECK((int64_t)L.nsplit * L.chunk >= m);
            CHECK((int64_t)(L.nsplit - 1) * L.chunk < m);  // no part is empty
            // the split rule: ~512 workgroups of >= 8 slabs
            int64_t want = 512 / L.ntile;
            if (want < 1) want = 1;
            if (want > cdiv(m, 256)) want = cdiv(m, 256);
            CHECK(L.chunk == rup(cdiv(m, want), 32) && L.nsplit == cdiv(m, L.chunk));

            const size_t rp = (size_t)L.rp, n_s = rp * rp, n_linv = rp / 128 * 128 * 128, n_vec = 3 * (size_t)ld;
            const size_t n_gram = (size_t)L.nsplit * L.ntile * 64 * 64, n_u = (size_t)L.nsplit * rank * 3, n_part = n_gram + n_u;
            const size_t tr = 2 * (size_t)cdiv(m, 256);
            CHECK(L.n_s == n_s && L.n_linv == n_linv && L.n_vec == n_vec && L.n_gram == n_gram && L.n_u == n_u);
            {
                const NonrigidLowrankWs w = nonrigid_lowrank_ws(L, m);
                const size_t off[] = {w.S, w.linv, w.part, w.upart, w.b3, w.sp, w.fz, w.gb, w.r3, w.dw, w.z, w.trpart, w.info};
                const size_t len[] = {n_s, n_linv, n_gram, n_u, n_vec, n_vec, n_vec, n_vec, n_vec, n_vec, 3 * rp, tr, 16};
                check_regions(off, len, 13, w.total, n_s + n_linv + n_part + 6 * n_vec + rp * 3 + tr + 16);
            }
            {
                const BcpdLowrankWs w = bcpd_lowrank_ws(L);
                const size_t off[] = {w.S, w.X, w.linv, w.part, w.upart, w.b3, w.sp, w.nu, w.diag, w.z, w.info};
                const size_t len[] = {n_s, n_s, n_linv, n_gram, n_u, n_vec, n_vec, n_vec, n_vec, 3 * rp, 16};
                check_regions(off, len, 11, w.total, 2 * n_s + n_linv + n_part + 4 * n_vec + rp * 3 + 16);
            }
        }
    if (g_failed) {
        fprintf(stderr, "solve_layout_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("solve_layout_check ok\n");
    return 0;
}
