// Host check of the descriptor part of probreg_amd/csrc/cell_grid.h (tests/test_cell_grid_host.py builds this with the host
// compiler under AddressSanitizer / UBSan and runs it; it is not linked against the HIP runtime).  Every expectation is
// written out from DESIGN.md section 3.9: table = the power of two >= 2 n in [2^10, 2^26]; cells are floor((x - lo) / edge)
// clamped to [0, 2^30); dim = cell_of(hi) + 1; the key is row-major while the box has at most `table` cells and Teschner's
// hash masked to the table otherwise; slack = (max dim + 1) 2^-48.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../probreg_amd/csrc/cell_grid.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

int main() {
    using namespace prg;
    // table bits
    const int64_t ns[6] = {1, 512, 513, (int64_t)1 << 25, ((int64_t)1 << 25) + 1, (int64_t)1 << 30};
    const unsigned want_bits[6] = {10, 10, 11, 26, 26, 26};
    for (int i = 0; i < 6; ++i) CHECK(cell_table_bits(ns[i]) == want_bits[i]);

    // 16 x 8 x 8 = 1024 cells of edge 0.5 from (-1, 2, 3): exactly the table of 2^10, dense
    const double lo[3] = {-1.0, 2.0, 3.0};
    const double hi[3] = {-1.0 + 7.75, 2.0 + 3.75, 3.0 + 3.5};  // cells 15, 7, 7
    const CellGrid d = make_cell_grid(lo, hi, 0.5, 10);
    CHECK(d.dim[0] == 16 && d.dim[1] == 8 && d.dim[2] == 8);
    CHECK(d.mask == 1023u && d.dense == 1 && cell_entries(d) == 1024);
    CHECK(d.edge == 0.5 && d.slack == 17.0 / 281474976710656.0);  // (16 + 1) 2^-48
    for (int a = 0; a < 3; ++a) CHECK(d.lo[a] == lo[a] && d.hi[a] == hi[a]);
    // row-major keys at the corners of the box
    const int cx = cell_of(hi[0], lo[0], 0.5), cy = cell_of(hi[1], lo[1], 0.5), cz = cell_of(hi[2], lo[2], 0.5);
    CHECK(cx == 15 && cy == 7 && cz == 7);
    CHECK(cell_key(0, 0, 0, d) == 0u);
    CHECK(cell_key(cx, 0, 0, d) == 15u);
    CHECK(cell_key(0, cy, 0, d) == 7u * 16u);
    CHECK(cell_key(0, 0, cz, d) == 7u * 8u * 16u);
    CHECK(cell_key(cx, cy, cz, d) == 1023u);

    // one cell more (1025 x 1 x 1) is hashed, and its buckets are the table
    const double lo1[3] = {0.0, 0.0, 0.0}, hi1[3] = {1024.5, 0.0, 0.0};
    const CellGrid h = make_cell_grid(lo1, hi1, 1.0, 10);
    CHECK(h.dim[0] == 1025 && h.dim[1] == 1 && h.dim[2] == 1);
    CHECK(h.dense == 0 && h.mask == 1023u && cell_entries(h) == 1024);
    CHECK(h.slack == 1026.0 / 281474976710656.0);
    const int cells[4][3] = {{0, 0, 0}, {1024, 0, 0}, {7, 3, 1}, {1073741823, 1073741823, 1073741823}};
    for (int i = 0; i < 4; ++i) {
        const uint64_t x = (uint64_t)cells[i][0] * 73856093ull ^ (uint64_t)cells[i][1] * 19349663ull ^
                           (uint64_t)cells[i][2] * 83492791ull;
        const unsigned want = (unsigned)((x ^ (x >> 29)) & 1023ull);
        const unsigned got = cell_key(cells[i][0], cells[i][1], cells[i][2], h);
        CHECK(got <= h.mask && got == want);
    }
    // a far outlier: about 4e12 cells against a table of 2^11
    const double lo2[3] = {-1.0, -700.0, -1.0}, hi2[3] = {900.0, 1.0, 800.0};
    const CellGrid f = make_cell_grid(lo2, hi2, 0.05, 11);
    CHECK(f.dense == 0 && f.mask == 2047u && cell_entries(f) == 2048);

    // a single point
    const double p[3] = {0.25, -3.0, 1.0e6};
    const CellGrid one = make_cell_grid(p, p, 0.1, 10);
    CHECK(one.dim[0] == 1 && one.dim[1] == 1 && one.dim[2] == 1 && one.dense == 1 && cell_entries(one) == 1);
    CHECK(one.slack == 2.0 / 281474976710656.0);

    // the clamp: below lo, beyond 2^30 cells, NaN - the cast to int sees a value in range every time
    CHECK(cell_of(-5.0, 0.0, 1.0) == 0);
    CHECK(cell_of(-1.0e300, 0.0, 1.0e-300) == 0);
    CHECK(cell_of(1.0e300, 0.0, 1.0) == 1073741823);
    CHECK(cell_of(1.0e300, 0.0, 1.0e-300) == 1073741823);  // the quotient is +inf
    CHECK(cell_of(NAN, 0.0, 1.0) == 0);
    CHECK(cell_of(2.5, 1.0, 0.5) == 3 && cell_of(2.49, 1.0, 0.5) == 2);
    // monotone across the clamp
    CHECK(cell_of(1073741822.5, 0.0, 1.0) == 1073741822 && cell_of(1073741823.5, 0.0, 1.0) == 1073741823 &&
          cell_of(1073741824.5, 0.0, 1.0) == 1073741823);

    if (g_failed) {
        fprintf(stderr, "cell_grid_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("cell_grid_check ok\n");
    return 0;
}
