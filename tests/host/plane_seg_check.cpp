// Drives csrc/plane_seg.h on the host (tests/test_plane_host.py builds it with -ffp-contract=off under AddressSanitizer and UBSan
// and runs it on its own; no HIP runtime): for every cloud file named on the command line it draws the hypotheses, builds their
// planes, scores them in the definition's order (pieces of kScorePiece points, ascending), picks the winner with ranks_ahead
// and forms one refit's ten sums and covariance on the winner's inliers, and prints all of it with the doubles as hex floats.
// The test compares the output with tests/oracle_plane.py bit for bit.
//
// A cloud file: "n H seed offset tau cos_theta" (cos_theta < 0: no normal test), then n rows of x y z, then, with a normal
// test, n rows of m_x m_y m_z; every number a hex float or an integer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../probreg_amd/csrc/plane_seg.h"

namespace {

namespace ps = prg::plane;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Cloud {
    int64_t n = 0, H = 0;
    uint64_t seed = 0, offset = 0;
    double tau = 0.0, cos_theta = -1.0;
    std::vector<double> xyz, nrm, len;
};

Cloud read_cloud(const char* path) {
    Cloud c;
    std::FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr);
    long long n, H;
    unsigned long long seed, offset;
    CHECK(std::fscanf(f, "%lld %lld %llu %llu %la %la", &n, &H, &seed, &offset, &c.tau, &c.cos_theta) == 6);
    CHECK(n >= 1 && n < (1ll << 31) && H >= 1 && H <= (1ll << 24));
    c.n = n; c.H = H; c.seed = seed; c.offset = offset;
    c.xyz.resize((size_t)n * 3);
    for (double& v : c.xyz) CHECK(std::fscanf(f, "%la", &v) == 1);
    if (c.cos_theta >= 0.0) {
        c.nrm.resize((size_t)n * 3);
        for (double& v : c.nrm) CHECK(std::fscanf(f, "%la", &v) == 1);
        c.len.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) c.len[(size_t)i] = ps::norm3(c.nrm[(size_t)i * 3], c.nrm[(size_t)i * 3 + 1], c.nrm[(size_t)i * 3 + 2]);
    }
    std::fclose(f);
    return c;
}

bool inlier(const Cloud& c, const double pl[6], int64_t i, double* dist) {
    const double* p = &c.xyz[(size_t)i * 3];
    const double d = ps::distance(pl, p[0], p[1], p[2]);
    *dist = d;
    bool in = ps::within(d, c.tau);
    if (c.cos_theta >= 0.0) {
        const double* m = &c.nrm[(size_t)i * 3];
        in = in && ps::normal_agrees(pl, m[0], m[1], m[2], c.len[(size_t)i], c.cos_theta);
    }
    return in;
}

void run(const char* path) {
    const Cloud c = read_cloud(path);
    std::printf("cloud %lld %lld\n", (long long)c.n, (long long)c.H);
    int best_c = -1;
    double best_s = 0.0;
    int64_t best_h = -1;
    std::vector<double> best_pl(6, 0.0);
    for (int64_t h = 0; h < c.H; ++h) {
        uint32_t id[3];
        for (int j = 0; j < 3; ++j) {
            id[j] = ps::draw(c.seed, c.offset + (uint64_t)h, j, (uint32_t)c.n);
            CHECK((int64_t)id[j] < c.n);
        }
        double pl[6];
        bool ok = ps::plane_of_triple(&c.xyz[(size_t)id[0] * 3], &c.xyz[(size_t)id[1] * 3], &c.xyz[(size_t)id[2] * 3], pl);
        ok = ok && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
        if (!ok)
            for (double& v : pl) v = 0.0;
        int cnt = -1;
        double sum = 0.0;
        if (ok) {
            cnt = 0;
            for (int64_t c0 = 0; c0 < c.n; c0 += ps::kScorePiece) {
                double piece = 0.0;
                for (int64_t i = c0; i < c0 + ps::kScorePiece && i < c.n; ++i) {
                    double d;
                    const bool in = inlier(c, pl, i, &d);
                    cnt += in ? 1 : 0;
                    piece = ps::add(piece, in ? ps::mul(d, d) : 0.0);
                }
                sum = ps::add(sum, piece);
            }
            if (best_h < 0 || ps::ranks_ahead(cnt, sum, h, best_c, best_s, best_h)) {
                best_c = cnt; best_s = sum; best_h = h;
                for (int k = 0; k < 6; ++k) best_pl[(size_t)k] = pl[k];
            }
        }
        std::printf("hyp %lld %u %u %u %d %a %a %a %a %a %a %d %a\n", (long long)h, id[0], id[1], id[2], ok ? 1 : 0, pl[0], pl[1],
                    pl[2], pl[3], pl[4], pl[5], cnt, sum);
    }
    std::printf("winner %lld\n", (long long)best_h);
    if (best_h < 0) return;
    // one refit's sums on the winner's inliers: runs of kRefitRun points in ascending order, the runs added in ascending order
    double t[10] = {0.0};
    for (int64_t c0 = 0; c0 < c.n; c0 += ps::kRefitRun) {
        double acc[10] = {0.0};
        for (int64_t i = c0; i < c0 + ps::kRefitRun && i < c.n; ++i) {
            double d;
            if (!inlier(c, best_pl.data(), i, &d)) continue;
            const double* p = &c.xyz[(size_t)i * 3];
            const double q[3] = {ps::sub(p[0], best_pl[3]), ps::sub(p[1], best_pl[4]), ps::sub(p[2], best_pl[5])};
            const double term[10] = {1.0, q[0], q[1], q[2], ps::mul(q[0], q[0]), ps::mul(q[0], q[1]), ps::mul(q[0], q[2]),
                                     ps::mul(q[1], q[1]), ps::mul(q[1], q[2]), ps::mul(q[2], q[2])};
            for (int k = 0; k < 10; ++k) acc[k] = ps::add(acc[k], term[k]);
        }
        for (int k = 0; k < 10; ++k) t[k] = ps::add(t[k], acc[k]);
    }
    std::printf("sums");
    for (double v : t) std::printf(" %a", v);
    std::printf("\n");
    if (t[0] >= 3.0) {
        double ctr[3], cov[6];
        ps::covariance(t, ctr, cov);
        std::printf("cov %a %a %a %a %a %a %a %a %a\n", ctr[0], ctr[1], ctr[2], cov[0], cov[1], cov[2], cov[3], cov[4], cov[5]);
    }
}

void check_sign_rule() {
    double a[3] = {-0.5, 0.5, 0.1};  // a tie of magnitudes: the lowest axis decides
    ps::fix_sign(a);
    CHECK(a[0] == 0.5 && a[1] == -0.5 && a[2] == -0.1);
    double b[3] = {0.1, -0.2, 0.2};
    ps::fix_sign(b);
    CHECK(b[0] == -0.1 && b[1] == 0.2 && b[2] == -0.2);
    double z[3] = {0.0, 0.0, 0.0};
    ps::fix_sign(z);
    CHECK(z[0] == 0.0 && z[1] == 0.0 && z[2] == 0.0);
    CHECK(ps::ranks_ahead(5, 1.0, 9, 4, 0.0, 0) && ps::ranks_ahead(5, 0.5, 9, 5, 1.0, 0) && ps::ranks_ahead(5, 1.0, 3, 5, 1.0, 4));
    CHECK(!ps::ranks_ahead(5, 1.0, 3, 5, 1.0, 3));
    CHECK(ps::within(0.25, 0.25) && ps::within(-0.25, 0.25) && !ps::within(0.2500000000000001, 0.25));
    const double pl[6] = {0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    CHECK(!ps::normal_agrees(pl, 0.0, 0.0, 0.0, 0.0, 0.0));  // a zero normal never passes
    CHECK(ps::normal_agrees(pl, 0.0, 0.0, -2.0, 2.0, 1.0));
}

}  // namespace

int main(int argc, char** argv) {
    check_sign_rule();
    for (int a = 1; a < argc; ++a) run(argv[a]);
    std::printf("plane_seg_check ok\n");
    return 0;
}
