// Drives csrc/fgr.h on the host (tests/test_fgr_host.py builds it with -ffp-contract=off under AddressSanitizer and UBSan and
// runs it on its own; no HIP runtime): for every case file named on the command line it normalises the clouds, runs the tuple
// test in ascending trial order, forms the 28 sums and the weights of the used pairs at the file's pose and mu in the
// definition's order (runs of kRun pairs, ascending), walks the schedule of mu and takes the pose back to the caller's units,
// and prints all of it with the doubles as hex floats.  The test compares the output with tests/oracle_fgr.py bit for bit.
//
// A case file: "M N C seed tuple_scale cap use_absolute_scale tuple_test iterations decrease_mu division_factor mcd mu", the
// pose (12), M rows of the source, N rows of the target, C rows of (source index, target index); every number a hex float or
// an integer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../probreg_amd/csrc/fgr.h"

namespace {

namespace fg = prg::fgr;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

void read_rows(std::FILE* f, std::vector<double>& v) {
    for (double& x : v) CHECK(std::fscanf(f, "%la", &x) == 1);
}

// mean of n rows: runs of kRun rows in ascending order, the runs added in ascending order, divided by the count
void mean_of(const std::vector<double>& x, int64_t n, double mean[3]) {
    double total[3] = {0.0, 0.0, 0.0};
    for (int64_t i0 = 0; i0 < n; i0 += fg::kRun) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t i = i0; i < i0 + fg::kRun && i < n; ++i)
            for (int a = 0; a < 3; ++a) acc[a] = fg::add(acc[a], x[(size_t)i * 3 + a]);
        for (int a = 0; a < 3; ++a) total[a] = fg::add(total[a], acc[a]);
    }
    for (int a = 0; a < 3; ++a) mean[a] = fg::quot(total[a], (double)n);
}

double farthest2(const std::vector<double>& x, int64_t n, const double mean[3]) {
    double far = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double dx = fg::sub(x[(size_t)i * 3], mean[0]), dy = fg::sub(x[(size_t)i * 3 + 1], mean[1]);
        const double dz = fg::sub(x[(size_t)i * 3 + 2], mean[2]);
        const double d2 = fg::add(fg::add(fg::mul(dx, dx), fg::mul(dy, dy)), fg::mul(dz, dz));
        if (d2 > far) far = d2;
    }
    return far;
}

void run(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    CHECK(f != nullptr);
    long long M, N, C, cap;
    unsigned long long seed;
    int use_abs, tuple_test, iterations, decrease;
    double s, division, mcd, mu, pose[12];
    CHECK(std::fscanf(f, "%lld %lld %lld %llu %la %lld %d %d %d %d %la %la %la", &M, &N, &C, &seed, &s, &cap, &use_abs, &tuple_test,
                      &iterations, &decrease, &division, &mcd, &mu) == 13);
    CHECK(M >= 1 && N >= 1 && C >= 3 && C <= (1ll << 31) / fg::kTrialsPerPair && cap >= 1 && iterations >= 0);
    for (double& v : pose) CHECK(std::fscanf(f, "%la", &v) == 1);
    std::vector<double> src((size_t)M * 3), tgt((size_t)N * 3);
    read_rows(f, src);
    read_rows(f, tgt);
    std::vector<long long> corr((size_t)C * 2);
    for (long long& v : corr) CHECK(std::fscanf(f, "%lld", &v) == 1);
    std::fclose(f);
    for (long long c = 0; c < C; ++c) CHECK(corr[(size_t)c * 2] >= 0 && corr[(size_t)c * 2] < M && corr[(size_t)c * 2 + 1] >= 0 && corr[(size_t)c * 2 + 1] < N);

    double mp[3], mq[3];
    mean_of(src, M, mp);
    mean_of(tgt, N, mq);
    const double far_p = farthest2(src, M, mp), far_q = farthest2(tgt, N, mq);
    const double scale = fg::root(far_p > far_q ? far_p : far_q);
    const double sg = use_abs ? 1.0 : scale;
    std::printf("norm %a %a %a %a %a %a %a\n", mp[0], mp[1], mp[2], mq[0], mq[1], mq[2], scale);
    std::vector<double> pq((size_t)C * 6);
    for (long long c = 0; c < C; ++c)
        for (int a = 0; a < 3; ++a) {
            pq[(size_t)c * 6 + a] = fg::normalised(src[(size_t)corr[(size_t)c * 2] * 3 + a], mp[a], sg);
            pq[(size_t)c * 6 + 3 + a] = fg::normalised(tgt[(size_t)corr[(size_t)c * 2 + 1] * 3 + a], mq[a], sg);
        }

    std::vector<long long> used;
    long long n_tuples = 0, n_trials = 0;
    if (tuple_test) {
        const long long limit = (long long)fg::kTrialsPerPair * C;
        n_trials = limit;
        for (long long t = 0; t < limit && n_tuples < cap; ++t) {
            uint32_t id[3];
            double p[3][3], q[3][3];
            for (int j = 0; j < 3; ++j) {
                id[j] = fg::draw(seed, (uint64_t)t, j, (uint32_t)C);
                CHECK((long long)id[j] < C);
                for (int a = 0; a < 3; ++a) {
                    p[j][a] = pq[(size_t)id[j] * 6 + a];
                    q[j][a] = pq[(size_t)id[j] * 6 + 3 + a];
                }
            }
            if (!fg::tuple_passes(p, q, s)) continue;
            for (int j = 0; j < 3; ++j) used.push_back(id[j]);
            if (++n_tuples == cap) n_trials = t + 1;
        }
    } else {
        for (long long c = 0; c < C; ++c) used.push_back(c);
    }
    std::printf("tuples %lld %lld\nused", n_tuples, n_trials);
    for (long long u : used) std::printf(" %lld", u);
    std::printf("\n");

    const long long K = (long long)used.size();
    double total[fg::kSums] = {0.0};
    std::vector<double> w((size_t)K);
    for (long long k0 = 0; k0 < K; k0 += fg::kRun) {
        double acc[fg::kSums] = {0.0};
        for (long long k = k0; k < k0 + fg::kRun && k < K; ++k) {
            double c[fg::kSums];
            const double* e = &pq[(size_t)used[(size_t)k] * 6];
            const double l = fg::pair_terms(pose, mu, e, e + 3, c);
            w[(size_t)k] = fg::pair_weight(pose, mu, e, e + 3);
            CHECK(l == w[(size_t)k]);
            for (int i = 0; i < fg::kSums; ++i) acc[i] = fg::add(acc[i], c[i]);
        }
        for (int i = 0; i < fg::kSums; ++i) total[i] = fg::add(total[i], acc[i]);
    }
    std::printf("sums");
    for (double v : total) std::printf(" %a", v);
    std::printf("\nweights");
    for (double v : w) std::printf(" %a", v);
    std::printf("\nmu");
    double m = use_abs ? scale : 1.0;
    for (int i = 0; i < iterations; ++i) {
        m = fg::next_mu(m, i, decrease != 0, division, mcd);
        std::printf(" %a", m);
    }
    double out[12];
    fg::denormalise(pose, mp, mq, sg, out);
    std::printf("\npose");
    for (double v : out) std::printf(" %a", v);
    std::printf("\n");
}

void check_rules() {
    CHECK(fg::weight(0.37, 0.0) == 1.0 && fg::weight(0.5, 0.5) == 0.25);
    CHECK(!fg::edge_agrees(0.0, 0.0, 0.95));                          // a repeated correspondence: both edges 0, "<" is strict
    CHECK(!fg::edge_agrees(0.95, 1.0, 0.95 / 0.95) && fg::edge_agrees(1.0, 1.0, 0.95));
    CHECK(!fg::edge_agrees(1.0, 2.0, 0.95) && !fg::edge_agrees(2.0, 1.0, 0.95));
    CHECK(fg::next_mu(1.0, 0, true, 2.0, 0.025) == 0.5 && fg::next_mu(1.0, 1, true, 2.0, 0.025) == 1.0);
    CHECK(fg::next_mu(0.025, 4, true, 2.0, 0.025) == 0.025 && fg::next_mu(1.0, 4, false, 2.0, 0.025) == 1.0);
}

}  // namespace

int main(int argc, char** argv) {
    check_rules();
    for (int a = 1; a < argc; ++a) run(argv[a]);
    std::printf("fgr_check ok\n");
    return 0;
}
