// Drives csrc/union_find.h on the host (tests/test_union_find_host.py builds it under AddressSanitizer and UBSan and runs
// it on its own; no HIP runtime): random graphs with their edges in random orders against a sequential reference, the
// invariant parent[x] <= x after every operation, vertices that never enter (parent -1), and eight threads on std::atomic<int>.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../probreg_amd/csrc/union_find.h"

namespace {

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// one thread: a plain array
struct Plain {
    std::vector<int>& p;
    int load(int x) const { return p[(size_t)x]; }
    int fetch_min(int x, int v) {
        const int old = p[(size_t)x];
        p[(size_t)x] = std::min(old, v);
        return old;
    }
    int compare_swap(int x, int e, int v) {
        const int old = p[(size_t)x];
        if (old == e) p[(size_t)x] = v;
        return old;
    }
};

// many threads: relaxed atomics, as on the device
struct Shared {
    std::vector<std::atomic<int>>& p;
    int load(int x) const { return p[(size_t)x].load(std::memory_order_relaxed); }
    int fetch_min(int x, int v) {
        int old = p[(size_t)x].load(std::memory_order_relaxed);
        // at most old - v + 1 rounds: a failed exchange reloads a smaller value (parent only shrinks)
        while (old > v && !p[(size_t)x].compare_exchange_weak(old, v, std::memory_order_relaxed)) {
        }
        return old;
    }
    int compare_swap(int x, int e, int v) {
        p[(size_t)x].compare_exchange_strong(e, v, std::memory_order_relaxed);
        return e;
    }
};

using Edges = std::vector<std::pair<int, int>>;

// the smallest vertex of the component of every vertex that is in (a label propagation to the fixed point)
std::vector<int> reference(int n, const std::vector<char>& in, const Edges& edges) {
    std::vector<int> low((size_t)n, -1);
    for (int i = 0; i < n; ++i)
        if (in[(size_t)i]) low[(size_t)i] = i;
    for (bool moved = true; moved;) {
        moved = false;
        for (const auto& e : edges) {
            const int m = std::min(low[(size_t)e.first], low[(size_t)e.second]);
            if (low[(size_t)e.first] != m || low[(size_t)e.second] != m) {
                low[(size_t)e.first] = low[(size_t)e.second] = m;
                moved = true;
            }
        }
    }
    return low;
}

Edges random_graph(std::mt19937& rng, int n, int m, const std::vector<char>& in, int shape) {
    Edges edges;
    std::vector<int> members;
    for (int i = 0; i < n; ++i)
        if (in[(size_t)i]) members.push_back(i);
    if (members.size() < 2) return edges;
    std::uniform_int_distribution<size_t> pick(0, members.size() - 1);
    if (shape == 1) {  // one long path through a shuffle of the members: the deepest trees
        std::vector<int> path = members;
        std::shuffle(path.begin(), path.end(), rng);
        for (size_t k = 1; k < path.size(); ++k) edges.emplace_back(path[k - 1], path[k]);
    } else if (shape == 2) {  // a path in index order
        for (size_t k = 1; k < members.size(); ++k) edges.emplace_back(members[k - 1], members[k]);
    } else {
        for (int k = 0; k < m; ++k) edges.emplace_back(members[pick(rng)], members[pick(rng)]);
    }
    std::shuffle(edges.begin(), edges.end(), rng);
    return edges;
}

void check_roots(int n, const std::vector<char>& in, const std::vector<int>& low, const std::vector<int>& parent) {
    std::vector<int> copy = parent;
    Plain a{copy};
    for (int i = 0; i < n; ++i) {
        if (!in[(size_t)i]) {
            CHECK(parent[(size_t)i] == -1);
            continue;
        }
        CHECK(prg::uf_find(a, i) == low[(size_t)i]);
    }
}

void sequential_case(std::mt19937& rng, int n, int m, int shape, double keep) {
    std::vector<char> in((size_t)n);
    std::vector<int> parent((size_t)n);
    std::bernoulli_distribution coin(keep);
    for (int i = 0; i < n; ++i) {
        in[(size_t)i] = coin(rng) ? 1 : 0;
        parent[(size_t)i] = in[(size_t)i] ? i : -1;
    }
    const Edges edges = random_graph(rng, n, m, in, shape);
    const bool every = n <= 256;  // the whole invariant after every operation; else the vertices the operation names
    Plain a{parent};
    for (const auto& e : edges) {
        prg::uf_hook(a, e.first, e.second);
        if (every) {
            for (int x = 0; x < n; ++x) CHECK(parent[(size_t)x] <= x && (in[(size_t)x] ? parent[(size_t)x] >= 0 : parent[(size_t)x] == -1));
        } else {
            CHECK(parent[(size_t)e.first] <= e.first && parent[(size_t)e.second] <= e.second);
        }
        CHECK(prg::uf_find(a, e.first) == prg::uf_find(a, e.second));
    }
    for (int x = 0; x < n; ++x) CHECK(parent[(size_t)x] <= x);
    check_roots(n, in, reference(n, in, edges), parent);
}

void threaded_case(std::mt19937& rng, int n, int m, int shape) {
    constexpr int kThreads = 8;
    std::vector<char> in((size_t)n, 1);
    const Edges edges = random_graph(rng, n, m, in, shape);
    std::vector<std::atomic<int>> parent((size_t)n);
    for (int i = 0; i < n; ++i) parent[(size_t)i].store(i);
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t] {
            Shared a{parent};
            for (size_t k = (size_t)t; k < edges.size(); k += kThreads) prg::uf_hook(a, edges[k].first, edges[k].second);
        });
    for (auto& th : pool) th.join();
    std::vector<int> flat((size_t)n);
    for (int i = 0; i < n; ++i) {
        flat[(size_t)i] = parent[(size_t)i].load();
        CHECK(flat[(size_t)i] >= 0 && flat[(size_t)i] <= i);
    }
    check_roots(n, in, reference(n, in, edges), flat);
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    const int sizes[] = {1, 2, 3, 17, 64, 256, 1000, 4000};
    int cases = 0;
    for (int n : sizes)
        for (int shape = 0; shape < 3; ++shape)
            for (double keep : {1.0, 0.6}) {
                sequential_case(rng, n, shape == 0 ? 2 * n : n, shape, keep);
                if (shape == 0) sequential_case(rng, n, n / 2 + 1, shape, keep);  // many components
                ++cases;
            }
    for (int round = 0; round < 6; ++round)
        for (int shape = 0; shape < 3; ++shape) {
            threaded_case(rng, 3000, 12000, shape);
            ++cases;
        }
    std::printf("union_find_check ok (%d cases)\n", cases);
    return 0;
}
