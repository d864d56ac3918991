// TEST-ONLY program: the index work of the Vecchia ordering (csrc/ck_host.cpp: ck_host_vecchia_order) under
// -fsanitize=address,undefined (tests/test_vecchia_order_host.py builds and runs it; CPU only).
#include <stdio.h>

#include <numeric>
#include <random>

#include "ck_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Layout {
    int n_procs;
    int64_t n[2], n0p, npad;
    std::vector<int64_t> perm[2];
};

static Layout make_layout(std::mt19937_64& rng, int n_procs, int64_t n0, int64_t n1) {
    Layout L;
    L.n_procs = n_procs;
    L.n[0] = n0;
    L.n[1] = n_procs == 2 ? n1 : 0;
    L.n0p = L.n[1] > 0 ? (n0 + 63) / 64 * 64 : n0;
    L.npad = (L.n0p + L.n[1] + 127) / 128 * 128;
    for (int k = 0; k < 2; ++k) {
        L.perm[k].resize((size_t)L.n[k]);
        std::iota(L.perm[k].begin(), L.perm[k].end(), (int64_t)0);
        std::shuffle(L.perm[k].begin(), L.perm[k].end(), rng);
    }
    return L;
}

// distinct ranks: every output against its definition
static int run(const Layout& L, const std::vector<int64_t>& rank) {
    const int64_t N = L.n[0] + L.n[1];
    CHECK((int64_t)rank.size() == N);
    CkVecchiaOrder ord;
    CHECK(ck_host_vecchia_order(rank.data(), L.n_procs, L.n, L.n0p, L.npad, L.perm[0].data(), L.n_procs == 2 ? L.perm[1].data() : nullptr,
                                &ord) == 0);
    CHECK((int64_t)ord.pos.size() == N && (int64_t)ord.gself.size() == N && (int64_t)ord.rs.size() == L.npad);
    std::vector<int64_t> at((size_t)N, -1);   // datum at every position
    for (int64_t t = 0; t < N; ++t) {
        CHECK(ord.pos[(size_t)t] >= 0 && ord.pos[(size_t)t] < N && at[(size_t)ord.pos[(size_t)t]] == -1);
        at[(size_t)ord.pos[(size_t)t]] = t;
    }
    for (int64_t j = 1; j < N; ++j) CHECK(rank[(size_t)at[(size_t)(j - 1)]] < rank[(size_t)at[(size_t)j]]);
    int64_t n_real = 0;
    for (int64_t g = 0; g < L.npad; ++g) n_real += ord.rs[(size_t)g] != INT32_MAX;
    CHECK(n_real == N);
    for (int k = 0; k < L.n_procs; ++k)
        for (int64_t j = 0; j < L.n[k]; ++j) {
            const int64_t g = (k == 0 ? 0 : L.n0p) + j, t = (k == 0 ? 0 : L.n[0]) + L.perm[k][(size_t)j];
            CHECK(ord.rs[(size_t)g] == ord.pos[(size_t)t] && ord.gself[(size_t)t] == g);
        }
    return 0;
}

static int run_duplicate(const Layout& L, std::vector<int64_t> rank, int64_t a, int64_t b) {
    rank[(size_t)b] = rank[(size_t)a];
    CkVecchiaOrder ord;
    CHECK(ck_host_vecchia_order(rank.data(), L.n_procs, L.n, L.n0p, L.npad, L.perm[0].data(), L.n_procs == 2 ? L.perm[1].data() : nullptr,
                                &ord) == -1);
    CHECK(ord.dup[0] == std::min(a, b) && ord.dup[1] == std::max(a, b));
    return 0;
}

int main() {
    std::mt19937_64 rng(7);
    const int64_t sizes[][3] = {{2, 70, 33}, {2, 50, 0}, {1, 50, 0}, {2, 64, 64}, {1, 1, 0}, {2, 1, 0}, {2, 1, 1}, {2, 300, 257}};
    for (const auto& sz : sizes) {
        const Layout L = make_layout(rng, (int)sz[0], sz[1], sz[2]);
        const int64_t N = L.n[0] + L.n[1];
        std::vector<int64_t> rank((size_t)N);
        std::iota(rank.begin(), rank.end(), (int64_t)0);
        std::shuffle(rank.begin(), rank.end(), rng);
        CHECK(run(L, rank) == 0);   // a permutation: the one-pass route
        std::vector<int64_t> other(rank);
        for (auto& r : other) r = r * 5 - 3;   // negative ranks and ranks beyond N: the sort route
        CHECK(run(L, other) == 0);
        other = rank;
        for (auto& r : other) r = r == N - 1 ? INT64_MAX : (r == 0 ? INT64_MIN : r);   // the extremes of the type
        CHECK(run(L, other) == 0);
        if (N >= 2) {
            const int64_t a = (int64_t)(rng() % (uint64_t)N), b = (a + 1 + (int64_t)(rng() % (uint64_t)(N - 1))) % N;
            CHECK(run_duplicate(L, rank, a, b) == 0);
            std::vector<int64_t> distinct(rank);
            for (auto& r : distinct) r = r * 9 + 1000;
            CHECK(run_duplicate(L, distinct, a, b) == 0);
        }
    }
    printf("all checks passed\n");
    return 0;
}
