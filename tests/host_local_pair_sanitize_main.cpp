// TEST-ONLY program: the host planning of both processes in the moving neighbourhood (csrc/ck_host.cpp: ck_host_sim_order,
// ck_host_sim_ext, ck_host_local_pair_needs) under -fsanitize=address,undefined (tests/test_local_pair_host.py builds and runs
// it; CPU only).
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <random>

#include "ck_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    std::mt19937_64 rng(11);
    const int64_t sizes[][2] = {{1, 0}, {0, 1}, {1, 1}, {3, 5}, {257, 2}, {64, 64}, {1000, 777}};
    for (const auto& sz : sizes) {
        const int64_t m[2] = {sz[0], sz[1]}, mt = sz[0] + sz[1];
        const int64_t n[2] = {37, 91}, N = n[0] + n[1];
        // ranks: a shuffled arithmetic progression (no permutation of 0 .. mt - 1: the sorting path), then a permutation
        for (int direct = 0; direct < 2; ++direct) {
            std::vector<int64_t> rank((size_t)mt);
            std::iota(rank.begin(), rank.end(), 0);
            std::shuffle(rank.begin(), rank.end(), rng);
            if (!direct)
                for (auto& r : rank) r = 7 * r - 100;
            CkSimSites S;
            CHECK(ck_host_sim_order(rank.data(), m, &S) == 0);
            CHECK((int64_t)S.pos.size() == mt);
            std::vector<int> at((size_t)mt, -1);
            for (int64_t t = 0; t < mt; ++t) {
                CHECK(S.pos[(size_t)t] >= 0 && S.pos[(size_t)t] < mt && at[(size_t)S.pos[(size_t)t]] == -1);
                at[(size_t)S.pos[(size_t)t]] = (int)t;
            }
            for (int64_t q = 1; q < mt; ++q) CHECK(rank[(size_t)at[(size_t)(q - 1)]] < rank[(size_t)at[(size_t)q]]);
            // the augmented layout: shuffled perms, process 1 behind padding
            const int64_t nc[2] = {n[0] + m[0], n[1] + m[1]};
            const int64_t n0p = (nc[0] + 63) / 64 * 64, npad = n0p + (nc[1] + 63) / 64 * 64;
            std::vector<int64_t> perm[2];
            for (int k = 0; k < 2; ++k) {
                perm[k].resize((size_t)nc[k]);
                std::iota(perm[k].begin(), perm[k].end(), 0);
                std::shuffle(perm[k].begin(), perm[k].end(), rng);
            }
            ck_host_sim_ext(2, n, m, n0p, npad, perm[0].data(), perm[1].data(), &S);
            CHECK((int64_t)S.ext.size() == npad && (int64_t)S.rs.size() == npad && (int64_t)S.rp.size() == mt);
            std::vector<int> seen((size_t)(N + mt), 0);
            for (int64_t g = 0; g < npad; ++g) {
                const bool valid = g < nc[0] || (g >= n0p && g < n0p + nc[1]);
                if (!valid) {
                    CHECK(S.ext[(size_t)g] == -1 && S.rs[(size_t)g] == INT32_MAX);
                    continue;
                }
                const int e = S.ext[(size_t)g];
                CHECK(e >= 0 && e < N + mt && ++seen[(size_t)e] == 1);
                const int k = g >= n0p;
                if (e < N) {
                    CHECK(S.rs[(size_t)g] == e && (k == 0 ? e < n[0] : e >= n[0]));
                } else {
                    CHECK(S.rs[(size_t)g] == N + S.pos[(size_t)(e - N)] && (k == 0 ? e - N < m[0] : e - N >= m[0]));
                }
            }
            for (int64_t t = 0; t < mt; ++t) CHECK(S.rp[(size_t)t] == N + S.pos[(size_t)t]);
            if (mt >= 2) {   // a duplicate rank names both stacked sites, the earlier first
                rank[(size_t)(mt - 1)] = rank[0];
                CkSimSites D;
                CHECK(ck_host_sim_order(rank.data(), m, &D) == -1 && D.dup[0] == 0 && D.dup[1] == mt - 1);
            }
        }
    }
    // one process: the second perm is null and never read
    {
        const int64_t m[2] = {9, 0}, n[2] = {20, 0};
        std::vector<int64_t> rank(9), perm(29);
        std::iota(rank.begin(), rank.end(), 0);
        std::iota(perm.begin(), perm.end(), 0);
        CkSimSites S;
        CHECK(ck_host_sim_order(rank.data(), m, &S) == 0);
        ck_host_sim_ext(1, n, m, 64, 64, perm.data(), nullptr, &S);
        CHECK(S.ext[19] == 19 && S.ext[20] == 20 && S.rs[28] == 20 + 8 && S.ext[29] == -1);
    }
    // the size classes with three extra rows
    {
        std::vector<int> cnt;
        for (int k = 0; k <= 200; ++k) cnt.push_back(k);
        for (int tile_min : {64, 0, 1000000}) {
            CkLocalNeeds nd;
            ck_host_local_pair_needs(cnt.data(), (int64_t)cnt.size(), 64, tile_min, &nd);
            const int k_hi = std::min(tile_min, 64);
            CHECK(nd.n_empty == 1 && nd.k_max == 200 && (int64_t)nd.tiled.size() == 200 - k_hi);
            for (long long x : nd.need) CHECK(x == 0);   // no slab class
            CkLocalPlan plan;
            ck_host_local_plan(cnt.data(), nd, 1 << 20, CK_LOCAL_PAIR_ROWS - 2, &plan);
            long long end = 0;
            for (const auto& tb : plan.tbatches) {
                long long at = 0;
                for (int64_t t = tb.first; t < tb.second; ++t) {
                    const CkLocalSys& s = plan.sys[(size_t)t];
                    CHECK(s.kq == (s.k + 3 + 63) / 64 * 64 && s.kq >= s.k + 3 && s.ld == s.kq + 128 && s.off == at);
                    at += ck_local_tiled_doubles(s.k, 1);
                    CHECK(at <= plan.slab_doubles);
                }
                CHECK(tb.first == end);
                end = tb.second;
            }
            CHECK(end == (long long)plan.sys.size());
        }
    }
    printf("all checks passed\n");
    return 0;
}
