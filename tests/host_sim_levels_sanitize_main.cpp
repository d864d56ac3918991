// TEST-ONLY program: the level planner of the local conditional simulation (csrc/ck_host.cpp: ck_host_sim_levels) under
// -fsanitize=address,undefined (tests/test_local_sim_host.py builds and runs it; CPU only).
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

// every output against its definition
static int run(int64_t m, int ld, const std::vector<int32_t>& pos, const std::vector<int32_t>& ns, const std::vector<int32_t>& nbr,
               int64_t want_levels) {
    CkSimLevels lv;
    const int64_t n = ck_host_sim_levels(m, ld, pos.data(), ns.data(), nbr.data(), &lv);
    CHECK(n >= 1 && (want_levels < 0 || n == want_levels));
    CHECK((int64_t)lv.level.size() == m && (int64_t)lv.order.size() == m && (int64_t)lv.off.size() == n + 1);
    CHECK(lv.off[0] == 0 && lv.off[(size_t)n] == m);
    std::vector<int32_t> at((size_t)m);
    for (int64_t t = 0; t < m; ++t) at[(size_t)pos[(size_t)t]] = (int32_t)t;
    for (int64_t t = 0; t < m; ++t) {
        int32_t want = 1;
        for (int32_t j = 0; j < ns[(size_t)t]; ++j) want = std::max(want, 1 + lv.level[(size_t)at[(size_t)nbr[(size_t)(t * ld + j)]]]);
        CHECK(lv.level[(size_t)t] == want);
    }
    std::vector<char> seen((size_t)m, 0);
    for (int64_t l = 1; l <= n; ++l) {
        CHECK(lv.off[(size_t)l] > lv.off[(size_t)(l - 1)]);   // no level is empty
        for (int64_t e = lv.off[(size_t)(l - 1)]; e < lv.off[(size_t)l]; ++e) {
            const int32_t t = lv.order[(size_t)e];
            CHECK(t >= 0 && t < m && !seen[(size_t)t] && lv.level[(size_t)t] == l);
            seen[(size_t)t] = 1;
            if (e > lv.off[(size_t)(l - 1)]) CHECK(pos[(size_t)lv.order[(size_t)(e - 1)]] < pos[(size_t)t]);
        }
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(11);
    const int ld = 64;
    for (int64_t m : {1, 2, 63, 64, 65, 257, 3000}) {
        std::vector<int32_t> pos((size_t)m);
        std::iota(pos.begin(), pos.end(), 0);
        std::shuffle(pos.begin(), pos.end(), rng);
        std::vector<int32_t> ns((size_t)m, 0), nbr((size_t)(m * ld), -1);
        CHECK(run(m, ld, pos, ns, nbr, 1) == 0);   // no site-neighbours: one level
        for (int64_t t = 0; t < m; ++t)            // a chain: every site on its predecessor, m levels
            if (pos[(size_t)t] > 0) {
                ns[(size_t)t] = 1;
                nbr[(size_t)(t * ld)] = pos[(size_t)t] - 1;
            }
        CHECK(run(m, ld, pos, ns, nbr, m) == 0);
        for (int64_t t = 0; t < m; ++t) {          // random earlier positions, up to a full row
            const int32_t q = pos[(size_t)t];
            const int32_t k = (int32_t)std::min<int64_t>(q, (int64_t)(rng() % (uint64_t)(ld + 1)));
            ns[(size_t)t] = k;
            for (int32_t j = 0; j < k; ++j) nbr[(size_t)(t * ld + j)] = (int32_t)(rng() % (uint64_t)q);
        }
        CHECK(run(m, ld, pos, ns, nbr, -1) == 0);
        // refusals: a neighbour that is not earlier, a position twice
        CkSimLevels lv;
        if (m >= 2) {
            std::vector<int32_t> ns2(ns), nbr2(nbr);
            int64_t t = 0;
            while (pos[(size_t)t] != 0) ++t;       // the first site of the ordering can have no neighbour
            ns2[(size_t)t] = 1;
            nbr2[(size_t)(t * ld)] = 0;
            CHECK(ck_host_sim_levels(m, ld, pos.data(), ns2.data(), nbr2.data(), &lv) == -1 && lv.off[0] == t);
            std::vector<int32_t> pos2(pos);
            pos2[1] = pos2[0];
            CHECK(ck_host_sim_levels(m, ld, pos2.data(), ns.data(), nbr.data(), &lv) == -1 && lv.off[0] == 1);
        }
    }
    printf("all checks passed\n");
    return 0;
}
