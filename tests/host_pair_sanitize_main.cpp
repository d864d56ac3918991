// TEST-ONLY program: the stacked layout of the joint prediction of both processes (csrc/ck_host.cpp: ck_host_pair_plan,
// ck_host_pair_coincident) under -fsanitize=address,undefined (tests/test_pair_host.py builds and runs it; CPU only).
#include <stdio.h>

#include <random>

#include "ck_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

static std::vector<double> sites(std::mt19937_64& rng, int64_t m) {
    std::uniform_real_distribution<double> lat(25.0, 50.0), lon(-120.0, -70.0);
    std::vector<double> xy((size_t)(2 * m));
    for (int64_t k = 0; k < m; ++k) {
        xy[(size_t)(2 * k)] = lat(rng);
        xy[(size_t)(2 * k + 1)] = lon(rng);
    }
    return xy;
}

int main() {
    std::mt19937_64 rng(5);
    const int64_t sizes[][2] = {{0, 0}, {1, 1}, {0, 40}, {40, 0}, {63, 65}, {64, 64}, {65, 63}, {255, 256}, {300, 277}, {512, 130},
                                {5000, 3000}};
    for (const auto& sz : sizes)
        for (int so = 0; so < 2; ++so) {
            const int64_t m0 = sz[0], m1 = sz[1];
            const std::vector<double> a = sites(rng, m0), b = sites(rng, m1);
            CkPairPlan P;
            ck_host_pair_plan(a.data(), m0, b.data(), m1, so != 0, &P);
            CHECK(P.m0p == (m0 + 63) / 64 * 64 && P.rows == P.m0p + m1);
            CHECK((int64_t)P.cmap.size() == P.rows && (int64_t)P.row_of.size() == m0 + m1 && (int64_t)P.xy.size() == 2 * P.rows);
            CHECK(P.sorted[0] == (so && m0 >= CK_HOST_PAIR_SORT_MIN) && P.sorted[1] == (so && m1 >= CK_HOST_PAIR_SORT_MIN));
            std::vector<int> seen((size_t)(m0 + m1), 0);
            for (int64_t j = 0; j < P.rows; ++j) {
                const int c = P.cmap[(size_t)j];
                if (j >= m0 && j < P.m0p) {
                    CHECK(c == -1 && P.xy[(size_t)(2 * j)] == 0.0 && P.xy[(size_t)(2 * j + 1)] == 0.0);
                    continue;
                }
                CHECK(j < m0 ? (c >= 0 && c < m0) : (c >= m0 && c < m0 + m1));
                CHECK(P.row_of[(size_t)c] == j && ++seen[(size_t)c] == 1);
                const double* src = c < m0 ? &a[(size_t)(2 * c)] : &b[(size_t)(2 * (c - m0))];
                CHECK(P.xy[(size_t)(2 * j)] == src[0] && P.xy[(size_t)(2 * j + 1)] == src[1]);
            }
            // no coincidence among distinct random sites, whatever is masked
            std::vector<unsigned char> mask((size_t)P.rows, 0);
            for (int64_t j = m0; j < P.m0p; ++j) mask[(size_t)j] = 2;
            CHECK(ck_host_pair_coincident(P, a.data(), b.data(), mask.data()) == -1);
        }
    // coincidence: inside a process it stops at the later row, across the processes it does not
    {
        const int64_t m0 = 70, m1 = 300;
        std::vector<double> a = sites(rng, m0), b = sites(rng, m1);
        b[2 * 17] = a[2 * 3];   // process 1's site 17 on process 0's site 3
        b[2 * 17 + 1] = a[2 * 3 + 1];
        CkPairPlan P;
        ck_host_pair_plan(a.data(), m0, b.data(), m1, true, &P);
        std::vector<unsigned char> mask((size_t)P.rows, 0);
        for (int64_t j = m0; j < P.m0p; ++j) mask[(size_t)j] = 2;
        CHECK(ck_host_pair_coincident(P, a.data(), b.data(), mask.data()) == -1);
        b[2 * 200] = b[2 * 17];   // process 1's sites 17 and 200 coincide
        b[2 * 200 + 1] = b[2 * 17 + 1];
        ck_host_pair_plan(a.data(), m0, b.data(), m1, true, &P);
        const int64_t later = std::max(P.row_of[(size_t)(m0 + 17)], P.row_of[(size_t)(m0 + 200)]);
        CHECK(ck_host_pair_coincident(P, a.data(), b.data(), mask.data()) == later);
        mask[(size_t)P.row_of[(size_t)(m0 + 17)]] = 1;   // one of them deflated: nothing stops
        CHECK(ck_host_pair_coincident(P, a.data(), b.data(), mask.data()) == -1);
        a[2 * 60] = a[2 * 3];   // process 0 wins: its rows come first
        a[2 * 60 + 1] = a[2 * 3 + 1];
        mask[(size_t)P.row_of[(size_t)(m0 + 17)]] = 0;
        ck_host_pair_plan(a.data(), m0, b.data(), m1, true, &P);
        CHECK(ck_host_pair_coincident(P, a.data(), b.data(), mask.data()) == 60);
    }
    printf("all checks passed\n");
    return 0;
}
