// TEST-ONLY program: the terms of the Vecchia likelihood (csrc/ck_vecchia.h) and their fixed-order sums under
// -fsanitize=address,undefined (tests/test_vecchia_host.py builds and runs it; CPU only), against a plain loop in long double.
#include <math.h>
#include <stdio.h>

#include <random>

#include "host_vecchia_terms.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

// n data, every `empty_every`-th with an empty set; bad >= 0: that datum gets v . v beyond its prior variance
static int run(long n, int empty_every, long bad, bool with_noise) {
    std::mt19937_64 rng((unsigned long long)n * 7 + 1);
    std::normal_distribution<double> G(0.0, 1.0);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> z((size_t)n), mu((size_t)n), vv((size_t)n), prior((size_t)n), noise((size_t)n), mean((size_t)n), var((size_t)n);
    std::vector<int> cnt((size_t)(2 * n));
    long double s1 = 0, s2 = 0;
    for (long t = 0; t < n; ++t) {
        z[(size_t)t] = G(rng);
        mu[(size_t)t] = G(rng);
        prior[(size_t)t] = 1.02;
        noise[(size_t)t] = with_noise ? 0.5 * U(rng) : 0.0;
        vv[(size_t)t] = 0.99 * U(rng);
        const bool empty = empty_every > 0 && t % empty_every == 0;
        cnt[(size_t)(2 * t)] = empty ? 0 : 1 + (int)(t % 5);
        cnt[(size_t)(2 * t + 1)] = empty ? 0 : (int)(t % 3);
        if (empty) mu[(size_t)t] = NAN;   // never read
        if (t == bad) {
            vv[(size_t)t] = 2.0;
            cnt[(size_t)(2 * t)] = 3;
            mu[(size_t)t] = 0.1;
        }
        const long double m = empty && t != bad ? 0.0L : (long double)mu[(size_t)t];
        const long double v = (long double)prior[(size_t)t] + noise[(size_t)t] - (empty && t != bad ? 0.0L : (long double)vv[(size_t)t]);
        s1 += logl(v);
        s2 += ((long double)z[(size_t)t] - m) * ((long double)z[(size_t)t] - m) / v;
    }
    double out3[3];
    const long long info = host_vecchia_terms(n, z.data(), mu.data(), vv.data(), prior.data(), with_noise ? noise.data() : nullptr,
                                              cnt.data(), mean.data(), var.data(), out3);
    if (bad >= 0) {
        CHECK(info == bad + 1);
        CHECK(out3[0] != out3[0] && out3[1] != out3[1] && out3[2] != out3[2]);
        CHECK(var[(size_t)bad] < 0.0);
        return 0;
    }
    CHECK(info == 0);
    CHECK(fabsl(out3[1] - s1) <= 1e-12L * (fabsl(s1) + (long double)n));
    CHECK(fabsl(out3[2] - s2) <= 1e-12L * (fabsl(s2) + (long double)n));
    const long double l = -0.5L * ((long double)n * logl(2.0L * acosl(-1.0L)) + s1 + s2);
    CHECK(fabsl(out3[0] - l) <= 1e-12L * (fabsl(l) + (long double)n));
    for (long t = 0; t < n; ++t)
        if (cnt[(size_t)(2 * t)] + cnt[(size_t)(2 * t + 1)] == 0) CHECK(mean[(size_t)t] == 0.0 && var[(size_t)t] == prior[(size_t)t] + (with_noise ? noise[(size_t)t] : 0.0));
    return 0;
}

int main() {
    for (long n : {1L, 2L, 255L, 256L, 257L, 65536L, 65537L, 70001L}) {   // one block, block edges, more blocks than threads
        CHECK(run(n, 0, -1, false) == 0);
        CHECK(run(n, 3, -1, true) == 0);
    }
    CHECK(run(1000, 4, 0, false) == 0);
    CHECK(run(1000, 4, 999, true) == 0);
    CHECK(run(70001, 0, 66000, true) == 0);
    double out4[4];
    CHECK(ck_vecchia_term(1.0, NAN, 0.0, 1.0, 0.0, 2, &out4[0], &out4[1], &out4[2], &out4[3]) == 1);   // not positive definite
    CHECK(ck_vecchia_term(1.0, 0.5, 1.0, 1.0, 0.0, 2, &out4[0], &out4[1], &out4[2], &out4[3]) == 1 && out4[1] == 0.0);   // s^2 = 0
    CHECK(ck_vecchia_term(1.0, NAN, NAN, 1.0, 0.25, 0, &out4[0], &out4[1], &out4[2], &out4[3]) == 0 && out4[0] == 0.0 && out4[1] == 1.25);
    printf("all checks passed\n");
    return 0;
}
