// TEST-ONLY program: the rows, the fixed-order Gram matrix and the host GLS step of the Vecchia likelihood with a trend
// (csrc/ck_vecchia_trend.h, csrc/ck_host.cpp) under -fsanitize=address,undefined (tests/test_vecchia_trend_host.py builds and
// runs it; CPU only), against plain loops in long double.
#include <math.h>
#include <stdio.h>

#include <random>

#include "host_vecchia_trend.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

// n data with p regressors, every `empty_every`-th with an empty set; bad >= 0: that datum gets v . v beyond its prior variance;
// dup: the last regressor repeats the first (a rank-deficient design)
static int run(long n, int p, int empty_every, long bad, bool with_noise, bool dup) {
    std::mt19937_64 rng((unsigned long long)n * 7 + (unsigned long long)p);
    std::normal_distribution<double> G(0.0, 1.0);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const size_t N = (size_t)n, P = (size_t)p;
    std::vector<double> z(N), mu(N), vv(N), prior(N), noise(N), mean(N), var(N), x(N * P + 1), g(N * P + 1);
    std::vector<int> cnt(2 * N);
    std::vector<long double> Gm((P + 1) * (P + 1), 0.0L);
    long double s1 = 0;
    for (long t = 0; t < n; ++t) {
        const size_t T = (size_t)t;
        z[T] = G(rng);
        mu[T] = G(rng);
        prior[T] = 1.02;
        noise[T] = with_noise ? 0.5 * U(rng) : 0.0;
        vv[T] = 0.99 * U(rng);
        const bool empty = empty_every > 0 && t % empty_every == 0 && t != bad;
        cnt[2 * T] = empty ? 0 : 1 + (int)(t % 5);
        cnt[2 * T + 1] = empty ? 0 : (int)(t % 3);
        for (int j = 0; j < p; ++j) {
            x[T * P + (size_t)j] = j == 0 ? 1.0 : G(rng);
            g[T * P + (size_t)j] = empty ? NAN : 0.3 * G(rng);   // an empty set's dots are never read
        }
        if (dup && p > 1) {
            x[T * P + P - 1] = x[T * P];
            g[T * P + P - 1] = g[T * P];
        }
        if (empty) mu[T] = NAN;   // never read
        if (t == bad) vv[T] = 2.0;
        const long double m = empty ? 0.0L : (long double)mu[T];
        const long double v = (long double)prior[T] + noise[T] - (empty ? 0.0L : (long double)vv[T]);
        if (t == bad) continue;
        s1 += logl(v);
        std::vector<long double> r(P + 1);
        r[0] = ((long double)z[T] - m) / sqrtl(v);
        for (size_t j = 0; j < P; ++j) r[1 + j] = ((long double)x[T * P + j] - (empty ? 0.0L : (long double)g[T * P + j])) / sqrtl(v);
        for (size_t a = 0; a <= P; ++a)
            for (size_t b = 0; b <= P; ++b) Gm[a * (P + 1) + b] += r[a] * r[b];
    }
    // the fixed-order Gram matrix on rows of its own
    {
        std::vector<double> rows(N * (P + 1)), tri(CK_VT_NTRI);
        for (double& e : rows) e = G(rng);
        host_vecchia_trend_gram(n, p, rows.data(), tri.data());
        for (int e = 0; e < (p + 1) * (p + 2) / 2; ++e) {
            int r, c;
            ck_vecchia_trend_pair(e, &r, &c);
            CHECK(r >= c && r <= p);
            long double acc = 0;
            for (size_t t = 0; t < N; ++t) acc += (long double)rows[t * (P + 1) + (size_t)r] * rows[t * (P + 1) + (size_t)c];
            CHECK(fabsl(tri[(size_t)e] - acc) <= 1e-12L * (fabsl(acc) + (long double)n));
        }
        for (int e = (p + 1) * (p + 2) / 2; e < CK_VT_NTRI; ++e) CHECK(tri[(size_t)e] == 0.0);
    }
    double out5[5];
    std::vector<double> beta(P + 1), cov(P * P + 1);
    const long long rc = host_vecchia_trend_fit(n, p, 0, z.data(), mu.data(), vv.data(), prior.data(), with_noise ? noise.data() : nullptr,
                                                cnt.data(), x.data(), g.data(), 1e-10, out5, beta.data(), cov.data(), mean.data(),
                                                var.data());
    if (bad >= 0) {
        CHECK(rc == bad + 1);
        for (int k = 0; k < 5; ++k) CHECK(out5[k] != out5[k]);
        for (int j = 0; j < p; ++j) CHECK(beta[(size_t)j] != beta[(size_t)j]);
        return 0;
    }
    if (dup && p > 1) {
        CHECK(rc == -(long long)p);   // the last column is the first again
        return 0;
    }
    CHECK(rc == 0);
    CHECK(fabsl(out5[1] - s1) <= 1e-12L * (fabsl(s1) + (long double)n));
    CHECK(fabsl(out5[4] - Gm[0]) <= 1e-12L * (fabsl(Gm[0]) + (long double)n));
    // A beta = b and Q = yy - b . beta in long double
    long double bb = 0;
    for (size_t j = 0; j < P; ++j) {
        long double acc = 0;
        for (size_t l = 0; l < P; ++l) acc += Gm[(1 + j) * (P + 1) + 1 + l] * beta[l];
        CHECK(fabsl(acc - Gm[(1 + j) * (P + 1)]) <= 1e-9L * (fabsl(Gm[(1 + j) * (P + 1)]) + (long double)n));
        bb += Gm[(1 + j) * (P + 1)] * beta[j];
    }
    CHECK(fabsl(out5[3] - (Gm[0] - bb)) <= 1e-10L * (fabsl(Gm[0]) + (long double)n));
    const long double l = -0.5L * ((long double)n * logl(2.0L * acosl(-1.0L)) + s1 + (Gm[0] - bb));
    CHECK(fabsl(out5[0] - l) <= 1e-10L * (fabsl(l) + (long double)n));
    if (p == 0) CHECK(out5[2] == 0.0 && out5[3] == out5[4]);
    return 0;
}

int main() {
    for (long n : {1L, 17L, 255L, 256L, 257L, 65537L})   // one block, block edges, more blocks than threads
        for (int p : {0, 1, 2, 6, 16}) {
            if (n < 4 * p) continue;   // fewer data than regressors: the design is rank deficient by construction
            CHECK(run(n, p, 0, -1, false, false) == 0);
            CHECK(run(n, p, 3, -1, true, false) == 0);
        }
    CHECK(run(1000, 6, 4, 0, false, false) == 0);
    CHECK(run(1000, 6, 4, 999, true, false) == 0);
    CHECK(run(1000, 6, 4, -1, true, true) == 0);
    double out4[4], row[CK_VT_ROW], x[2] = {1.0, 0.5}, g[2] = {0.25, NAN};
    CHECK(ck_vecchia_trend_row(1.0, NAN, 0.0, 1.0, 0.0, 2, 2, x, 1, g, &out4[0], &out4[1], &out4[2], &out4[3], row) == 1);
    CHECK(row[0] == 0.0 && row[1] == 0.0 && row[2] == 0.0);   // no term: nothing for G
    CHECK(ck_vecchia_trend_row(1.0, NAN, NAN, 4.0, 0.0, 0, 2, x, 1, g, &out4[0], &out4[1], &out4[2], &out4[3], row) == 0);
    CHECK(row[0] == 0.5 && row[1] == 0.5 && row[2] == 0.25);  // an empty set: (z, x) / s
    printf("all checks passed\n");
    return 0;
}
