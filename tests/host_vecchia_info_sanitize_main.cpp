// TEST-ONLY program: one datum's share of the Vecchia information (csrc/ck_vecchia_info.h through host_vecchia_info.h) under
// -fsanitize=address,undefined (tests/test_vecchia_info_host.py builds and runs it; CPU only).  Sets of 0, 1, 2, 17 and 64 data,
// with and without noise: the matrix is finite, symmetric to the bit and obeys |I_jk| <= sqrt(I_jj I_kk); the empty set against
// its closed form; the rank-one part against central differences of the datum's variance; a masked call against the unmasked
// one; a variance of zero.
#include <math.h>
#include <stdio.h>

#include <random>

#include "host_vecchia_info.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Datum {
    int k;
    std::vector<double> xy, d;   // (k + 1) x 2, k + 1: the datum last
    std::vector<int> proc;
};

// the local system of the datum under par and the noise scales s2: S (k x k), c (k), prior, own
static void build(const Datum& D, const double* par, const double* s2, bool noise, std::vector<double>& S, std::vector<double>& c,
                  double* prior, double* own) {
    CkMatern blk5[15];
    CkVecchiaModel V;
    host_vg_model(2, par, 0x1fffu, blk5, &V);
    const int k = D.k;
    S.assign((size_t)k * k + 1, 0.0);
    c.assign((size_t)k + 1, 0.0);
    auto cov = [&](int a, int b) {
        const double h = a == b ? 0.0 : ck_euclid(D.xy[2 * a], D.xy[2 * a + 1], D.xy[2 * b], D.xy[2 * b + 1]);
        return ck_cov_entry(blk5[5 * (D.proc[a] + D.proc[b])], h, D.proc[a] == D.proc[b]);
    };
    for (int a = 0; a < k; ++a) {
        for (int b = 0; b < k; ++b) S[(size_t)a * k + b] = cov(a, b);
        if (noise) S[(size_t)a * k + a] += s2[D.proc[a]] * D.d[a];
        c[a] = cov(k, a);
    }
    *prior = cov(k, k);
    *own = noise ? s2[D.proc[k]] * D.d[k] : 0.0;
}

static int info_of(const Datum& D, const double* par, const double* s2, bool noise, unsigned live, double* out169) {
    std::vector<double> S, c;
    double prior, own;
    build(D, par, s2, noise, S, c, &prior, &own);
    CkMatern blk5[15];
    CkVecchiaModel V;
    host_vg_model(2, par, live, blk5, &V);
    return host_vecchia_info(V, D.k, D.xy.data(), D.proc.data(), S.data(), c.data(), 0.3, prior, own, noise ? D.d.data() : nullptr,
                             out169);
}

// the variance of the datum's term, prior + own - c^T S^-1 c, by a Cholesky of its own
static double var_of(const Datum& D, const double* par, const double* s2, bool noise) {
    std::vector<double> S, c;
    double prior, own;
    build(D, par, s2, noise, S, c, &prior, &own);
    const int k = D.k;
    double vv = 0.0;
    for (int j = 0; j < k; ++j) {   // left-looking, the c row solved along
        double dj = S[(size_t)j * k + j], x = c[j];
        for (int b = 0; b < j; ++b) {
            dj -= S[(size_t)j * k + b] * S[(size_t)j * k + b];
            x -= S[(size_t)j * k + b] * c[b];
        }
        dj = sqrt(dj);
        S[(size_t)j * k + j] = dj;
        for (int a = j + 1; a < k; ++a) {
            double s = S[(size_t)a * k + j];
            for (int b = 0; b < j; ++b) s -= S[(size_t)a * k + b] * S[(size_t)j * k + b];
            S[(size_t)a * k + j] = s / dj;
        }
        c[j] = x / dj;
        vv += c[j] * c[j];
    }
    return prior + own - vv;
}

static int run(int k, bool noise) {
    std::mt19937_64 rng((unsigned long long)k * 13 + noise);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    Datum D;
    D.k = k;
    for (int a = 0; a <= k; ++a) {
        D.xy.push_back(U(rng));
        D.xy.push_back(U(rng));
        D.proc.push_back(a == k ? 1 : a % 2);
        D.d.push_back(0.01 + 0.04 * U(rng));
    }
    if (k > 0) {   // a co-located partner of the other process: h == 0 without a nugget
        D.xy[0] = D.xy[2 * k];
        D.xy[1] = D.xy[2 * k + 1];
        D.proc[0] = 0;
    }
    double par[11] = {1.0, 0.8, 1.3, 1.7, 2.2, 0.2, 0.25, 0.3, 0.05, 0.03, 0.5};   // generic nu: the Temme branch
    double s2[2] = {0.7, 1.3};
    const int NP = CK_VI_NPAR;
    double I[169], masked[169];
    CHECK(info_of(D, par, s2, noise, 0x1fffu, I) == 0);
    for (int j = 0; j < NP; ++j)
        for (int q = 0; q < NP; ++q) {
            CHECK(isfinite(I[j * NP + q]) && I[j * NP + q] == I[q * NP + j]);
            CHECK(fabs(I[j * NP + q]) <= sqrt(I[j * NP + j] * I[q * NP + q]) * (1.0 + 1e-9) + 1e-300);
        }
    if (!noise)
        for (int j = 0; j < NP; ++j) CHECK(I[11 * NP + j] == 0.0 && I[12 * NP + j] == 0.0);
    const double v = var_of(D, par, s2, noise);
    if (k == 0) {   // the datum is of process 1: 1/2 q q^T / s^4 with q = (2 sigma_22, 1, d) in sigma_22, nugget_22, s_1
        double q[13] = {};
        q[1] = 2.0 * par[1];
        q[9] = 1.0;
        q[12] = noise ? D.d[0] : 0.0;
        for (int j = 0; j < NP; ++j)
            for (int r = 0; r < NP; ++r) CHECK(fabs(I[j * NP + r] - 0.5 * q[j] * q[r] / (v * v)) <= 1e-14 * (1.0 + fabs(I[j * NP + r])));
    }
    // I_jj >= 1/2 (ds2 / dtheta_j)^2 / s^4, with equality for the empty set: the rank-one part by differences of the variance
    for (int s : {0, 1, 6, 9, 10}) {
        const double h = 1e-5;
        double up[11], dn[11];
        for (int j = 0; j < 11; ++j) up[j] = dn[j] = par[j];
        up[s] += h;
        dn[s] -= h;
        const double q = (var_of(D, up, s2, noise) - var_of(D, dn, s2, noise)) / (2.0 * h);
        CHECK(I[s * NP + s] >= 0.5 * q * q / (v * v) * (1.0 - 1e-6) - 1e-12);
        if (k == 0) CHECK(fabs(I[s * NP + s] - 0.5 * q * q / (v * v)) <= 1e-6 * fmax(1.0, I[s * NP + s]));
    }
    const unsigned live = 0x1fffu & ~(1u << 2 | 1u << 3 | 1u << 4 | 1u << 12);   // the nu slots and one noise slot off
    CHECK(info_of(D, par, s2, noise, live, masked) == 0);
    for (int j = 0; j < NP; ++j)
        for (int q = 0; q < NP; ++q)
            CHECK(((live >> j & 1u) && (live >> q & 1u)) ? masked[j * NP + q] == I[j * NP + q] : masked[j * NP + q] == 0.0);
    return 0;
}

int main() {
    for (int k : {0, 1, 2, 17, 64}) {
        CHECK(run(k, false) == 0);
        CHECK(run(k, true) == 0);
    }
    // a duplicate of the datum as its only conditioning datum, no nugget, no noise: s^2 = 0
    Datum D;
    D.k = 1;
    D.xy = {0.3, 0.4, 0.3, 0.4};
    D.proc = {0, 0};
    D.d = {0.0, 0.0};
    double par[11] = {1.0, 0.8, 1.5, 1.5, 1.5, 0.2, 0.2, 0.2, 0.0, 0.0, 0.5};
    double s2[2] = {1.0, 1.0}, I[169];
    CHECK(info_of(D, par, s2, false, 0x7ffu, I) == 1);
    for (int j = 0; j < 13; ++j)
        for (int q = 0; q < 13; ++q) CHECK((j < 11 && q < 11) ? I[j * 13 + q] != I[j * 13 + q] : I[j * 13 + q] == 0.0);
    double v;
    CHECK(ck_vecchia_info_var(1.0, NAN, 0.1, 1.0, 0.0, 3, &v) == 1);                 // not positive definite
    CHECK(ck_vecchia_info_var(0.5, NAN, NAN, 2.0, 0.5, 0, &v) == 0 && v == 2.5);     // empty set: s^2 = prior + noise
    printf("all checks passed\n");
    return 0;
}
