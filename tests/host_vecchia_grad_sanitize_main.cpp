// TEST-ONLY program: one datum's score of the Vecchia gradient (csrc/ck_vecchia_grad.h through host_vecchia_grad.h) under
// -fsanitize=address,undefined (tests/test_vecchia_grad_host.py builds and runs it; CPU only).  Sets of 0, 1 and 64 data, with
// and without noise: the score against central differences of the datum's own term in sigma_11, len_scale_12, nugget_22, rho and
// the noise scales; a masked call against the unmasked one; a variance of zero.
#include <math.h>
#include <stdio.h>

#include <random>

#include "host_vecchia_grad.h"

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
    std::vector<double> z;       // k + 1
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

static int score_of(const Datum& D, const double* par, const double* s2, bool noise, unsigned live, double* out2, double* score) {
    std::vector<double> S, c;
    double prior, own;
    build(D, par, s2, noise, S, c, &prior, &own);
    CkMatern blk5[15];
    CkVecchiaModel V;
    host_vg_model(2, par, live, blk5, &V);
    return host_vecchia_score(V, D.k, D.xy.data(), D.proc.data(), S.data(), c.data(), D.z.data(), D.z[D.k], prior, own,
                              noise ? D.d.data() : nullptr, out2, score);
}

// the datum's term -1/2 (log s^2 + e^2 / s^2)
static double term_of(const Datum& D, const double* par, const double* s2, bool noise) {
    double out2[2] = {0.0, 0.0}, score[CK_VG_NPAR];
    std::vector<double> S, c;
    double prior, own;
    build(D, par, s2, noise, S, c, &prior, &own);
    score_of(D, par, s2, noise, 0x1fffu, out2, score);
    double m, v, lv, qd;
    ck_vecchia_term(D.z[D.k], out2[0], out2[1], prior, own, D.k, &m, &v, &lv, &qd);
    return -0.5 * (lv + qd);
}

static int run(int k, bool noise) {
    std::mt19937_64 rng((unsigned long long)k * 11 + noise);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> G(0.0, 1.0);
    Datum D;
    D.k = k;
    for (int a = 0; a <= k; ++a) {
        D.xy.push_back(U(rng));
        D.xy.push_back(U(rng));
        D.proc.push_back(a == k ? 1 : a % 2);
        D.z.push_back(G(rng));
        D.d.push_back(0.01 + 0.04 * U(rng));
    }
    if (k > 0) {   // a co-located partner of the other process: h == 0 without a nugget
        D.xy[0] = D.xy[2 * k];
        D.xy[1] = D.xy[2 * k + 1];
        D.proc[0] = 0;
    }
    double par[11] = {1.0, 0.8, 1.3, 1.7, 2.2, 0.2, 0.25, 0.3, 0.05, 0.03, 0.5};   // generic nu: the Temme branch
    double s2[2] = {0.7, 1.3};
    double out2[2] = {0.0, 0.0}, score[CK_VG_NPAR], masked[CK_VG_NPAR];
    CHECK(score_of(D, par, s2, noise, 0x1fffu, out2, score) == 0);
    for (int s = 0; s < CK_VG_NPAR; ++s) CHECK(isfinite(score[s]));
    if (!noise) CHECK(score[11] == 0.0 && score[12] == 0.0);
    if (k == 0) {
        for (int s : {0, 2, 3, 4, 5, 6, 7, 8, 10, 11}) CHECK(score[s] == 0.0);   // the datum is of process 1: sigma_22, nugget_22, s_1
        CHECK(score[1] != 0.0 && score[9] != 0.0 && (noise ? score[12] != 0.0 : score[12] == 0.0));
    }
    const int slots[4] = {0, 6, 9, 10};
    for (int s : slots) {
        const double h = 1e-5;
        double up[11], dn[11];
        for (int j = 0; j < 11; ++j) up[j] = dn[j] = par[j];
        up[s] += h;
        dn[s] -= h;
        const double fd = (term_of(D, up, s2, noise) - term_of(D, dn, s2, noise)) / (2.0 * h);
        CHECK(fabs(fd - score[s]) <= 1e-6 * fmax(1.0, fabs(fd)));
    }
    if (noise)
        for (int q = 0; q < 2; ++q) {
            const double h = 1e-5;
            double up[2] = {s2[0], s2[1]}, dn[2] = {s2[0], s2[1]};
            up[q] += h;
            dn[q] -= h;
            const double fd = (term_of(D, par, up, noise) - term_of(D, par, dn, noise)) / (2.0 * h);
            CHECK(fabs(fd - score[11 + q]) <= 1e-6 * fmax(1.0, fabs(fd)));
        }
    const unsigned live = 0x1fffu & ~(1u << 2 | 1u << 3 | 1u << 4 | 1u << 12);   // the nu slots and one noise slot off
    CHECK(score_of(D, par, s2, noise, live, out2, masked) == 0);
    for (int s = 0; s < CK_VG_NPAR; ++s) CHECK((live >> s & 1u) ? masked[s] == score[s] : masked[s] == 0.0);
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
    D.z = {0.2, -0.1};
    D.d = {0.0, 0.0};
    double par[11] = {1.0, 0.8, 1.5, 1.5, 1.5, 0.2, 0.2, 0.2, 0.0, 0.0, 0.5};
    double s2[2] = {1.0, 1.0}, out2[2], score[CK_VG_NPAR];
    CHECK(score_of(D, par, s2, false, 0x7ffu, out2, score) == 1);
    for (int s = 0; s < 11; ++s) CHECK(score[s] != score[s]);
    CHECK(score[11] == 0.0 && score[12] == 0.0);
    double w[2];
    CHECK(ck_vecchia_weights(1.0, NAN, 0.1, 1.0, 0.0, 3, &w[0], &w[1]) == 1 && w[0] != w[0]);   // not positive definite
    CHECK(ck_vecchia_weights(0.5, NAN, NAN, 2.0, 0.5, 0, &w[0], &w[1]) == 0 && w[1] == 0.2);   // empty set: e = z, s^2 = prior + noise
    printf("all checks passed\n");
    return 0;
}
