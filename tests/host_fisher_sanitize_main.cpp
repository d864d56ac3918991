// TEST-ONLY program: the REML correction and the operand -> parameter combination of the Fisher information
// (csrc/ck_host.cpp: ck_host_fisher_reml / _coef / _combine) under -fsanitize=address,undefined (tests/test_fisher_host.py
// builds and runs it; CPU only).  Exactly sized buffers: a read or write past an end is the sanitizer's to report.
#include <math.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "ck_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    std::mt19937_64 rng(3);
    std::normal_distribution<double> nd;
    const int NO = CK_HOST_FISHER_NOPS, NP = CK_HOST_FISHER_NPAR;
    for (int p : {1, 2, 6, 16}) {
        // D_a = d_a d_a^T (rank one), Sigma^-1 = identity on n sites: every term has a closed form
        const int n = 40;
        std::vector<double> X((size_t)n * p), d((size_t)NO * n);
        for (auto& x : X) x = nd(rng);
        for (auto& x : d) x = nd(rng);
        std::vector<double> A((size_t)p * p, 0.0), Y((size_t)NO * p * n), K((size_t)NO * p * NO * p), Gm((size_t)NO * p * p),
            T((size_t)NO * NO);
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j)
                for (int g = 0; g < n; ++g) A[(size_t)i * p + j] += X[(size_t)g * p + i] * X[(size_t)g * p + j];
        for (int a = 0; a < NO; ++a)   // Y_a = D_a H, H = X
            for (int j = 0; j < p; ++j) {
                double dot = 0.0;
                for (int g = 0; g < n; ++g) dot += d[(size_t)a * n + g] * X[(size_t)g * p + j];
                for (int g = 0; g < n; ++g) Y[((size_t)a * p + j) * n + g] = d[(size_t)a * n + g] * dot;
            }
        const int64_t ldk = (int64_t)NO * p;
        for (int r = 0; r < NO * p; ++r) {
            for (int c = 0; c < NO * p; ++c) {
                double s = 0.0;
                for (int g = 0; g < n; ++g) s += Y[(size_t)r * n + g] * Y[(size_t)c * n + g];
                K[(size_t)r * ldk + c] = s;
            }
            for (int j = 0; j < p; ++j) {
                double s = 0.0;
                for (int g = 0; g < n; ++g) s += Y[(size_t)r * n + g] * X[(size_t)g * p + j];
                Gm[(size_t)r * p + j] = s;
            }
        }
        for (int a = 0; a < NO; ++a)
            for (int b = 0; b < NO; ++b) {
                double dot = 0.0;
                for (int g = 0; g < n; ++g) dot += d[(size_t)a * n + g] * d[(size_t)b * n + g];
                T[(size_t)a * NO + b] = 0.5 * dot * dot;
            }
        CHECK(ck_host_fisher_reml(p, NO, A.data(), K.data(), ldk, Gm.data(), T.data()) == 0);
        for (int a = 0; a < NO; ++a)
            for (int b = 0; b < NO; ++b) CHECK(isfinite(T[(size_t)a * NO + b]) && T[(size_t)a * NO + b] == T[(size_t)b * NO + a]);
        for (int a = 0; a < NO; ++a) CHECK(T[(size_t)a * NO + a] >= -1e-9);
        std::vector<double> C((size_t)NP * NO), I((size_t)NP * NP);
        std::vector<unsigned char> live((size_t)NP, 1);
        live[3] = 0;
        ck_host_fisher_coef(2, 1.1, 0.9, -0.2, C.data());
        ck_host_fisher_combine(C.data(), T.data(), live.data(), I.data());
        for (int k = 0; k < NP; ++k) CHECK(I[(size_t)3 * NP + k] == 0.0 && I[(size_t)k * NP + 3] == 0.0);
        ck_host_fisher_coef(1, 1.1, 0.0, 0.0, C.data());
        ck_host_fisher_combine(C.data(), T.data(), live.data(), I.data());
        CHECK(I[0] > 0.0 && I[(size_t)5 * NP + 5] == 0.0);
    }
    // a singular A is reported, not divided by
    const double A2[4] = {1.0, 1.0, 1.0, 1.0};
    std::vector<double> K((size_t)(2 * NO) * (2 * NO), 0.0), Gm((size_t)(2 * NO) * 2, 0.0), T((size_t)NO * NO, 0.0);
    CHECK(ck_host_fisher_reml(2, NO, A2, K.data(), 2 * NO, Gm.data(), T.data()) == 2);
    CHECK(ck_host_fisher_reml(0, NO, nullptr, nullptr, 0, nullptr, T.data()) == 0);
    printf("all checks passed\n");
    return 0;
}
