// ck_vecchia_trend.h -- one datum of the Vecchia likelihood with a GLS trend (ck_loglik_vecchia_trend, include/cokrige.h): from
// the datum's local solve with the trend rows riding along (mu = v . y, v . v and g_j = v . U_j) to the row r_t = (e_t, f_t) / s_t
// whose Gram matrix G = sum_t r_t r_t^T = [[yy, b^T], [b, A]] holds everything the GLS step needs, and the totals built from it.
// Compiles for the host and for the device: k_vecchia_trend_terms (ck_local.hip) runs it once per datum;
// tests/host_vecchia_trend_shim.cpp runs the same lines with g++ so that the rules can be checked against numpy without a GPU.
#pragma once

#include "ck_vecchia.h"

#define CK_VT_PMAX 16                                        // trend columns of both processes (2 CK_TREND_PMAX)
#define CK_VT_ROW (CK_VT_PMAX + 1)                           // entries of a row at most
#define CK_VT_NTRI 156                                       // the lower triangle of G, 17 * 18 / 2 = 153, in 12 groups of 13 columns

// (z, mu, vv, prior, noise, k): as ck_vecchia_term, which gives mean, var, logv, quad and the return value.  x: the datum's p
// regressors (x[j * xs]: row t of X); g: the p dots v . U_j of its solve, read only when k > 0.
//   e = z - mean,  f_j = x_j - g_j  (k == 0: f_j = x_j),  row = (e, f_0 .. f_{p-1}) / sqrt(var)
// A datum without a term (return 1) has a row of zeros: it adds nothing to G.
CK_HD int ck_vecchia_trend_row(double z, double mu, double vv, double prior, double noise, int k, int p, const double* x, long xs,
                               const double* g, double* mean, double* var, double* logv, double* quad, double* row) {
    const int bad = ck_vecchia_term(z, mu, vv, prior, noise, k, mean, var, logv, quad);
    if (bad) {
        for (int j = 0; j <= p; ++j) row[j] = 0.0;
        return 1;
    }
    const double rs = 1.0 / sqrt(*var);
    row[0] = (z - *mean) * rs;
    for (int j = 0; j < p; ++j) row[1 + j] = (k > 0 ? x[j * xs] - g[j] : x[j * xs]) * rs;
    return 0;
}

// entry e of the lower triangle of G -> (r, c), r >= c, rows first: G[0][0] = yy, G[1 + j][0] = b_j, G[1 + j][1 + l] = A_jl
CK_HD void ck_vecchia_trend_pair(int e, int* r, int* c) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    *r = a;
    *c = e - a * (a + 1) / 2;
}

// Q = yy - b . beta, the terms in their order
CK_HD double ck_vecchia_trend_q(int p, double yy, const double* b, const double* beta) {
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += b[j] * beta[j];
    return yy - s;
}

// profile:  l_P = -1/2 [N log 2 pi + sum log s^2 + Q];   reml:  l_R = -1/2 [(N - p) log 2 pi + sum log s^2 + log|A| + Q]
CK_HD double ck_vecchia_trend_total(int64_t n, int p, int reml, double sum_logv, double logdet_a, double q) {
    return reml ? ck_vecchia_total(n - p, sum_logv + logdet_a, q) : ck_vecchia_total(n, sum_logv, q);
}

// the conditional mean of the observation under the fitted trend: mean + f . beta, f as in the row
CK_HD double ck_vecchia_trend_mean(double mean, int k, int p, const double* x, long xs, const double* g, const double* beta) {
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += (k > 0 ? x[j * xs] - g[j] : x[j * xs]) * beta[j];
    return mean + s;
}
