// TEST-ONLY: the Vecchia likelihood with a GLS trend on the host -- the rows of csrc/ck_vecchia_trend.h, the fixed-order Gram
// matrix of k_vecchia_trend_gram and its tree (csrc/ck_local.hip) driven serially the way workgroups of 256 threads drive them,
// then the host GLS step of ck_loglik_vecchia_trend (csrc/ck_host.cpp: ck_host_gls).  Shared by
// tests/host_vecchia_trend_shim.cpp and tests/host_vecchia_trend_sanitize_main.cpp.
#pragma once

#include <vector>

#include "ck_host.h"
#include "ck_vecchia_trend.h"
#include "host_vecchia_terms.h"

// G = R^T R of n rows of 1 + p doubles: tri (CK_VT_NTRI) = its lower triangle in ck_vecchia_trend_pair's order
static inline void host_vecchia_trend_gram(long n, int p, const double* rows, double* tri) {
    const int w = p + 1, ntri = w * (w + 1) / 2;
    const long nblk = (n + HV_TPB - 1) / HV_TPB;
    std::vector<double> part((size_t)(nblk * CK_VT_NTRI), 0.0);
    for (long blk = 0; blk < nblk; ++blk)
        for (int e = 0; e < ntri; ++e) {
            int r, c;
            ck_vecchia_trend_pair(e, &r, &c);
            double acc = 0.0;
            for (int t = 0; t < HV_TPB; ++t) {
                const long s = blk * HV_TPB + t;
                if (s < n) acc += rows[s * w + r] * rows[s * w + c];   // (the device stages zeros behind the last row)
            }
            part[(size_t)(blk * CK_VT_NTRI + e)] = acc;
        }
    for (int e = 0; e < CK_VT_NTRI; ++e) {   // vg_tree over the workgroups' partial sums
        double red[HV_TPB];
        for (int tid = 0; tid < HV_TPB; ++tid) {
            red[tid] = 0.0;
            for (long b = tid; b < nblk; b += HV_TPB) red[tid] += part[(size_t)(b * CK_VT_NTRI + e)];
        }
        for (int s = HV_TPB / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) red[t] += red[t + s];
        tri[e] = red[0];
    }
}

// x, g: n x p (a datum's regressors and dots); noise may be null.  out5, beta (p), cov (p x p): NaN when a datum has no term;
// mean (mu_t + f_t . beta), var: n each.  Returns 1 + the first datum without a term, 0, or -(1 + c) when column c of the design
// is rank deficient.
static inline long long host_vecchia_trend_fit(long n, int p, int reml, const double* z, const double* mu, const double* vv,
                                               const double* prior, const double* noise, const int* cnt2, const double* x,
                                               const double* g, double tol, double* out5, double* beta, double* cov, double* mean,
                                               double* var) {
    std::vector<double> rows((size_t)(n * (p + 1)));
    double out3[3];
    const long long first_bad = host_vecchia_terms(n, z, mu, vv, prior, noise, cnt2, mean, var, out3);
    for (long t = 0; t < n; ++t) {
        double m, s2, lv, qd;
        ck_vecchia_trend_row(z[t], mu[t], vv[t], prior[t], noise ? noise[t] : 0.0, cnt2[2 * t] + cnt2[2 * t + 1], p, x + t * p, 1,
                             g + t * p, &m, &s2, &lv, &qd, &rows[(size_t)(t * (p + 1))]);
    }
    double tri[CK_VT_NTRI];
    host_vecchia_trend_gram(n, p, rows.data(), tri);
    for (int k = 0; k < 5; ++k) out5[k] = NAN;
    for (int k = 0; k < p; ++k) beta[k] = NAN;
    for (int k = 0; k < p * p; ++k) cov[k] = NAN;
    if (first_bad) return first_bad;
    std::vector<double> A((size_t)(p * p)), b((size_t)p);
    for (int e = 0; e < (p + 1) * (p + 2) / 2; ++e) {
        int r, c;
        ck_vecchia_trend_pair(e, &r, &c);
        if (r > 0 && c == 0) b[(size_t)(r - 1)] = tri[e];
        if (c > 0) A[(size_t)((r - 1) * p + c - 1)] = A[(size_t)((c - 1) * p + r - 1)] = tri[e];
    }
    double logdet = 0.0;
    const int bad = ck_host_gls(p, A.data(), b.data(), tol, nullptr, beta, cov, &logdet, nullptr);
    if (bad) return -(long long)bad;
    const double q = ck_vecchia_trend_q(p, tri[0], b.data(), beta);
    out5[0] = ck_vecchia_trend_total(n, p, reml, out3[1], logdet, q);
    out5[1] = out3[1];
    out5[2] = logdet;
    out5[3] = q;
    out5[4] = tri[0];
    for (long t = 0; t < n; ++t)
        mean[t] = ck_vecchia_trend_mean(mean[t], cnt2[2 * t] + cnt2[2 * t + 1], p, x + t * p, 1, g + t * p, beta);
    return 0;
}
