// TEST-ONLY: k_vecchia_info's steps for one datum, serially on the host, on the lines of csrc/ck_vecchia_info.h (the entry rule
// of the product, the variance, the combination, the mirror and the rule for slots that are not live): the Cholesky with the c
// row riding along, v . v, the back substitution to b = -w, the product U = D b over the full square of the set plus the datum,
// q = b . U, the forward substitution Y = L^-1 U column by column as the kernel's waves run it, the 91 sums.  Euclidean sites.
// Used by host_vecchia_info_shim.cpp (against numpy) and host_vecchia_info_sanitize_main.cpp (under the sanitizers).
#pragma once
#include <math.h>

#include <vector>

#include "ck_vecchia_info.h"
#include "host_vecchia_grad.h"   // host_vg_model

// One datum.  xy: (k + 1) x 2 sites, the datum last; proc: their processes; S: k x k local covariance (row-major, the noise on
// its diagonal); c: k; dvar: k + 1 raw variances or null; zt only decides whether a term exists.  out169: I_t, 13 x 13.
// Returns 1 for a datum without a term (NaN in the live block).
inline int host_vecchia_info(const CkVecchiaModel& V, int k, const double* xy, const int* proc, const double* S_in, const double* c,
                             double zt, double prior, double own, const double* dvar, double* out169) {
    const int ld = k > 0 ? k : 1;
    std::vector<double> S((size_t)(k + 1) * ld, 0.0);
    for (int a = 0; a < k; ++a) {
        for (int b = 0; b <= a; ++b) S[(size_t)a * ld + b] = S_in[(size_t)a * k + b];
        S[(size_t)k * ld + a] = c[a];
    }
    int fail = 0;
    for (int j = 0; j < k && !fail; ++j) {
        const double piv = S[(size_t)j * ld + j];
        if (!(piv > 0.0)) {
            fail = 1;
            break;
        }
        const double rd = 1.0 / sqrt(piv);
        for (int a = j + 1; a < k + 1; ++a) S[(size_t)a * ld + j] *= rd;
        S[(size_t)j * ld + j] = sqrt(piv);
        for (int a = j + 1; a < k + 1; ++a)
            for (int b = j + 1; b < k && b <= a; ++b) S[(size_t)a * ld + b] -= S[(size_t)a * ld + j] * S[(size_t)b * ld + j];
    }
    double vv = 0.0, s2 = 0.0;
    for (int a = 0; a < k; ++a) vv += S[(size_t)k * ld + a] * S[(size_t)k * ld + a];
    double tri[CK_VI_NTRI] = {};
    if (ck_vecchia_info_var(zt, fail ? NAN : 0.0, vv, prior, own, k, &s2)) {
        ck_vecchia_info_mirror(tri, V.live, 1, out169);
        return 1;
    }
    std::vector<double> bv((size_t)k + 1, 1.0);   // b = (-w, 1)
    double* xv = &S[(size_t)k * ld];
    for (int j = k - 1; j >= 0; --j) {
        const double vj = xv[j] / S[(size_t)j * ld + j];
        xv[j] = vj;
        for (int a = 0; a < j; ++a) xv[a] -= S[(size_t)j * ld + a] * vj;
    }
    for (int a = 0; a < k; ++a) bv[a] = -xv[a];
    // U = D b: row a's 13 sums over the entries q of the full square
    std::vector<double> U((size_t)CK_VI_NPAR * (k + 1), 0.0);
    for (int a = 0; a <= k; ++a) {
        double row[CK_VI_NPAR] = {};
        for (int q = 0; q <= k; ++q) {
            const double h = a == q ? 0.0 : ck_euclid(xy[2 * a], xy[2 * a + 1], xy[2 * q], xy[2 * q + 1]);
            ck_vecchia_info_entry(row, V, proc[a], proc[q], a == q, h, bv[q], a == q && dvar ? dvar[a] : 0.0);
        }
        for (int s = 0; s < CK_VI_NPAR; ++s) U[(size_t)s * (k + 1) + a] = row[s];
    }
    double qv[CK_VI_NPAR];
    for (int s = 0; s < CK_VI_NPAR; ++s) {
        double* x = &U[(size_t)s * (k + 1)];
        double q = 0.0;
        for (int a = 0; a <= k; ++a) q += bv[a] * x[a];
        qv[s] = q;
        for (int j = 0; j < k; ++j) {   // the wave's steps: entry j is divided, the entries behind it updated
            const double xj = x[j] / S[(size_t)j * ld + j];
            x[j] = xj;
            for (int a = j + 1; a < k; ++a) x[a] -= S[(size_t)a * ld + j] * xj;
        }
    }
    for (int e = 0; e < CK_VI_NTRI; ++e) {
        int j, kk;
        ck_vg_pair_of(e, &j, &kk);
        double yy = 0.0;
        for (int a = 0; a < k; ++a) yy += U[(size_t)j * (k + 1) + a] * U[(size_t)kk * (k + 1) + a];
        tri[e] = ck_vecchia_info_combine(V, j, kk, yy, qv[j], qv[kk], s2);
    }
    ck_vecchia_info_mirror(tri, V.live, 0, out169);
    return 0;
}
