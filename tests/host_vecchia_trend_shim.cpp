// TEST-ONLY shim: a datum's row of the Vecchia likelihood with a GLS trend (csrc/ck_vecchia_trend.h), the fixed-order Gram
// matrix and the host GLS step compiled for the host (tests/test_vecchia_trend_host.py; no GPU).
#include "host_vecchia_trend.h"

extern "C" {
int shim_vecchia_trend_row(double z, double mu, double vv, double prior, double noise, int k, int p, const double* x,
                           const double* g, double* out4, double* row) {
    return ck_vecchia_trend_row(z, mu, vv, prior, noise, k, p, x, 1, g, &out4[0], &out4[1], &out4[2], &out4[3], row);
}
void shim_vecchia_trend_gram(long n, int p, const double* rows, double* tri) { host_vecchia_trend_gram(n, p, rows, tri); }
long long shim_vecchia_trend_fit(long n, int p, int reml, const double* z, const double* mu, const double* vv, const double* prior,
                                 const double* noise, const int* cnt2, const double* x, const double* g, double tol, double* out5,
                                 double* beta, double* cov, double* mean, double* var) {
    return host_vecchia_trend_fit(n, p, reml, z, mu, vv, prior, noise, cnt2, x, g, tol, out5, beta, cov, mean, var);
}
}
