// TEST-ONLY shim: the Matern derivative functions of csrc/ck_math.h (the log-likelihood gradient) compiled for the host
// with g++, so that tests/test_host_matern_grad.py can check them against scipy without a GPU.  Never linked into the
// product library.
#include "ck_model.h"

extern "C" {
// D(x) = 2^(1-nu) / Gamma(nu) x^nu K_(nu-1)(x) for an array of scaled lags
void shim_dlen_scaled(double nu, const double* s, long n, double* out) {
    CkMatern m;
    ck_matern_prepare(nu, 1.0, 1.0, 0.0, &m);
    for (long i = 0; i < n; ++i) out[i] = ck_matern_dlen_scaled(m, s[i]);
}
// (M, dM/dnu, dM/dell) at lags h for one block, with the nu +- dnu, nu +- 2 dnu blocks prepared as the library prepares them
void shim_grad(double nu, double len_scale, const double* h, long n, double* out3) {
    CkMatern m, mv[4];
    const double d = ck_matern_dnu_step(nu);
    const double off[4] = {-2.0, -1.0, 1.0, 2.0};
    ck_matern_prepare(nu, len_scale, 1.0, 0.0, &m);
    for (int k = 0; k < 4; ++k) ck_matern_prepare(nu + off[k] * d, len_scale, 1.0, 0.0, &mv[k]);
    for (long i = 0; i < n; ++i) {
        const CkMaternGrad g = ck_matern_grad(m, mv, d, h[i]);
        out3[3 * i] = g.M;
        out3[3 * i + 1] = g.dnu;
        out3[3 * i + 2] = g.dlen;
    }
}
}
