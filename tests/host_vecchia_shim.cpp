// TEST-ONLY shim: a term of the Vecchia likelihood (csrc/ck_vecchia.h) and the fixed-order sums of k_vecchia_terms /
// k_vecchia_sum compiled for the host (tests/test_vecchia_host.py; no GPU).
#include "host_vecchia_terms.h"

extern "C" {
int shim_vecchia_term(double z, double mu, double vv, double prior, double noise, int k, double* out4) {
    return ck_vecchia_term(z, mu, vv, prior, noise, k, &out4[0], &out4[1], &out4[2], &out4[3]);
}
long long shim_vecchia_terms(long n, const double* z, const double* mu, const double* vv, const double* prior, const double* noise,
                             const int* cnt2, double* mean, double* var, double* out3) {
    return host_vecchia_terms(n, z, mu, vv, prior, noise, cnt2, mean, var, out3);
}
}
