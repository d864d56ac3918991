// TEST-ONLY shim: one datum's score of the Vecchia gradient (csrc/ck_vecchia_grad.h, driven serially by host_vecchia_grad.h)
// compiled for the host (tests/test_vecchia_grad_host.py; no GPU).
#include "host_vecchia_grad.h"

extern "C" {
int shim_vecchia_weights(double z, double mu, double vv, double prior, double noise, int k, double* out2) {
    return ck_vecchia_weights(z, mu, vv, prior, noise, k, &out2[0], &out2[1]);
}
int shim_vecchia_score(int n_procs, const double* par, unsigned live, int k, const double* xy, const int* proc, const double* S,
                       const double* c, const double* zc, double zt, double prior, double own, const double* dvar, double* out2,
                       double* score13) {
    CkMatern blk5[15];
    CkVecchiaModel V;
    host_vg_model(n_procs, par, live, blk5, &V);
    return host_vecchia_score(V, k, xy, proc, S, c, zc, zt, prior, own, dvar, out2, score13);
}
}
