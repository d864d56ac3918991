// TEST-ONLY shim: one datum's share of the Vecchia information (csrc/ck_vecchia_info.h, driven serially by host_vecchia_info.h)
// compiled for the host (tests/test_vecchia_info_host.py; no GPU).
#include "host_vecchia_info.h"

extern "C" {
int shim_vecchia_info(int n_procs, const double* par, unsigned live, int k, const double* xy, const int* proc, const double* S,
                      const double* c, double zt, double prior, double own, const double* dvar, double* out169) {
    CkMatern blk5[15];
    CkVecchiaModel V;
    host_vg_model(n_procs, par, live, blk5, &V);
    return host_vecchia_info(V, k, xy, proc, S, c, zt, prior, own, dvar, out169);
}
}
