// TEST-ONLY shim: the host part of the Fisher information (csrc/ck_host.cpp: ck_host_fisher_coef / _combine / _reml) compiled
// with g++, so that tests/test_fisher_host.py can check it against numpy without a GPU.  Never linked into the product library.
#include "ck_host.h"

extern "C" void shim_fisher_coef(int n_procs, double sig1, double sig2, double rho, double* C) {
    ck_host_fisher_coef(n_procs, sig1, sig2, rho, C);
}

extern "C" void shim_fisher_combine(const double* C, const double* T, const unsigned char* live, double* I) {
    ck_host_fisher_combine(C, T, live, I);
}

extern "C" int shim_fisher_reml(int p, int nops, const double* A, const double* K, int64_t ldk, const double* Gm, double* T) {
    return ck_host_fisher_reml(p, nops, A, K, ldk, Gm, T);
}
