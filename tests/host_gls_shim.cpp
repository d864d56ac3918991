// TEST-ONLY shim: the host GLS step of universal cokriging (csrc/ck_host.cpp: ck_host_gls) compiled with g++, so that
// tests/test_universal_host.py can check it against numpy without a GPU.  Never linked into the product library.
#include "ck_host.h"

extern "C" int shim_gls(int p, const double* A, const double* b, double tol, double* R, double* beta, double* Ainv,
                        double* logdet, double* bAb) {
    return ck_host_gls(p, A, b, tol, R, beta, Ainv, logdet, bAb);
}
