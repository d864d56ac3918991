// TEST-ONLY shim: the per-neighbourhood GLS step of local universal cokriging (csrc/ck_local_gls.h, the code the local
// kernels run on the device) compiled with g++, so that tests/test_local_universal_host.py can check it against numpy
// without a GPU.  Never linked into the product library.
#include <vector>

#include "ck_local_gls.h"

// A: p x p row-major (p = p0 + p1).  Returns the status; beta: p values, out2 = (r^T beta, r^T A^-1 r).
extern "C" int shim_local_gls(int p0, int p1, int n0, int n1, int i, const double* A, const double* b, const double* r,
                              double tol, double* beta, double* out2) {
    const int p = p0 + p1;
    std::vector<double> W((std::size_t)(p * p + 2 * p + 1));
    return ck_local_gls(p0, p1, n0, n1, i, A, p, b, r, tol, W.data(), beta, &out2[0], &out2[1]);
}
