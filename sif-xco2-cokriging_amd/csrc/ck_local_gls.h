// ck_local_gls.h -- the p x p GLS step of universal cokriging in ONE neighbourhood (ck_predict_local_universal).
// Compiles for the host and for the device: the local kernels (ck_local.hip) run it on one thread of a workgroup, and
// tests/local_gls_shim.cpp builds it with g++ so that it can be checked against numpy without a GPU.
//
// A = U^T U, b = U^T y, r = x0 - U^T v over the p = p0 + p1 trend columns (process 0's columns first).  Steps:
//   1. a process with regressors but no neighbour in range has identically zero columns: if it is the predicted process i the
//      unbiasedness constraint cannot be met (rank deficient), else its columns are dropped from the system;
//   2. the kept block of A is factored (Cholesky, left-looking, the order of ck_host_gls) with the relative pivot threshold
//      of the joint path: a pivot not above tol times its diagonal entry is a rank-deficient design;
//   3. w = R^-1 b, s = R^-1 r, beta = R^-T w, r^T beta = s . w, r^T A^-1 r = |s|^2.
// Everything lives in caller-provided memory (W: p p + 2 p doubles; LDS on the device), nothing is indexed in registers:
// the kernels that inline this keep no scratch.
#pragma once

#if defined(__HIPCC__)
#define CK_LG_FN __host__ __device__ __forceinline__
#else
#define CK_LG_FN inline
#endif

#define CK_LG_OK 0
#define CK_LG_RANK_DEF 1

// A: the lower triangle of the p x p matrix, row-major with leading dimension lda.  n0 / n1: neighbours of process 0 / 1.
// beta (p values): the coefficients, NaN in dropped columns (all NaN when rank deficient).  *rb = r^T beta, *rar = r^T A^-1 r.
CK_LG_FN int ck_local_gls(int p0, int p1, int n0, int n1, int i, const double* A, int lda, const double* b, const double* r,
                          double tol, double* W, double* beta, double* rb, double* rar) {
    const int p = p0 + p1;
    const double nan = __builtin_nan("");
    for (int j = 0; j < p; ++j) beta[j] = nan;
    *rb = 0.0;
    *rar = 0.0;
    const bool drop0 = p0 > 0 && n0 == 0, drop1 = p1 > 0 && n1 == 0;
    if (i == 0 ? drop0 : drop1) {
        *rb = *rar = nan;
        return CK_LG_RANK_DEF;
    }
    const int lo = drop0 ? p0 : 0, hi = drop1 ? p0 : p, pp = hi - lo;
    if (pp <= 0) return CK_LG_OK;
    double *R = W, *w = W + pp * pp, *s = w + pp;
    for (int j = 0; j < pp; ++j) {
        const double ajj = A[(lo + j) * lda + lo + j];
        double d = ajj;
        for (int k = 0; k < j; ++k) d -= R[j * pp + k] * R[j * pp + k];
        if (!(ajj > 0.0) || !(d > tol * ajj) || !(d - d == 0.0)) {
            *rb = *rar = nan;
            return CK_LG_RANK_DEF;
        }
        const double rjj = __builtin_sqrt(d);
        R[j * pp + j] = rjj;
        for (int a = j + 1; a < pp; ++a) {
            double t = A[(lo + a) * lda + lo + j];
            for (int k = 0; k < j; ++k) t -= R[a * pp + k] * R[j * pp + k];
            R[a * pp + j] = t / rjj;
        }
    }
    double q = 0.0, g = 0.0;
    for (int a = 0; a < pp; ++a) {   // forward substitution of b and r
        double tw = b[lo + a], ts = r[lo + a];
        for (int k = 0; k < a; ++k) {
            tw -= R[a * pp + k] * w[k];
            ts -= R[a * pp + k] * s[k];
        }
        w[a] = tw / R[a * pp + a];
        s[a] = ts / R[a * pp + a];
        q += s[a] * s[a];
        g += s[a] * w[a];
    }
    for (int a = pp - 1; a >= 0; --a) {   // beta = R^-T w, in place
        double t = w[a];
        for (int k = a + 1; k < pp; ++k) t -= R[k * pp + a] * w[k];
        w[a] = t / R[a * pp + a];
        beta[lo + a] = w[a];
    }
    *rb = g;
    *rar = q;
    return CK_LG_OK;
}
