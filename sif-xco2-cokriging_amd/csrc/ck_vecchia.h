// ck_vecchia.h -- one factor of the Vecchia likelihood (ck_loglik_vecchia, include/cokrige.h): from a datum's local simple-
// cokriging solve (mean v . y and v . v over the earlier data it is conditioned on) to its conditional mean, the variance of
// the OBSERVATION and the two terms the likelihood sums.
// Compiles for the host and for the device: k_vecchia_terms (ck_local.hip) runs it once per datum; tests/host_vecchia_shim.cpp
// runs the same lines with g++ so that the rules can be checked against numpy without a GPU.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef CK_HD   // as in ck_math.h
#if defined(__HIPCC__)
#define CK_HD __host__ __device__ __forceinline__
#else
#define CK_HD inline
#endif
#endif

// z: the datum; (mu, vv): its local solve, read only when k > 0 (mu NaN: the local system was not positive definite);
// prior = sigma_i^2 + nugget_i; noise = the datum's own s_i d_t (0: none); k: size of the conditioning set.
//   k == 0:  mean = 0, var = prior + noise               (counted, not an error)
//   else     mean = mu, var = prior + noise - vv         (raw: no clamp, no square root)
//   logv = log var,  quad = (z - mean)^2 / var
// Returns 1 -- and NaN in logv and quad -- when the local system was not positive definite or var is not > 0 (then mean and
// var are still what the solve gave), else 0.
CK_HD int ck_vecchia_term(double z, double mu, double vv, double prior, double noise, int k, double* mean, double* var,
                          double* logv, double* quad) {
    const double m = k > 0 ? mu : 0.0;
    const double s2 = k > 0 ? (prior + noise) - vv : prior + noise;
    *mean = m;
    *var = s2;
    if (!(s2 > 0.0) || m != m) {
        *logv = NAN;
        *quad = NAN;
        return 1;
    }
    const double e = z - m;
    *logv = log(s2);
    *quad = e * e / s2;
    return 0;
}

// l = -1/2 (N log 2 pi + sum log var + sum quad)
CK_HD double ck_vecchia_total(int64_t n, double sum_logv, double sum_quad) {
    return -0.5 * ((double)n * 1.8378770664093454835606594728112 + sum_logv + sum_quad);
}
