// TEST-ONLY: the terms of the Vecchia likelihood (csrc/ck_vecchia.h) and their fixed-order sums, driven serially the way
// k_vecchia_terms / k_vecchia_sum (csrc/ck_local.hip) drive them with workgroups of 256 threads.  Shared by
// tests/host_vecchia_shim.cpp and tests/host_vecchia_sanitize_main.cpp.
#pragma once

#include <vector>

#include "ck_vecchia.h"

#define HV_TPB 256

// the tree of one workgroup: red[t] += red[t + s] for s = 128, 64, .., 1; first = the smallest non-zero entry
static inline void hv_tree(double* a, double* b, long long* first) {
    for (int s = HV_TPB / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) {
            a[t] += a[t + s];
            b[t] += b[t + s];
            const long long o = first[t + s];
            if (o != 0 && (first[t] == 0 || o < first[t])) first[t] = o;
        }
}

// noise may be null (none).  mean, var: n each; out3 = (l, sum log var, sum quad), NaN when a datum has no term; returns
// 1 + the first such datum, or 0
static inline long long host_vecchia_terms(long n, const double* z, const double* mu, const double* vv, const double* prior,
                                           const double* noise, const int* cnt2, double* mean, double* var, double* out3) {
    const long nblk = (n + HV_TPB - 1) / HV_TPB;
    std::vector<double> part((size_t)(2 * nblk), 0.0);
    std::vector<long long> bad((size_t)nblk, 0);
    double a[HV_TPB], b[HV_TPB];
    long long f[HV_TPB];
    for (long blk = 0; blk < nblk; ++blk) {
        for (int tid = 0; tid < HV_TPB; ++tid) {
            const long t = blk * HV_TPB + tid;
            a[tid] = b[tid] = 0.0;
            f[tid] = 0;
            if (t < n) {
                if (ck_vecchia_term(z[t], mu[t], vv[t], prior[t], noise ? noise[t] : 0.0, cnt2[2 * t] + cnt2[2 * t + 1], &mean[t],
                                    &var[t], &a[tid], &b[tid]))
                    f[tid] = t + 1;
            }
        }
        hv_tree(a, b, f);
        part[(size_t)(2 * blk)] = a[0];
        part[(size_t)(2 * blk + 1)] = b[0];
        bad[(size_t)blk] = f[0];
    }
    for (int tid = 0; tid < HV_TPB; ++tid) {
        a[tid] = b[tid] = 0.0;
        f[tid] = 0;
        for (long e = tid; e < nblk; e += HV_TPB) {
            a[tid] += part[(size_t)(2 * e)];
            b[tid] += part[(size_t)(2 * e + 1)];
            if (f[tid] == 0) f[tid] = bad[(size_t)e];
        }
    }
    hv_tree(a, b, f);
    out3[1] = f[0] ? NAN : a[0];
    out3[2] = f[0] ? NAN : b[0];
    out3[0] = f[0] ? NAN : ck_vecchia_total(n, a[0], b[0]);
    return f[0];
}
