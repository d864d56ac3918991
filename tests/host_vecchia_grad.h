// TEST-ONLY: k_vecchia_grad's steps for one datum, serially on the host, on the lines of csrc/ck_vecchia_grad.h (the two
// weights, the empty set, the pair rule and its slots): the Cholesky with the two rows riding along, mu and v . v, the back
// substitution as the kernel's single wave runs it (step j divides entry j and updates the entries below it), the contraction
// over the lower triangle of the set plus the datum.  Euclidean sites.  Used by host_vecchia_grad_shim.cpp (against numpy) and
// host_vecchia_grad_sanitize_main.cpp (under the sanitizers).
#pragma once
#include <math.h>

#include <vector>

#include "ck_model.h"
#include "ck_vecchia_grad.h"

// par: the flat parameters (n_procs == 1: sigma nu len nugget; 2: the 11 of ck_loglik); blk5: 15 blocks, filled here
inline void host_vg_model(int n_procs, const double* par, unsigned live, CkMatern* blk5, CkVecchiaModel* V) {
    const int nblk = n_procs == 1 ? 1 : 3;
    const double offs[4] = {-2.0, -1.0, 1.0, 2.0};
    V->blk5 = blk5;
    V->n_procs = n_procs;
    V->sig1 = par[0];
    V->sig2 = n_procs == 2 ? par[1] : 0.0;
    V->rho = n_procs == 2 ? par[10] : 0.0;
    V->live = live;
    V->nu_live = 0;
    for (int b = 0; b < 3; ++b) {
        const int bb = b < nblk ? b : 0;
        double nu, len, amp, nug;
        if (n_procs == 1) {
            nu = par[1], len = par[2], amp = par[0] * par[0], nug = par[3];
        } else {
            nu = par[2 + bb], len = par[5 + bb];
            amp = bb == 0 ? par[0] * par[0] : bb == 2 ? par[1] * par[1] : par[10] * par[0] * par[1];
            nug = bb == 0 ? par[8] : bb == 2 ? par[9] : 0.0;
        }
        V->dnu[b] = ck_matern_dnu_step(nu);
        ck_matern_prepare(nu, len, amp, nug, &blk5[5 * b]);
        for (int k = 0; k < 4; ++k) ck_matern_prepare(nu + offs[k] * V->dnu[b], len, amp, nug, &blk5[5 * b + 1 + k]);
        if (b < nblk && (live >> ck_vg_nu_slot(n_procs, b) & 1u)) V->nu_live |= 1u << b;
    }
}

// One datum.  xy: (k + 1) x 2 sites, the datum last; proc: their processes; S: k x k local covariance (row-major, the noise on
// its diagonal); c, zc: k; dvar: k + 1 raw variances or null.  out2 = (mu, v . v) (untouched for k == 0).  Returns 1 for a
// datum without a term (NaN in the live slots).
inline int host_vecchia_score(const CkVecchiaModel& V, int k, const double* xy, const int* proc, const double* S_in, const double* c,
                              const double* zc, double zt, double prior, double own, const double* dvar, double* out2,
                              double* score) {
    const int ld = k > 0 ? k : 1;
    std::vector<double> S((size_t)(k + 2) * ld, 0.0);
    for (int a = 0; a < k; ++a) {
        for (int b = 0; b <= a; ++b) S[(size_t)a * ld + b] = S_in[(size_t)a * k + b];
        S[(size_t)k * ld + a] = c[a];
        S[(size_t)(k + 1) * ld + a] = zc[a];
    }
    int fail = 0;
    for (int j = 0; j < k && !fail; ++j) {
        const double piv = S[(size_t)j * ld + j];
        if (!(piv > 0.0)) {
            fail = 1;
            break;
        }
        const double rd = 1.0 / sqrt(piv);
        for (int a = j + 1; a < k + 2; ++a) S[(size_t)a * ld + j] *= rd;
        S[(size_t)j * ld + j] = sqrt(piv);
        for (int a = j + 1; a < k + 2; ++a)
            for (int b = j + 1; b < k && b <= a; ++b) S[(size_t)a * ld + b] -= S[(size_t)a * ld + j] * S[(size_t)b * ld + j];
    }
    double mu = 0.0, vv = 0.0;
    for (int a = 0; a < k; ++a) {
        mu += S[(size_t)k * ld + a] * S[(size_t)(k + 1) * ld + a];
        vv += S[(size_t)k * ld + a] * S[(size_t)k * ld + a];
    }
    if (fail) mu = NAN;
    if (k > 0) {
        out2[0] = mu;
        out2[1] = vv;
    }
    double w_bb, w_ab;
    const int bad = ck_vecchia_weights(zt, mu, vv, prior, own, k, &w_bb, &w_ab);
    if (bad) {
        for (int s = 0; s < CK_VG_NPAR; ++s) score[s] = ck_vecchia_slot_out(V, s, 0.0, 1);
        return 1;
    }
    double* xv = &S[(size_t)k * ld];
    double* xa = &S[(size_t)(k + 1) * ld];
    for (int j = k - 1; j >= 0; --j) {   // the wave's steps, lane by lane
        const double dj = S[(size_t)j * ld + j];
        const double vj = xv[j] / dj, yj = xa[j] / dj;
        xv[j] = vj;
        xa[j] = yj;
        for (int a = 0; a < j; ++a) {
            xv[a] -= S[(size_t)j * ld + a] * vj;
            xa[a] -= S[(size_t)j * ld + a] * yj;
        }
    }
    for (int a = 0; a < k; ++a) xv[a] = -xv[a];
    double acc[CK_VG_NPAR] = {};
    const long npair = (long)(k + 1) * (k + 2) / 2;
    for (long e = 0; e < npair; ++e) {
        int a, b;
        ck_vg_pair_of(e, &a, &b);
        const double ba = a < k ? xv[a] : 1.0, aa = a < k ? xa[a] : 0.0, bb = b < k ? xv[b] : 1.0, ab = b < k ? xa[b] : 0.0;
        const double h = a == b ? 0.0 : ck_euclid(xy[2 * a], xy[2 * a + 1], xy[2 * b], xy[2 * b + 1]);
        ck_vecchia_pair(acc, V, proc[a], proc[b], a == b, h, ck_vecchia_m(w_bb, w_ab, ba, aa, bb, ab), a == b && dvar ? dvar[a] : 0.0);
    }
    for (int s = 0; s < CK_VG_NPAR; ++s) score[s] = ck_vecchia_slot_out(V, s, acc[s], 0);
    return 0;
}
