// ck_vecchia_grad.h -- one datum's share of the gradient of the Vecchia likelihood (ck_loglik_vecchia_grad, include/cokrige.h).
//
// For datum t with the conditioning set c (k data), Sigma_loc = C[c, c], w = Sigma_loc^-1 C[c, t], alpha = Sigma_loc^-1 z_c:
//   b = (-w, 1), a = (alpha, 0) over the set plus the datum;  e = z_t - mu_t,  s2 = the term's variance;
//   score_t = 1/2 sum_pq M[p, q] dC_t[p, q] / dtheta,   M = (e^2 / s2^2 - 1 / s2) b b^T + (e / s2) (b a^T + a b^T),
// C_t the (k + 1) x (k + 1) covariance of the set and the observation (ck_set_noise's s d on its diagonal, the datum's own
// included).  An empty set is the one-entry system b = (1), a = (0), e = z_t: the prior observation variance is differentiated.
// Compiles for the host and for the device: k_vecchia_grad (ck_local.hip) runs these lines per pair; tests/host_vecchia_grad_shim.cpp
// drives them serially with g++ so that the rules can be checked against numpy without a GPU.
#pragma once

#include "ck_math.h"
#include "ck_vecchia.h"

#define CK_VG_NPAR 13   // == CK_FISHER_NPAR: the 11 model parameters in ck_loglik's flat order (one process: the first 4), s_0, s_1

// What the pair rule reads besides the pair: blk5 / dnu as ck_loglik prepares them (block b at blk5[5 b], its four shifted
// copies behind it), the model's sigma and rho, and which slots are live.
struct CkVecchiaModel {
    const CkMatern* blk5;
    double dnu[3];
    double sig1, sig2, rho;
    int n_procs;
    unsigned live;      // bit k: slot k is live (free and existing)
    unsigned nu_live;   // bit b: the nu slot of block b is live -- else its four shifted evaluations are skipped
};

// the nu slot of block b (0 = 11, 1 = 12, 2 = 22)
CK_HD int ck_vg_nu_slot(int n_procs, int b) { return n_procs == 1 ? 1 : 2 + b; }

// the two weights of M, from the term's arithmetic (ck_vecchia_term).  Returns 1 -- and NaN weights -- where the term has no
// value (local system not positive definite: mu NaN; variance not > 0).
CK_HD int ck_vecchia_weights(double z, double mu, double vv, double prior, double noise, int k, double* w_bb, double* w_ab) {
    double m, s2, lv, qd;
    if (ck_vecchia_term(z, mu, vv, prior, noise, k, &m, &s2, &lv, &qd)) {
        *w_bb = NAN;
        *w_ab = NAN;
        return 1;
    }
    const double e = z - m;
    *w_bb = (e / s2) * (e / s2) - 1.0 / s2;
    *w_ab = e / s2;
    return 0;
}

// M[p, q] from the entries of b and a
CK_HD double ck_vecchia_m(double w_bb, double w_ab, double bp, double ap, double bq, double aq) {
    return w_bb * (bp * bq) + w_ab * (bp * aq + ap * bq);
}

// ck_matern_grad with the four shifted evaluations optional: M and dlen are computed by the same expressions either way
CK_HD CkMaternGrad ck_vg_matern(const CkMatern& m, const CkMatern* mv, double dnu, double h, bool want_nu) {
    if (want_nu) return ck_matern_grad(m, mv, dnu, h);
    CkMaternGrad g;
    g.dnu = 0.0;
    g.dlen = 0.0;
    if (h == 0.0) {
        g.M = 1.0;
        return g;
    }
    const double s = m.sqrt2nu * (h / m.len_scale);
    g.M = ck_matern_rho_scaled(m, s);
    if (g.M == 0.0) return g;
    g.dlen = (s / m.len_scale) * ck_matern_dlen_scaled(m, s);
    return g;
}

// One pair (p, q) of the lower triangle, p >= q, of processes pp / pq at distance h (the distance and the h == 0 test of
// k_loglik_grad): acc += the pair's weight times dC[p, q] / dtheta, by k_loglik_grad's slot rule.  mpq = M[p, q]; on the
// diagonal the weight is mpq / 2 and d_p (the raw measurement-error variance of the entry, 0: none) goes to slot 11 + pp.
CK_HD void ck_vecchia_pair(double* acc, const CkVecchiaModel& V, int pp, int pq, bool diag, double h, double mpq, double d_p) {
    const int b = V.n_procs == 2 ? pp + pq : 0;
    const double w = (diag ? 0.5 : 1.0) * mpq;
    const CkMatern& m = V.blk5[5 * b];
    const double dnu = b == 0 ? V.dnu[0] : b == 1 ? V.dnu[1] : V.dnu[2];
    const CkMaternGrad gr = ck_vg_matern(m, V.blk5 + 5 * b + 1, dnu, h, (V.nu_live >> b & 1u) != 0);
    const double z0 = h == 0.0 ? w : 0.0;
    if (V.n_procs == 1) {   // sigma nu len nugget
        acc[0] += w * (2.0 * V.sig1 * gr.M);
        acc[1] += w * (m.amp * gr.dnu);
        acc[2] += w * (m.amp * gr.dlen);
        acc[3] += z0;
    } else if (b == 0) {    // sigma_11 sigma_22 nu_11 nu_12 nu_22 len_11 len_12 len_22 nugget_11 nugget_22 rho_12
        acc[0] += w * (2.0 * V.sig1 * gr.M);
        acc[2] += w * (m.amp * gr.dnu);
        acc[5] += w * (m.amp * gr.dlen);
        acc[8] += z0;
    } else if (b == 2) {
        acc[1] += w * (2.0 * V.sig2 * gr.M);
        acc[4] += w * (m.amp * gr.dnu);
        acc[7] += w * (m.amp * gr.dlen);
        acc[9] += z0;
    } else {
        acc[0] += w * (V.rho * V.sig2 * gr.M);
        acc[1] += w * (V.rho * V.sig1 * gr.M);
        acc[10] += w * (V.sig1 * V.sig2 * gr.M);
        acc[3] += w * (m.amp * gr.dnu);
        acc[6] += w * (m.amp * gr.dlen);
    }
    if (diag) {
        if (pp == 0)
            acc[11] += w * d_p;
        else
            acc[12] += w * d_p;
    }
}

// what a datum's score holds in slot k at the end: its sum where the slot is live (NaN where the term has no value), exact 0
// where it is not
CK_HD double ck_vecchia_slot_out(const CkVecchiaModel& V, int k, double sum, int bad) {
    if (!(V.live >> k & 1u)) return 0.0;
    return bad ? NAN : sum;
}

// the lower-triangle index e -> (a, b), a >= b (the local kernels' expression)
CK_HD void ck_vg_pair_of(long e, int* a_out, int* b_out) {
    long a = (long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > e) --a;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    *a_out = (int)a;
    *b_out = (int)(e - a * (a + 1) / 2);
}
