// ck_vecchia_info.h -- one datum's share of the expected information of the Vecchia likelihood (ck_loglik_vecchia_fisher,
// include/cokrige.h).
//
// The Vecchia value is sum_t [log p(z_S) - log p(z_c)], c the conditioning set of datum t (k data) and S = c + {t}; every term is
// a Gaussian marginal of the exact model, so the expected negative Hessian under the model is
//   I^V = sum_t [I(S_t) - I(c_t)],   I(A)_jk = 1/2 tr(C_A^-1 D_j,A C_A^-1 D_k,A),   D_j = dC_t / dtheta_j,
// C_t the (k + 1) x (k + 1) covariance of the set and the OBSERVATION (ck_vecchia_grad.h).  The datum is the last row of S, so
// the Cholesky factor of C_t holds that of C_c and the difference collapses onto the last row of L_t^-1 D_j L_t^-T.  With
// Sigma_loc = C_c = L L^T, w = Sigma_loc^-1 C[c, t], b = (-w, 1) and s2 the term's variance:
//   g_j = (D_j b)[c]  (k entries),   q_j = b^T D_j b  (= ds2 / dtheta_j),   y_j = L^-1 g_j,
//   I_t[j, k] = (y_j . y_k) / s2 + 1/2 q_j q_k / s2^2.
// An empty set is b = (1): I_t = 1/2 q_j q_k / s2^2 with q_j the derivative of the prior observation variance.  Every I_t is a
// Gram matrix plus a rank-one term: the sum is positive semi-definite; when every earlier datum is in every set it telescopes to
// the dense information (ck_loglik_fisher), whatever the ordering.
// D_j is, entry for entry, the matrix whose contraction gives the gradient: the entry rule below IS ck_vecchia_pair.
// Compiles for the host and for the device: k_vecchia_info (ck_local.hip) runs these lines; tests/host_vecchia_info.h drives them
// serially with g++ so that the rules can be checked against numpy without a GPU.
#pragma once

#include "ck_vecchia_grad.h"

#define CK_VI_NPAR CK_VG_NPAR                            // the 13 slots of ck_loglik_fisher
#define CK_VI_NTRI (CK_VI_NPAR * (CK_VI_NPAR + 1) / 2)   // 91: the lower triangle, e -> (j, k) by ck_vg_pair_of

// Entry (a, q) of the full square of C_t in the product U = D b: row13 (row a's 13 sums, one per slot) += b_q D_slot[a, q].
// ck_vecchia_pair halves its weight on the diagonal (a pair of the lower triangle stands for two entries, a diagonal one for
// itself), so the diagonal passes 2 b_a and the rule's 1/2 gives b_a exactly.
CK_HD void ck_vecchia_info_entry(double* row13, const CkVecchiaModel& V, int pa, int pq, bool diag, double h, double b_q, double d_a) {
    ck_vecchia_pair(row13, V, pa, pq, diag, h, diag ? 2.0 * b_q : b_q, d_a);
}

// The variance of the datum's term (ck_vecchia_term's); returns 1 where the datum has no term (local system not positive
// definite: mu NaN; variance not > 0).
CK_HD int ck_vecchia_info_var(double z, double mu, double vv, double prior, double noise, int k, double* s2) {
    double m, lv, qd;
    return ck_vecchia_term(z, mu, vv, prior, noise, k, &m, s2, &lv, &qd);
}

// I_t[j, k] from yy = y_j . y_k (0 for an empty set), q_j, q_k and s2; exact 0 where either slot is not live
CK_HD double ck_vecchia_info_combine(const CkVecchiaModel& V, int j, int k, double yy, double qj, double qk, double s2) {
    if (!(V.live >> j & 1u) || !(V.live >> k & 1u)) return 0.0;
    return yy / s2 + 0.5 * (qj * qk) / (s2 * s2);
}

// The 91 sums -> the 13 x 13 array (row-major), symmetric to the bit: rows and columns of slots that are not live are exact 0,
// the live block is NaN when some datum had no term.
CK_HD void ck_vecchia_info_mirror(const double* tri, unsigned live, int bad, double* out) {
    for (int e = 0; e < CK_VI_NTRI; ++e) {
        int j, k;
        ck_vg_pair_of(e, &j, &k);
        const bool on = (live >> j & 1u) && (live >> k & 1u);
        const double v = !on ? 0.0 : bad ? NAN : tri[e];
        out[j * CK_VI_NPAR + k] = v;
        out[k * CK_VI_NPAR + j] = v;
    }
}
