// ck_internal.h -- launch wrappers shared between the translation units of
// libcokrige_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ck_host.h"
#include "ck_math.h"
#include "ck_vecchia_grad.h"
#include "ck_vecchia_info.h"
#include "ck_vecchia_trend.h"

#define CK_NB 512   // outer block column width (panel width)
#define CK_IB 64    // inner block (diagonal factor / row solves)
#define CK_BM 256   // GEMM tile rows
#define CK_AUX_ALIGN 256
// every packed panel carries, behind its rows, the inverses of its eight 64 x 64 diagonal blocks
// (k_potrf64 -> k_trsm64m); they travel with the panel in the multi-GPU broadcast
#define CK_PANEL_TAIL ((CK_NB / CK_IB) * CK_IB * CK_IB)

// ---- covariance assembly (ck_cov.hip) ---------------------------------------
// per-site transform: degrees -> (lat_rad, lon_rad, cos lat) | (x, y, 0)
void ck_launch_prep_sites(hipStream_t s, const double* coords, int64_t n, int metric, double* c0, double* c1,
                          double* c2, double* u /* 3 x n chord vectors, may be null */);
// tabulated fast path (ck_math.h "Tabulated correlation")
void ck_launch_table_nodes(hipStream_t s, const CkMatern* m, int metric, const double* q, int64_t n, double* out);
void ck_launch_table_check(hipStream_t s, const CkMatern* m, int metric, CkTable tab, const double* coef,
                           unsigned long long* max_err_bits);
// Internal site order: process 0 in [0, n0), process 1 in [n0p, nend), n0p = roundup(n0, 64);
// every other index below npad is padding (identity in Sigma, zero in the right-hand sides).
struct CkLayout {
    long n0, n0p, nend, npad;
};
// entries the table kernels defer to the exact evaluator: (row, col) pairs + device counter
// Two counters, used alternately (round 4): the pass that evaluates one assembly's list (k_assemble_fix) zeroes the counter
// of the NEXT assembly, so that no assembly starts with a memset launch of its own.
struct CkWorklist {
    int2* items;
    unsigned* count;   // count[0]: deferred entries; count[1]: work queue of the assembly kernel (option "assemble_queue")
    unsigned cap;
    unsigned* reset;   // the other pair of counters (may be null)
};
// which panels one assembly launch covers: Sigma -- the owned panels (tile0[j] = index of the first
// 64-row tile of the j-th owned panel, panel_of[j] = its block column, sigptr[K] = its storage);
// right-hand sides -- n_panels panels of aux_tiles tiles each, contiguous from `aux`
struct CkPanelMap {
    const int* tile0;
    const int* panel_of;
    double* const* sigptr;
    int n_panels;
    double* aux;
    long aux_tiles;
    const int* order;   // Sigma, work-queue form: the strips sorted by Matern block (may be null: back to front)
};
// Sigma: every owned block column (rows K*NB.., ld = CK_NB) in ONE launch.
// c: 3 x npad exact-formula coordinates, u: 3 x npad chord vectors.  fast: table path.
void ck_launch_assemble_sigma(hipStream_t s, bool fast, const CkMatern* blk, const CkTable* tabs,
                              const double* const* coefs, int metric, const double* c, const double* u, CkLayout L,
                              CkPanelMap pm, int total_tiles, CkWorklist wl, int queue_slots = 0 /* > 0 (table path): that many
                              resident workgroups take their strips from a work queue (the word behind wl.count, zero at launch) */);
// right-hand-side rows, every block column in one launch: rows = prediction sites p in [0, m)
// (row m = data values z, rows > m zero), cols = data sites.
// raw (table path only; may be null): the prediction sites' coordinates as the caller gave them (m x 2, padded with zeros
// to mpad).  The launch then transforms them itself -- every workgroup its own 64 rows, the workgroups of block column 0
// also write pc / pu for the later users (exact pass, _verify_model) -- instead of waiting for a k_prep_sites launch.
void ck_launch_assemble_aux(hipStream_t s, bool fast, const CkMatern* blk, const CkTable* tabs,
                            const double* const* coefs, int metric, int i_pred, double* pc, double* pu,
                            int64_t m, int64_t mpad, const double* c, const double* u, const double* z, CkLayout L,
                            int n_panels, double* aux, CkWorklist wl, const double* raw = nullptr, int queue_slots = 0,
                            int64_t pair_m0 = -1 /* >= 0: rows of BOTH processes (ck_predict_pair) -- process 0 in [0, pair_m0), zeros up
                            to roundup(pair_m0, 64), process 1 from there to m; i_pred is not used */);
// evaluate the deferred entries of the preceding table-path launches (no-op when the list is empty)
void ck_launch_assemble_fix(hipStream_t s, bool aux_rows, const CkMatern* blk, int metric, int i_pred,
                            const double* pc, int64_t mpad, const double* c, CkLayout L, CkWorklist wl,
                            double* const* sigptr, double* aux, int64_t pair_m0 = -1 /* as ck_launch_assemble_aux */);
// out[t] = C_01(d(a, b)) - V_a . V_b for the q row pairs rows[t] = (a, b) of the solved right-hand sides: the posterior
// covariance between a process-0 and a process-1 prediction site (ck_predict_pair); pc: 3 x mpad exact-formula coordinates
void ck_launch_pair_cov(hipStream_t s, const double* aux, int64_t mpad, int n_panels, const int2* rows, int64_t q,
                        const CkMatern* blk, int metric, const double* pc, double* out);
// measurement-error variances (ck_set_noise): Sigma_gg += nz[g] at every data site g (nz: npad values in the internal order,
// zero where there is none); behind ck_launch_assemble_fix, once per assembled Sigma.  nz == null: no launch.
void ck_launch_assemble_noise(hipStream_t s, double* const* sigptr, const double* nz, CkLayout L);
// dense a x b block for one (i, j) Matern block; mode 0 = covariance, 1 = distance only
void ck_launch_cov_dense(hipStream_t s, const CkMatern* blk_ij, int metric, int add_nugget, int mode,
                         const double* a0, const double* a1, const double* a2, int64_t a, const double* b0,
                         const double* b1, const double* b2, int64_t b, double* out);
void ck_launch_model_variogram(hipStream_t s, const CkMatern* blk, double sill, int kind, const int* pi,
                               const int* pj, const double* lags, int64_t n, double* out);
void ck_launch_cov_lags(hipStream_t s, const CkMatern* blk_ij, int add_nugget, const double* lags, int64_t n,
                        double* out);

// ---- block cokriging (ck_blocks.hip) ------------------------------------------------------
// block rows out[b] (+)= sum_k w_k aux[rows_k] over the member list off[b] .. off[b + 1] of every panel, in list order;
// row r = the data row zrow of aux; first != 0: start from zero and zero the padding rows (r, mpad_r)
void ck_launch_block_fold(hipStream_t s, const double* aux, int64_t mpad, int n_panels, double* out, int64_t mpad_r,
                          const int* off, const int* rows, const double* w, int64_t r, int64_t zrow, int first);
// Cbar[R][C] = sum_{a in R, c in C} w_a w_c C(h(a, c)) (nugget where h == 0) over members stored block by block
// (c0 / c1 / c2: exact-formula coordinates, off: r + 1 offsets).  full == 0: diag[b] = Cbar[b][b];
// full != 0: the lower triangle into packed panels (panel J = C / NB: rows J NB .., ld = NB).
// The pairs of element e (e = b | R (R + 1) / 2 + C) are cut into pieces of CK_PRIOR_PIECE pairs: poff[e] .. poff[e + 1]
// (n_elem + 1 words, host-built: ck_host_prior_pieces), part: n_pieces doubles of scratch
#define CK_PRIOR_PIECE 512
void ck_launch_block_prior(hipStream_t s, const CkMatern* blk, int metric, const double* c0, const double* c1,
                           const double* c2, const double* w, const int* off, int64_t r, int full, const long long* poff,
                           int64_t n_pieces, double* part, double* diag, double* const* panels);

// ---- dense linear algebra (ck_la.hip) ----------------------------------------
// C (M x N, ldc) -= A (M x K, lda) * B (N x K, ldb)^T on FP64 MFMA.
// M % 256 == 0, N % 64 == 0, K % 16 == 0.  lower: skip tiles whose rows are all above the
// diagonal  row + diag_off == col.
// batch > 1 repeats the product over blockIdx.y with element strides sC / sA / sB.
void ck_launch_gemm_nt(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t lda, const double* B,
                       int64_t ldb, int64_t M, int64_t N, int64_t K, int lower, int64_t diag_off, int batch,
                       int64_t sC, int64_t sA, int64_t sB);
// Cholesky trailing update of every owned block column J = J0 + y * Jstep (y < nJ) by panel K
// (device pointer table sigptr_dev[J], panel P = rows K*NB.. of L).
void ck_launch_cu_probe(hipStream_t s, unsigned* out, int n_wg, int spin);
void ck_launch_syrk_group(hipStream_t s, double* const* sigptr_dev, double* const* srcptr_dev, int K0, int np, int J0,
                          int Jstep, int nJ, int64_t Npad, int64_t nvalid /* rows / columns from here on are identity padding */,
                          unsigned long long* stamps = nullptr /* diagnostic: ck_debug_gemm_clock */);
// the whole panel step (diagonal blocks, inverses, row solves, panel-internal updates) in ONE launch: nrows / 64 workgroups
// that hand each other the pivot blocks through flags[0..7] == seq (ck_la.hip: k_panel_coop); *err != 0: a wait timed out
// X / xrows (round 4): right-hand-side rows of this block column, further workgroups of the same launch (null / 0: none)
void ck_launch_panel_coop(hipStream_t s, double* P, int64_t nrows, double* tail, int64_t g0, long long* info, unsigned* flags,
                          unsigned seq, unsigned* err, double* X = nullptr, int64_t xrows = 0, unsigned spins = 2000000u,
                          int drop = -1 /* tests: this chunk of the diagonal block never publishes */);
// one update of the TALL matrix [Sigma; c0^T; z^T]: block columns J0 .. J0 + nJ - 1 of Sigma and of the mpad right-hand-side
// rows by the panels K0 .. K0 + np - 1, one launch (ck_la.hip: k_tall_group_d)
void ck_launch_tall_group(hipStream_t s, double* const* sigptr_dev, double* aux, int64_t mpad, int K0, int np, int J0, int nJ,
                          int64_t nvalid, int64_t mrows = 0);
// diagnostic: the cooperative panel step with shader-clock stamps of its links 1 .. 7 (prof: 64 words)
void ck_launch_panel_coop_prof(hipStream_t s, double* P, int64_t nrows, double* tail, int64_t g0, long long* info,
                               unsigned* flags, unsigned seq, unsigned* err, long long* prof);
void ck_launch_aux_group(hipStream_t s, double* aux, int64_t mpad, double* const* sigptr_dev, int K0, int np, int J0,
                         int nJ, int64_t mrows, int64_t nvalid, int64_t live_rows = 0);
// S_J -= sum_p aux_p[rows of J..] aux_p[rows of block J]^T for the nJ block columns of the prediction sites' Schur
// complement (ck_verify_model); aux: np block columns of mpad x CK_NB solved right-hand-side rows
void ck_launch_schur_syrk(hipStream_t s, double* const* schur_dev, const double* aux, int64_t mpad, int np, int nJ,
                          int64_t Mpad);
// G = alpha alpha^T - W^T W over the unit right-hand-side rows of all data sites (ck_loglik; row 1 + p of aux = W_p, alpha[p]
// = W_p . y): the lower tiles of the first nvalid rows of the Npad = nK NB order, packed block columns G_dev[J]; a tile skips
// the panels in front of its first row, where its W rows are zero.  mpad >= Npad + dense (the rows read are dense ..
// dense + Npad - 1).  Rank-q start (ck_loglik_reml): the accumulators start from sum_j a_j[p] a_j[q] over the q vectors
// a_j = avec + j ald (q = 1, avec = alpha: ck_loglik's alpha alpha^T, the same bits); dense: the rows in front of the unit rows.
void ck_launch_ginv_syrk(hipStream_t s, double* const* G_dev, const double* aux, int64_t mpad, const double* avec, int nK,
                         int64_t nvalid, int q = 1, int64_t ald = 0, int dense = 1);
// Conditional simulation (ck_conditional_draws): X (nd x m, ld m, the caller's site order) = pred + eps L_S^T on the lower
// tiles of the factor L_S in the Schur buffers (L_dev[J]: packed block columns, upper triangles of the diagonal blocks zero).
// E: -eps in block columns of ldp >= roundup(nd, 128) rows (ck_launch_draw_noise); pred, cmap: Mp entries in the internal order
// (cmap[j]: the caller's index of internal site j, -1 beyond m); ones: 128 doubles equal to 1.
// rows (0: m): the internal sites where they outnumber the caller's m columns (ck_conditional_draws_pair's gap rows, cmap -1)
void ck_launch_draw_trmm(hipStream_t s, double* X, int64_t m, const double* E, int64_t ldp, int64_t nd, double* const* L_dev,
                         const double* pred, const double* ones, const int* cmap, int64_t rows = 0);
// In-place Cholesky of the 64 x 64 diagonal block at A (ld); info_dev gets global_index0 + j + 1 of
// the first non-positive pivot (only if still 0).
void ck_launch_potrf64(hipStream_t s, double* A, int64_t ld, int64_t global_index0, long long* info_dev,
                       double* Linv);
// diagnostic: the same with shader-clock stamps at its phase boundaries (prof: 16 words)
void ck_launch_potrf64_prof(hipStream_t s, double* A, int64_t ld, long long* info, double* Linv, long long* prof);
// X L^T = A in place for `nrows` rows of A (ld), 64 columns; L (64 x 64 lower, ldl).  nrows % 64 == 0.
// fused panel step (ck_la.hip, option "panel_fused")
void ck_launch_panel_diag(hipStream_t s, double* P, int j, int64_t g0, long long* info, double* Linv);
void ck_launch_panel_rows_all(hipStream_t s, double* X, int64_t nrows, const double* P, const double* tail, double* X2 = nullptr,
                              int64_t nrows2 = 0);
void ck_launch_panel_rows(hipStream_t s, double* X, int64_t row_first, int64_t nrows, const double* P, int j,
                          const double* Linv);
void ck_launch_trsm64(hipStream_t s, double* A, int64_t ld, int64_t nrows, const double* Linv);
// pred[p] = sum_c X[p][c] y[c];  err[p] = nan_to_num(sqrt(c0 - sum_c X[p][c]^2)); X rows live in
// n_panels panels of width CK_NB at aux + K * mpad * CK_NB; y is row `zrow`.
// c0 < 0: raw mode, pred[p] = X_p . y and err[p] = |X_p|^2 (leave-one-out).
void ck_launch_reduce_pred(hipStream_t s, const double* aux, int64_t mpad, int n_panels, int64_t m, int64_t zrow,
                           double c0, double* pred, double* err);
void ck_launch_tri_matvec(hipStream_t s, double* const* sigptr_dev, int64_t npad, const double* v, double* out);
// dense: the row of the unit vector of datum 0 (1: row 0 = z only; ck_loglik_reml: 1 + p, the trend rows in between)
void ck_launch_loo_rows(hipStream_t s, double* aux, int64_t mpad, int64_t m, int64_t g0, const double* z,
                        int64_t npad, int64_t dense = 1);
// Universal cokriging (ck_predict_universal / ck_loglik_reml): every row r < nrows of the right-hand sides dotted with the q
// basis rows brow0 .. brow0 + q - 1 ([y; U] = the data row and the trend rows) in one pass over the panels:
// out[r (q + 1)] = |X_r|^2, out[r (q + 1) + 1 + j] = X_r . X_{brow0 + j}.  q <= CK_UNIV_QMAX, brow0 + q <= mpad, nrows <= mpad.
// Every row sums in a fixed order that does not depend on nrows or on its neighbours.
#define CK_UNIV_QMAX 17
void ck_launch_reduce_univ(hipStream_t s, const double* aux, int64_t mpad, int n_panels, int64_t nrows, int64_t brow0, int q,
                           double* out);
void ck_launch_mfma_probe(hipStream_t s, int32_t* out);
int ck_launch_mfma_peak(hipStream_t s, int blocks, int waves_per_simd, int iters, double* sink);

// ---- Gaussian log-likelihood (ck_lik.hip) ----------------------------------------------------
// part[K] = sum of log L_qq over the valid rows q of panel K (sigptr[K]: rows K NB .., ld = NB), nK panels
void ck_launch_lik_logdet(hipStream_t s, double* const* sigptr_dev, int nK, CkLayout L, double* part);
// The contraction 1/2 sum_pq G_pq dSigma_pq / dtheta_k over the lower triangle of G (packed block columns G_dev[J], the
// off-diagonal entries counted twice) with the exact evaluator.  blk5[5 b .. 5 b + 4]: Matern block b = 0 (11), 1 (12), 2 (22)
// and the same block at nu - 2 dnu_b, nu - dnu_b, nu + dnu_b, nu + 2 dnu_b.  c: 3 x npad exact-formula coordinates.
// part: CK_LIK_NPAR doubles per workgroup (ck_lik_grad_groups of them), in the flat order of the parameters.
#define CK_LIK_NPAR 11
int64_t ck_lik_grad_groups(CkLayout L);
void ck_launch_loglik_grad(hipStream_t s, double* const* G_dev, CkLayout L, int n_procs, int metric, const double* c,
                           const CkMatern* blk5, const double* dnu3, double sig1, double sig2, double rho, double* part);
// out3[3 r ..] = (M, dM/dnu, dM/dlen) of ck_matern_grad at lag |lags[r]|; blk5: ONE block's five entries, dnu its step
void ck_launch_debug_matern_grad(hipStream_t s, const CkMatern* blk5, double dnu, const double* lags, int64_t n, double* out3);

// part[2 K + k] = sum of G_aa d_a over the sites a of process k in block column K (d: npad variances in the internal order);
// dl/ds_k = 1/2 sum_K part[2 K + k] (ck_loglik_noise_grad)
void ck_launch_lik_noise_grad(hipStream_t s, double* const* G_dev, int nK, CkLayout L, const double* d, double* part);

// ---- Fisher information of the likelihood fit (ck_fisher.hip; the product kernel: ck_la.hip) --------------------------
// Parameter slots: the CK_LIK_NPAR model parameters in the flat order, then the noise scales s_0, s_1.  Every dSigma/dtheta is a
// combination of the OPERANDS below (ck_host.h: ck_host_fisher_coef has the coefficients): per Matern block the correlation
// R, amp dR/dnu, amp dR/dlen and -- inside a process -- Z, the 0 / 1 pattern of h == 0; per process diag(d_a).
#define CK_FISHER_NPAR 13   // == CK_LIK_NPAR + 2 (include/cokrige.h has the same definition)
static_assert(CK_FISHER_NPAR == CK_LIK_NPAR + 2, "the model parameters and the two noise scales");
#define CK_FISHER_NOPS 13
#define CK_FISHER_NPAIR (CK_FISHER_NOPS * (CK_FISHER_NOPS + 1) / 2)
#define CK_FOP_R00 0     // R, dnu, dlen, Z of block (0, 0): operands 0 .. 3
#define CK_FOP_R11 4     // ... of block (1, 1): 4 .. 7
#define CK_FOP_R01 8     // R, dnu, dlen of the cross block and its transpose: 8 .. 10
#define CK_FOP_DIAG0 11  // diag(d_a) on process 0 / 1: 11, 12
#define CK_FISHER_YROWS 256   // rows of the thin REML operand Y^T (>= CK_FISHER_NOPS CK_LU_PMAX)
// One UNIT of a dense operand D: the columns n in [c0, c0 + wpad) of the product Sigma^-1 D with the rows k of D in the K-panels
// pK0 .. pK0 + npan - 1, stored as the product kernel's second operand: D[(pp wpad + n) NB + k'] = D[(pK0 + pp) NB + k', c0 + n]
// (zero outside the block: the kernel runs over whole panels and 128-column tiles).  nlo / nhi: the columns that belong to
// the unit's process.  A block-diagonal operand is one unit, a cross operand two (its columns in process 0 / in process 1).
struct CkFisherUnit {
    double* D;
    long c0, wpad, nlo, nhi;
    int pK0, npan;
};
// the assembly's view: D[op][r] = the unit of dense operand op whose columns lie in process r (null: not wanted)
struct CkFisherAsm {
    double* D[CK_FOP_DIAG0][2];
    long c0[2], wpad[2];
    int pK0[2];
};
#define CK_FOPK_NONE 0
#define CK_FOPK_DENSE 1
#define CK_FOPK_DIAG0 2   // + process
// the contraction's view of a product: B[r ld + (c - c0)] for c in [c0, c0 + w), zero elsewhere; a diagonal operand is read
// from Sigma^-1 itself
struct CkFisherOp {
    const double* B;
    long ld, c0, w;
    int kind;
};
struct CkFisherOps {
    CkFisherOp op[CK_FISHER_NOPS];
    unsigned mask[CK_FISHER_NOPS];   // mask[a] bit b (a <= b): the pair (a, b) is wanted
};
struct CkFisherCtx {
    const double* Sp;   // Sigma^-1 as full K-panels (ck_launch_fisher_expand)
    const double* d;    // npad measurement-error variances in the internal order (may be null without a diagonal operand)
    long npad, n0p;
    int n_procs;
};
// G_dev: the packed lower block columns of -Sigma^-1 (ck_launch_ginv_syrk with a zero start) -> Sp, npad x npad doubles
void ck_launch_fisher_expand(hipStream_t s, double* const* G_dev, CkLayout L, double* Sp);
// the units' buffers must be zero; blk5 / dnu3 / c as ck_launch_loglik_grad
void ck_launch_fisher_assemble(hipStream_t s, const CkFisherAsm& A, CkLayout L, int n_procs, int metric, const double* c,
                               const CkMatern* blk5, const double* dnu3);
// C (npad rows, ldc; its columns [0, U.wpad)) -= Sigma^-1[:, panels of U] D_U on the trailing updates' MFMA tile (ck_la.hip)
void ck_launch_fisher_prod(hipStream_t s, double* C, int64_t ldc, const double* Sp, int64_t npad, const double* D, int64_t wpad,
                           int pK0, int npan);
// part: CK_FISHER_NPAIR doubles per workgroup (ck_fisher_contract_groups of them), pair (a <= b) at b (b + 1) / 2 + a
int64_t ck_fisher_contract_groups(int64_t npad);
void ck_launch_fisher_contract(hipStream_t s, const CkFisherOps& O, const CkFisherCtx& X, double* part);
// REML: Y = D H into the K-panel operand Yp (rows row0 .. row0 + p - 1), and the sums over the sites out = Y^T R
void ck_launch_fisher_dh(hipStream_t s, const CkFisherUnit& U, const double* H, int p, int row0, double* Yp);
void ck_launch_fisher_dh_diag(hipStream_t s, CkLayout L, int n_procs, int proc, const double* d, const double* H, int p, int row0,
                              double* Yp);
void ck_launch_fisher_ytv(hipStream_t s, const double* Yp, int64_t npad, const double* R, int64_t ldr, int ncols, double* out,
                          int64_t ldo);

// ---- conditional simulation (ck_draws.hip) ---------------------------------------------------
// on the Schur buffers sch[J] (packed block columns of S, nJ of them), sites k < m:
// mask[k] = S_kk <= thr; S_kk = 1 where deflated, else S_kk + jit
void ck_launch_draw_deflate(hipStream_t s, double* const* sch, int nJ, int64_t m, double thr, double jit, unsigned char* mask);
// the same on the stacked sites of both processes (ck_conditional_draws_pair): process 0 in [0, m0), process 1 in [m0p, m), each
// with its own thr[k] / jit[k]; the gap rows [m0, m0p) get mask 2 -- deflated for good, no caller column -- and keep their 1
void ck_launch_draw_deflate_pair(hipStream_t s, double* const* sch, int64_t m0, int64_t m0p, int64_t m, const double thr[2],
                                 const double jit[2], unsigned char* mask);
// the strictly lower entries of the deflated sites' rows and columns -> 0
void ck_launch_draw_zero(hipStream_t s, double* const* sch, int nJ, int64_t m, const unsigned char* mask);
// above the diagonal of the nJ diagonal blocks -> 0 (after the factorisation, in front of ck_launch_draw_trmm)
void ck_launch_draw_upper(hipStream_t s, double* const* sch, int nJ);
// E = -eps of draws d0 .. d0 + nd - 1 (ldp x Mp, block columns of ld NB; 0 beyond nd, beyond m and at deflated sites):
// noise (nd x ldn, the caller's order) if given, else the Philox normals of ck_rng.h keyed on seed, counter (cmap[j], d / 2).
// ldn (0: m): the caller's number of sites where it is not m
void ck_launch_draw_noise(hipStream_t s, double* E, int64_t ldp, int64_t Mp, int64_t nd, int64_t m, int64_t d0, const int* cmap,
                          const unsigned char* mask, const double* noise, uint64_t seed, int64_t ldn = 0);

// ---- leave-group-out cross-validation (ck_la.hip: the Gram kernel; ck_folds.hip: the fold solves) ------------------
// Q_SS = W_S W_S^T of every fold, one workgroup per tile of the host's tile map (ck_host.h: CkFoldPlan): rows grow[a0 ..] and
// grow[b0 ..] of the solved right-hand sides (grow: the gather list as ROW indices of aux, all >= 1), product at out + c_off
// (ld), panels pos0 / CK_NB .. nK - 1.  mpad CK_NB 8 < 2^31 (a row's byte offset inside a panel is a 32-bit register).
void ck_launch_fold_gram(hipStream_t s, const double* aux, int64_t mpad, int nK, const CkFoldTile* tiles, int64_t n_tiles,
                         const int* grow, double* out);
// dots[row] = W_row . y (k_reduce_pred, raw mode).  Outputs indexed like the gather list: x = Q_SS^-1 alpha_S, d = diag(Q_SS^-1);
// stat2[2 f], stat2[2 f + 1] = log|Q_SS|, alpha_S^T Q_SS^-1 alpha_S; fail[f] = 1 where Q_SS did not factor (outputs NaN)
void ck_launch_fold_small(hipStream_t s, const CkFoldSmall* folds, int64_t n, const double* buf, const int* grow,
                          const double* dots, double* x_out, double* d_out, double* stat2, int* fail);
void ck_launch_fold_big_fill(hipStream_t s, const CkFoldBig* sys, int n_sys, int kq_max, double* buf, const int* grow,
                             const double* dots);
void ck_launch_fold_big_reduce(hipStream_t s, const CkFoldBig* sys, int n_sys, int s_max, const double* buf, const long long* info,
                               double* x_out, double* d_out, double* stat2, int* fail);

// ---- empirical variogram (ck_vario.hip) ----------------------------------------------------
#ifndef CK_VG_JSUB
#define CK_VG_JSUB 128   // "j" points of a sub-chunk: the unit of the level-window decision (and of the third set of bounding
                         // balls).  Bin pass at 1 M soundings: 64 -> 85.5 ms, 128 -> 80.9, 256 -> 87.1, 512 -> 122.5 (smaller blocks,
                         // narrower windows, more set-up); at 4 M soundings 128 and 256 are within 2 %
#endif
#ifndef CK_VG_JCHUNK
#define CK_VG_JCHUNK 1024   // "j" points of a wave's pair tile: the unit of the first culling test and of the tile -> wave deal
#endif
#define CK_VG_MAXBINS 60   // levels sit one per lane of a wave (ck_vario.hip); a few lanes of slack for the windows
struct CkVarioExt {
    double rmin, rmax;
    long long imin, jmin, imax, jmax;
};
// CkVarioPair (a pair the kernels leave to the host): ck_host.h
void ck_launch_vario_prep(hipStream_t s, const double* coords, int64_t n, int metric, double* u0, double* u1,
                          double* u2);
int ck_vario_bin_grid(int64_t ni, int64_t nj);   // workgroups of the three pair passes (wave tiles of 64 x 1024 points)
// iu / ju: 3 x n SoA (unit vectors | x, y, 0); part: CkVarioExt[grid]; q = squared chord | squared distance;
// ib64 / jb1024 / jbsub: bounding balls of the 64-point "i" blocks, 1024-point "j" chunks and 128-point sub-chunks
void ck_launch_vario_extent(hipStream_t s, int grid, int same, const double* iu, int64_t ni, const double* ju,
                            int64_t nj, double qcap, void* part, int rank, int world, const double* ib64,
                            const double* jb1024, const double* jbsub, double cmax, unsigned long long* best /* 2 words */,
                            double qwin_lo /* pairs with qwin_lo <= q <= qcap go to the list */, CkVarioPair* list, unsigned* count,
                            unsigned cap);
void ck_launch_vario_collect(hipStream_t s, int grid, int same, const double* iu, int64_t ni, const double* ju,
                             int64_t nj, double qtop_lo, double qcap, double qbot_hi, CkVarioPair* list, unsigned* count,
                             unsigned cap, int rank, int world, const double* ib64, const double* jb1024,
                             const double* jbsub);
// tile culling (ck_vario.hip): bounding balls of blocks of `blk` consecutive points, 4 x nblk doubles
int64_t ck_vario_nblocks(int64_t n, int blk);
void ck_launch_vario_bounds(hipStream_t s, const double* u, int64_t n, int blk, double* out);
// levels 1 .. nlev (xa / xb / dthr indexed by level; x = q (Euclid) or q / 2 - 1 (haversine), see ck_vario.hip);
// counts: CK_VG_MAXBINS + 1 words, the last = pairs visited; args_dev: CK_VG_ARGS_BYTES of device memory
#define CK_VG_ARGS_BYTES 256
void ck_launch_vario_bin(hipStream_t s, int metric, int same, int covariogram, const double* iu, const double* iv,
                         int64_t ni, const double* ju, const double* jv, int64_t nj, int nlev, const double* xa,
                         const double* xb, const double* dthr, double cmax, const double* ib64, const double* jb1024,
                         const double* jbsub, int grid, double* part_sum, unsigned long long* part_cnt, CkVarioPair* list,
                         unsigned* count, unsigned cap, int rank, int world, int nb, double* sums, long long* counts,
                         void* args_dev);

// ---- local-neighbourhood cokriging (ck_local.hip) -------------------------------------------
// One workgroup per point (or per tiled system).  Every launch that searches, assembles or solves is told about the call by
// ONE descriptor, filled once per call by ck_api.hip and passed to the kernels by value; a launcher's other arguments are
// what differs between launches (the point range, outputs, scratch).  ck_local.hip's header lists the steps and which kernel
// composes which.
void ck_launch_local_chunk_bounds(hipStream_t s, const double* su, CkLayout L, double* cb);
struct CkLocalProblem {
    // the model: the Matern blocks and their tables (ck_math.h "Tabulated covariance"; use_tab 0: exact formulas only)
    const CkMatern* blk = nullptr;
    const CkTable* tabs = nullptr;          // [3]
    const double* const* coefs = nullptr;   // [3]
    int use_tab = 0;
    int metric = 0, i_pred = 0;
    // cv: the search has a lower cut -- a site of process q at d <= lo[q] is no neighbour (lo[q] = -1: none for that process).
    // The reference's cross-validation flag is lo[i_pred] = 0: sites of process i_pred at distance 0 are no neighbours
    int cv = 0;
    double lo[2] = {-1.0, -1.0};
    double max_dist = 0.0;
    double c0var = 0.0;                     // the prior variance of process i_pred
    // the sites, internal order: sc = 3 x npad coordinates (exact-formula form), su = their chord vectors, z = the values,
    // nz = ck_set_noise's s d, added to the diagonal of every local system (null: off)
    const double *sc = nullptr, *su = nullptr, *z = nullptr;
    CkLayout L{};
    const double* nz = nullptr;
    // the points: pc = 3 x mpad coordinates, pu = their chord vectors
    const double *pc = nullptr, *pu = nullptr;
    int64_t mpad = 0;
    // the search: cb = chunk bounds of the sites (ck_launch_local_chunk_bounds: 4 x ceil(nend / 256) doubles), cmax = largest
    // chord (distance in the space of su / pu) a neighbour can have, with its safety margin.
    // Neighbour cap: rq = m x 2 cut distances, cp = m culling chords, as the select pass left them (both null: no cap, every
    // point reaches max_dist / cmax).  Precedence (ck_loglik_vecchia): rs = every site's position in the caller's ordering
    // (npad ints), rp = the points' (mpad ints); a site is searched only if rs[site] < rp[point] (both null: no condition).
    const double* cb = nullptr;
    double cmax = 0.0;
    const double *rq = nullptr, *cp = nullptr;
    const int *rs = nullptr, *rp = nullptr;
    // Withholding (ck_cv_local_folds), evaluated where the radius predicate is, so in front of the cap.  Fold: fs = one label
    // per site (npad ints, internal order; -1 in padding and for data never withheld), fp = one label per point (mpad ints); a
    // site is no candidate of a point when fs[site] >= 0 && fs[site] == fp[point] (both null: no condition, no label is
    // loaded).  Buffer: the radius of process q is the lower cut lo[q] above (cv set).  listed: rs or fs is set.
    const int *fs = nullptr, *fp = nullptr;
    int listed = 0;
    // Block cokriging (ck_predict_local_blocks): the points are the blocks' search centres.  bo = r + 1 offsets into the member
    // rows, the members grouped by block in the caller's order; mc = 3 x bmpad member coordinates (exact-formula form), mu =
    // their chord vectors, bw = their weights; sbb = the r prior variances of the block means (in place of c0var).  All null
    // for the point calls.
    const int* bo = nullptr;
    const double *mc = nullptr, *mu = nullptr, *bw = nullptr, *sbb = nullptr;
    int64_t bmpad = 0;
};
// neighbour count of the points [0, m) (an uncapped call's counting pass)
void ck_launch_local_count(hipStream_t s, const CkLocalProblem& P, int64_t m, int* counts);
// The neighbour cap (ck_set_local_neighbours; include/cokrige.h has the rule).  ck_launch_local_select is the counting pass
// of a capped call: per point and process the cut distance r_pq (rq: m x 2; max_dist where the cap does not bind) and the
// final counts (sel: m x 4 ints -- neighbours of process 0, of process 1, candidates before the cap, flags), their sum in
// counts, and the point's culling chord cp (the chord of max(r_p0, r_p1) with cmax's margin; cmax itself where that is
// max_dist).  key_cap: candidates per process kept in LDS (option "local_select_cap"); a process with more runs the same
// rounds re-scanning its chunks.  The pass itself searches within max_dist / cmax whatever P.rq / P.cp hold (they are
// usually the very buffers it fills); it honours the precedence pointers.
#define CK_LS_CAPPED 1   // sel flags: the cap binds for some process of the point
#define CK_LS_RESCAN 2   //            some process had more candidates than key_cap
int ck_local_select_capacity();
void ck_launch_local_select(hipStream_t s, const CkLocalProblem& P, int64_t m, int nmax0, int nmax1, int key_cap, int* counts,
                            int* sel, double* rq, double* cp);
// points [p_base, p_base + m).  slab_off[p]: offset (doubles) of point p's scratch slab ((k + 2) k doubles + k ints) when its
// neighbourhood exceeds the LDS limit, relative to `slab` within this batch; vv: the raw v . v of every solved point, or null
void ck_launch_local_solve(hipStream_t s, const CkLocalProblem& P, int64_t p_base, int64_t m, const int* counts,
                           const long long* slab_off, double* slab, int k_hi, double* pred, double* err, double* vv);
int ck_local_lds_limit();
// The Vecchia likelihood's terms (ck_loglik_vecchia), n data in the caller's stacked order: from (z, mu, v . v, prior variance,
// own noise -- null: none --, the two counts) to mean / var per datum and, by a fixed tree over part (2 x ceil(n / 256) doubles)
// and bad (ceil(n / 256) words), out2 = (sum log var, sum e^2 / var) and *info = 1 + the first datum without a term (0: none)
void ck_launch_vecchia_terms(hipStream_t s, int64_t n, const double* z, const double* mu, const double* vv, const double* prior,
                             const double* noise, const int* cnt2, double* mean, double* var, double* part, long long* bad,
                             double* out2, long long* info);
// The gradient of the Vecchia likelihood (ck_loglik_vecchia_grad; ck_vecchia_grad.h): k_vecchia_grad runs k_local_solve's steps
// (the same device functions: same pred / err / vv bits; an empty set writes NaN, NaN as there) on sets of at most
// ck_local_lds_limit() data, points [0, m), followed by the back substitution and the contraction.
// gself: the m points' own internal site indices; dvar: the raw measurement-error variances
// d in the internal order (npad) or null; score: m x CK_VG_NPAR, the points' order.  ck_launch_vecchia_grad_sum: column sums of
// n scores by the fixed tree of the terms (part: CK_VG_NPAR x ceil(n / 256) doubles).
struct CkVecchiaGradArgs {
    CkVecchiaModel V;
    const int* gself;
    const double* dvar;
    double* score;
};
void ck_launch_vecchia_grad(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, double* pred, double* err,
                            double* vv, CkVecchiaGradArgs A);
void ck_launch_vecchia_grad_sum(hipStream_t s, int64_t n, const double* score, double* part, double* out13);
// The expected information of the Vecchia likelihood (ck_loglik_vecchia_fisher; ck_vecchia_info.h): k_vecchia_info runs
// k_vecchia_grad's steps up to the back substitution on the points [0, m), ck_vecchia_info_run() consecutive points per
// workgroup, then the product D b, the forward substitution and the combination.  Workgroup w writes row row0 + w of part
// (CK_VI_NTRI sums) and of bad (1 + stacked0 + the first of its points without a term; 0: none).  gself, dvar: as above.
// ck_launch_vecchia_info_sum: column sums of n_rows rows by the fixed tree of the scores (part: CK_VI_NTRI x ceil(n_rows / 256)).
struct CkVecchiaInfoArgs {
    CkVecchiaModel V;
    const int* gself;
    const double* dvar;
    double* part;
    long long* bad;
    long long row0, stacked0;
};
int ck_vecchia_info_run();
void ck_launch_vecchia_info(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkVecchiaInfoArgs A);
void ck_launch_vecchia_info_sum(hipStream_t s, int64_t n_rows, const double* rows, double* part, double* out91);
// The Vecchia likelihood with a GLS trend (ck_loglik_vecchia_trend; ck_vecchia_trend.h).  ck_launch_vecchia_trend: k_local_solve's
// steps on sets of at most ck_local_lds_limit() data, points [0, m), with the p = Tr.p0 + Tr.p1 trend rows riding along (Tr.f0
// unused): mu = v . y, vv = v . v (ck_loglik_vecchia's bits) and g (m x p) = v . U_j per point; a point with an empty set is left
// as it was, one whose system is not positive definite gets NaN.  ck_launch_vecchia_trend_terms: ck_launch_vecchia_terms plus
// every datum's row (CkVecchiaTrendRows) in the caller's stacked order.  ck_launch_vecchia_trend_gram: out_tri (CK_VT_NTRI
// doubles) = the lower triangle of sum_t r_t r_t^T by a fixed tree (part: CK_VT_NTRI x ceil(n / 256) doubles).
// ck_launch_vecchia_residual: out = z - sum_j beta_j X[j] over npad sites of the internal order.
struct CkVecchiaTrendRows {
    int p;
    int64_t npad;
    const double* X;     // d_trendX: p rows of npad doubles, internal site order
    const int* gself;    // every datum's own internal site index, stacked order
    const double* g;     // n x p, stacked order
    double* rows;        // n x (1 + p), stacked order
};
struct CkVecchiaTrendBeta {
    double b[CK_VT_PMAX];
};
struct CkLocalTrend;   // below: the universal form of the local predictor
void ck_launch_vecchia_trend(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkLocalTrend Tr, double* mu,
                             double* vv, double* g);
void ck_launch_vecchia_trend_terms(hipStream_t s, int64_t n, const double* z, const double* mu, const double* vv, const double* prior,
                                   const double* noise, const int* cnt2, CkVecchiaTrendRows T, double* mean, double* var,
                                   double* part, long long* bad, double* out2, long long* info);
void ck_launch_vecchia_trend_gram(hipStream_t s, int64_t n, int p, const double* rows, double* part, double* out_tri);
void ck_launch_vecchia_residual(hipStream_t s, int64_t npad, int p, const double* z, const double* X, CkVecchiaTrendBeta B,
                                double* out);

// Large neighbourhoods (k > k_hi above): the "tiled" path.  The systems of a batch are factored TOGETHER,
// 64 columns per step, by launches over all systems that still have columns left (diagonal block + its
// inverse, row solves, trailing update on 128 x 128 MFMA tiles) -- the tile kernels of the joint path with a
// system index in the grid.  A system's scratch (slab + off):
//   S     CK_LT_ROWS(kq) rows x ld doubles, ld = kq + 128, kq = k + 2 rounded up to 64: ONE padded symmetric
//         matrix.  Rows/cols [0, k): local covariance (lower triangle); [k, kq - 2): identity padding; rows
//         kq - 2 and kq - 1: the c and z rows, which ride along as in the other local kernels -- here as two
//         more matrix rows with a huge diagonal (CK_LT_BIG), so that the Cholesky recurrences themselves do
//         their forward substitution (L[r][j] = (S[r][j] - sum) / L[j][j]) and never see a bad pivot there.
//         The 128 rows / columns beyond kq exist only so that whole tiles can be read and written without
//         bounds checks; nothing valid depends on them.
//   Linv  CK_LT_NINV x 64 x 64 doubles (inverses of the diagonal blocks of the current column group)
//   idx   k ints (neighbour list)
// CkLocalSys, CK_LT_ROWS, CK_LT_NINV and the sizes ck_local_tiled_kq / ck_local_tiled_doubles: ck_host.h (the host plans with them)
#define CK_LT_BIG 1e200
// pair: the three rows of ck_predict_local_pair behind the padding (kq = roundup(k + 3, 64)) in place of c and z
void ck_launch_local_assemble_t(hipStream_t s, const CkLocalProblem& P, const CkLocalSys* sys, int n_sys, double* slab,
                                int* k0buf /* n_sys ints: the process-0 neighbour counts */, bool pair = false);
// Columns are processed in groups of g 64-column blocks [g0, g0 + 64 g): block i of a group first receives the
// updates of the group's earlier blocks (one pass, K = 64 i), then its diagonal block is factored and inverted and
// the rows below are solved; the trailing matrix behind the group is updated once with K = 64 g (a g-th of the
// read-modify-write traffic of updating after every block).  Systems sorted by k descending: the first n_active
// are the ones that still have the block / trailing columns in question.
void ck_launch_local_tiled_block(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int i,
                                 const int* kq_host, long long* info, int group_blocks);
// the rows BELOW the group's diagonal region, through all of the group's blocks in one launch (group_blocks of them)
// kq_host: the padded sizes of the batch's systems on the host (largest first): the launches have exactly one workgroup
// per chunk / tile that exists (ck_tilemap.h)
void ck_launch_local_tiled_rows_all(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0,
                                    int group_blocks, const int* kq_host);
void ck_launch_local_tiled_trailing(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int K,
                                    const int* kq_host);
// left-looking form (round 4, option "local_left" = 1, the default): the columns [g0, g0 + W) of every system, rows g0 .., receive
// all updates from the columns to their left in ONE pass (K = g0) before the group is factored; W <= 256
void ck_launch_local_tiled_left(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int W,
                                const int* kq_host);
// sbb (here and in ck_launch_local_reduce_ut): the prior variance per point in place of c0var (block cokriging), or null
void ck_launch_local_reduce_t(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab,
                              const long long* info, double c0var, double* pred, double* err, double* vv /* or null */,
                              const double* sbb = nullptr);

// Universal cokriging in the neighbourhood (ck_predict_local_universal): the p = p0 + p1 trend rows X_loc^T ride along each
// local factorisation like c and z, and a GLS step per point (ck_local_gls.h) follows the reduction.
//   LDS class (k <= 64): k_local_solve_u, a (k + 2 + p) x k matrix -- rows k (c), k + 1 (z), k + 2 .. (trend) -- in dynamic
//   LDS sized by p;  tiled class: kq = roundup(k + 2 + p, 64), the trend rows in [kq - 2 - p, kq - 2), each with its own
//   CK_LT_BIG diagonal entry; the batched factorisation steps are those of the simple form.
#define CK_LU_PMAX 16   // 2 CK_TREND_PMAX (include/cokrige.h)
struct CkLocalTrend {
    const double* X;    // p rows of npad doubles in the internal site order (ck_api.hip: d_trendX)
    const double* f0;   // m x p_i regressors of the predicted process at the prediction points, finite
    int p0, p1;         // trend columns of process 0 / process 1
    double tol;         // relative pivot threshold of the GLS step
};
// status[p] of a point (beta: m x p, NaN rows unless CK_LU_OK; dropped columns NaN)
#define CK_LU_OK 0
#define CK_LU_EMPTY 1
#define CK_LU_NOT_PD 2
#define CK_LU_RANK_DEF 3
void ck_launch_local_solve_u(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, int k_hi, CkLocalTrend Tr,
                             double* pred, double* err, double* beta, int* status);
// behind ck_launch_local_assemble_t: the trend rows of the batch's systems
void ck_launch_local_trend_rows_t(hipStream_t s, const CkLocalSys* sys, int n_sys, double* slab, CkLayout L, CkLocalTrend Tr);
// k0buf: the process-0 neighbour counts ck_launch_local_assemble_t left
void ck_launch_local_reduce_ut(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab, const long long* info,
                               const int* k0buf, int i_pred, double c0var, double* pred, double* err, CkLocalTrend Tr,
                               double* beta, int* status, const double* sbb = nullptr);
// Block cokriging in the neighbourhood (ck_predict_local_blocks), LDS class: k_local_solve_u's steps with the c row replaced by
// cbar_g = sum_a w_a C(x_a, s_g) over the block's members (P.bo .. P.sbb set), the neighbourhood that of the block's centre.
// No trend (Tr.p0 + Tr.p1 == 0): k_local_solve's outputs (status and beta may be null).  The tiled class: ck_launch_local_assemble_t
// writes cbar where P.bo is set; the reductions take P.sbb.
void ck_launch_local_solve_b(hipStream_t s, const CkLocalProblem& P, int64_t r, const int* counts, int k_hi, CkLocalTrend Tr,
                             double* pred, double* err, double* beta, int* status);

// Both processes at every point from one local system (ck_predict_local_pair; include/cokrige.h has the definition).  The c rows of
// process 0 and 1 and z ride along one factorisation: LDS class k_local_solve_pair, a (k + 3) x k matrix; tiled class kq =
// roundup(k + 3, 64) with the rows kq - 3, kq - 2, kq - 1 (ck_launch_local_assemble_t with pair, the factorisation steps
// unchanged, ck_launch_local_reduce_pair_t).  Outputs per point: lp_write's of either process and cov = c01 - v0 . v1.
struct CkLocalPairOut {
    double *pred0, *err0, *pred1, *err1, *cov;   // m doubles each
    double c0var[2];                              // sigma_q^2 + nugget_q
    double c01;                                   // C_01(0), no nugget
};
void ck_launch_local_solve_pair(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, int k_hi,
                                const CkLocalPairOut& O);
void ck_launch_local_reduce_pair_t(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab, const long long* info,
                                   const CkLocalPairOut& O);

// Conditional simulation in the moving neighbourhood (ck_simulate_local; include/cokrige.h has the definition).  The sites are
// the points of a pass over the AUGMENTED data set (the data, then the sites as noise-free pseudo-data of process i_pred), with
// the precedence pointers set: P.rs < n_data for a datum, n_data + position in the ordering for a site.
// k_local_sim_weights (one workgroup per site, sets of at most ck_local_lds_limit() members): k_vecchia_grad's steps 1 - 5 on the
// same device functions, then the weights w = Sigma_loc^-1 c kept instead of contracted.  Per site p, rows of LP_KL entries:
//   gidx / w    the set's members in list order (internal index of the augmented set; -1 / 0 beyond the set) and their weights
//   spos / sw   the members that are earlier sites, in list order: their positions and weights (-1 / 0 beyond ns[p])
//   mu          sum of w_a z_a over the data of the set, in list order;  s2 = c0var - c . w, raw
// A local system that is not positive definite: NaN weights, mu and s2.  An empty set: mu = 0, s2 = c0var, ns = 0.
struct CkLocalSimOut {
    int n_data;
    int *gidx, *spos, *ns;
    double *w, *sw, *mu, *s2;
};
void ck_launch_local_sim_weights(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkLocalSimOut O);
// k_local_sim_level: the sites order[0 .. n) of one level (the caller's indices), draws d0 .. d0 + nd - 1 of the call:
//   Y[pos[t]][d] = mu[t] + sum_j sw[t][j] Y[spos[t][j]][d] (list order) + s_t eps[d][t],   s_t = sqrt(s2[t]), NaN unless s2[t] > 0
// Y: [position][draw], ldy doubles per position (even, >= nd; the draws beyond nd are scratch).  eps: with eps_in_y what the
// site's own row of Y holds (the caller's noise, put there by ck_launch_local_sim_gather: the reads run along the draws like
// every other), else the Philox normals of ck_rng.h keyed on seed, counter (t, (d0 + d) / 2); d0 is even, a thread makes the
// pair (d, d + 1).  Every input row was written by an earlier launch on the same stream: no waiting inside the kernel.
struct CkLocalSimLevel {
    const int *pos, *ns, *spos;
    const double *sw, *mu, *s2;
    double* Y;
    long ldy, d0;
    int eps_in_y;
    unsigned long long seed;
};
void ck_launch_local_sim_level(hipStream_t s, const CkLocalSimLevel& A, const int* order, int64_t n);
// Y (positions x ldy) <- E (nd x m, the caller's order), zeros in the draws nd .. ldy - 1
void ck_launch_local_sim_gather(hipStream_t s, const double* E, int64_t m, int64_t nd, const int* pos, double* Y, int64_t ldy);
// X (nd x m, the caller's order) <- Y (positions x ldy)
void ck_launch_local_sim_scatter(hipStream_t s, const double* Y, int64_t ldy, const int* pos, int64_t m, int64_t nd, double* X);

// Leave-group-out cross-validation in the moving neighbourhood (ck_cv_local_folds).  ck_launch_cv_labels: fs (npad ints, all -1
// at launch) <- the labels of both processes (fold0: n0, fold1: n1, the caller's order; either may be null) at every datum's own
// internal position (gself: n0 + n1 ints, stacked order, all < npad).  ck_launch_cv_fold_scores: one workgroup per group g of
// predicted data, idx[off[g] .. off[g + 1]) positions in the call's point list; z / pred / err / own (null: no noise) are indexed
// by those positions; out: n_groups x CK_CV_NSCORE -- data scored, sum e, sum e^2, sum e^2 / v, sum log v.
#define CK_CV_NSCORE 5
struct CkCvScoreArgs {
    const int* idx;
    const long long* off;
    const double *z, *pred, *err, *own;
    double* out;
};
void ck_launch_cv_labels(hipStream_t s, int64_t n0, int64_t n1, const int* fold0, const int* fold1, const int* gself, int* fs);
void ck_launch_cv_fold_scores(hipStream_t s, int64_t n_groups, CkCvScoreArgs A);
