/* cokrige.h -- C ABI of libcokrige_hip.so, the MI355X (gfx950) numeric core of
 * the bivariate Matern cokriging predictor.
 *
 * The reference (91Mrwu/sif-xco2-cokriging) is pure Python and has no FFI of its
 * own; its drop-in boundary is the Python class API
 *     joint_prediction.Predictor   (src/joint_prediction.py:13-92)
 *     point_prediction.Predictor   (src/point_prediction.py:21-96)
 *     MultivariateMatern.covariance/cross_covariance (src/model.py:193-207)
 *     fields.distance_matrix       (src/fields.py:318-342)
 *     MultiField.empirical_variograms (src/fields.py:192-252)
 * Each entry point below names the reference lines whose arithmetic it
 * replaces.  The Python host layer in sif-xco2-cokriging_amd/ binds these
 * symbols with ctypes (see INTEGRATION.md for the stub a maintainer of the
 * reference would add).
 *
 * Conventions
 *   - every function returns int: 0 = ok, < 0 = error (text from
 *     ck_last_error(), thread local).  Numerical failure of the Cholesky
 *     factorisation is NOT an error code: it is reported LAPACK-style through
 *     `info` (1-based index of the first non-positive pivot, 0 = success).
 *   - "host" pointers are caller-owned, C-contiguous float64 (numpy) buffers,
 *     read or written during the call and never retained.
 *   - "dev" pointers are device addresses (e.g. torch.Tensor.data_ptr()).
 *   - coordinates are rows [lat, lon] in degrees for CK_METRIC_HAVERSINE
 *     (fast_dist=True, km) or [x, y] for CK_METRIC_EUCLID (src/fields.py:326-342).
 *   - a handle owns one GPU and one HIP stream; it is not thread-safe, distinct
 *     handles may be used from distinct threads.
 */
#ifndef COKRIGE_H
#define COKRIGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ck_handle ck_handle;

#define CK_METRIC_HAVERSINE 0 /* fast_dist=True : 6371 km * haversine (src/fields.py:332-336) */
#define CK_METRIC_EUCLID 1    /* fast_dist=False, units=None : Euclidean (src/fields.py:340-342) */

#define CK_APPLY_SIGMA 1 /* ck_panel_apply: update the local trailing block columns of Sigma */
#define CK_APPLY_AUX 2   /* ck_panel_apply: forward-substitute / update the right-hand-side rows */
/* Every panel buffer (ck_panel_buffer: the owner's storage or a receive slot) is followed by this many bytes the
 * library never reads or writes: room for the host to pad a panel to a multiple of world x 4 KB, so that the exchange
 * can be an in-place all-gather of equal pieces (distributed.py, exchange = "sag"). */
#define CK_PANEL_SLACK_BYTES (64 * 512 * 8)

/* ---- library ------------------------------------------------------------- */
const char* ck_last_error(void);
int ck_version(void);
int ck_device_count(int* n);

/* ---- handle ---------------------------------------------------------------- */
int ck_create(int device_id, ck_handle** out);
/* The multi-GPU form of ck_create (SURVEY.md section 8b lists ck_create(device_ids, n_dev, ...)): the run is one process
 * -- one handle -- per GPU; every rank passes the SAME device list and its own rank and gets a handle on device_ids[rank]
 * that is already partitioned (ck_set_partition(rank, n_dev)).  The panels then travel between the ranks' ck_panel_buffer
 * addresses by whatever the host framework provides (RCCL under torch.distributed in distributed.py / workers.py). */
int ck_create_partitioned(const int* device_ids, int n_dev, int rank, ck_handle** out);
int ck_destroy(ck_handle* h);
/* external != 0: launch on the caller's HIP stream (hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream; NULL is the legacy default stream, which is what
 * torch uses unless told otherwise).  external == 0: back to the handle's own stream. */
int ck_set_stream(ck_handle* h, void* hip_stream, int external);
/* Let the caller provide all device storage (e.g. one torch uint8 tensor), so a
 * host framework owns the memory and can run collectives on slices of it.
 * Without an arena the library allocates with hipMalloc.  Must precede ck_set_data. */
int ck_set_arena(ck_handle* h, void* dev_base, int64_t nbytes);
int ck_synchronize(ck_handle* h);
/* Device bytes the handle will allocate for the data set so far, the current partition and
 * `m` prediction points (size an arena with it; call after ck_set_data/ck_set_partition). */
int ck_estimate_bytes(ck_handle* h, int64_t m, int64_t* out);

/* ---- model and data ------------------------------------------------------- */
/* Matern parameters in the reference's order (src/model.py:122-130,145-152):
 * sigma[n_procs], nu[3] = (11, 12, 22), len_scale[3] = (11, 12, 22),
 * nugget[n_procs], rho12.  n_procs = 1: nu[0], len_scale[0] only. */
int ck_set_model(ck_handle* h, int n_procs, const double* sigma, const double* nu, const double* len_scale,
                 const double* nugget, double rho12);
int ck_set_metric(ck_handle* h, int metric);
/* 1-D block-column-cyclic ownership of Sigma over `world` processes (one GPU
 * each); prediction points are sharded by the caller.  Default (0, 1). */
int ck_set_partition(ck_handle* h, int rank, int world);
/* Observation sites of process k: coords (n_k x 2), values (n_k): Field.coords_main /
 * Field.values_main (src/fields.py:78-81, consumed at src/joint_prediction.py:53-55,106-111,130-132). */
int ck_set_data(ck_handle* h, int k, const double* coords_host, const double* values_host, int64_t n_k);

/* ---- element-wise parity surface (tests, and the model/fields mirrors) ----- */
/* fields.distance_matrix(A, B) (src/fields.py:318-342) -> out (a x b). */
int ck_distance_dense(ck_handle* h, const double* A_host, int64_t a, const double* B_host, int64_t b,
                      double* out_host);
/* covariance(i, D(A,B), use_nugget) if i == j else cross_covariance(i, j, D(A,B))
 * (src/model.py:193-207 on src/fields.py:318-342) -> out (a x b). */
int ck_cov_dense(ck_handle* h, int i, int j, const double* A_host, int64_t a, const double* B_host, int64_t b,
                 int use_nugget, double* out_host);
/* the same at given lags h[n] (MultivariateMatern.covariance / cross_covariance on an array). */
int ck_cov_lags(ck_handle* h, int i, int j, const double* lags_host, int64_t n, int use_nugget, double* out_host);
/* Model (cross-)variograms row by row -- the "fit" column of MultivariateMatern._map_fit and the
 * curves of variograms() / FittedVariogram (src/model.py:209-260, 330-331): row r has process pair
 * (i[r], j[r]) and lag h[r]; kind 0: semivariance(i, h) if i == j else cross_semivariance(i, j, h);
 * kind 1 ("covariogram"): covariance(i, h) incl. nugget at h == 0 / cross_covariance(i, j, h). */
int ck_model_variogram(ck_handle* h, const int32_t* i_host, const int32_t* j_host, const double* lags_host, int64_t n,
                       int kind, double* out_host);

/* ---- joint (global) cokriging: src/joint_prediction.py:35-153 --------------- */
/* K1: assemble the lower block triangle of Sigma = [[C11, C12], [C12^T, C22]] for the
 * locally owned block columns (Predictor._joint_cov, src/joint_prediction.py:124-153). */
int ck_assemble_joint(ck_handle* h);
/* K3: in-place blocked Cholesky Sigma = L L^T (cho_factor(lower=True), src/joint_prediction.py:69).
 * info = 0, or the 1-based order of the leading minor that is not positive definite
 * (scipy raises LinAlgError with that number).  Single-process form; for world > 1 drive
 * ck_panel_factor / ck_panel_apply from the host with a broadcast in between.
 * The rows below a 64 x 64 diagonal block are solved as a product with that block's explicit inverse, so the backward error of
 * L grows with the condition number of the diagonal blocks: DESIGN.md section 4b, "Stability of the inverse-based row solves". */
int ck_factor(ck_handle* h, int64_t* info);
/* K2 + K4: prediction and standard error of process i at pcoords (m x 2):
 * c0 (Predictor._pred_cross_cov, :104-122), forward substitution V = L^-1 [c0 | z],
 * pred = V^T y, pred_err = nan_to_num(sqrt(sigma_i^2 + nugget_i - |V_k|^2)) (:68-78).
 * Needs ck_factor; may be called repeatedly. */
int ck_predict(ck_handle* h, int i, const double* pcoords_host, int64_t m, double* pred_host, double* pred_err_host);
/* ck_factor + ck_predict in one call, for a Sigma that is assembled and not yet factored (Predictor.__call__,
 * src/joint_prediction.py:60-78, does exactly this sequence): the factorisation and the forward substitution of the
 * right-hand sides run as two overlapped sweeps, the substitution one panel group behind the factorisation, so that each
 * fills the other's idle stretches (panel chain, under-filled in-group launches, launch drains).  Same results to rounding,
 * same *info and error behaviour as ck_factor; *info != 0 leaves pred / pred_err untouched.  Beyond 128 panels (N > 65 536),
 * where the overlap no longer pays, the call runs the two sweeps one after the other (option "fused_sweeps": -1 this rule,
 * 0 never overlapped, 1 always).  The factor stays resident:
 * further ck_predict calls work as after ck_factor. */
int ck_factor_predict(ck_handle* h, int i, const double* pcoords_host, int64_t m, double* pred_host, double* pred_err_host,
                      int64_t* info);

/* _verify_model (src/joint_prediction.py:60-66, 260-274): is the stacked matrix [[C_pp, c0^T], [c0, Sigma]] of the
 * prediction sites of the LAST ck_predict positive definite?  Sigma is (ck_factor succeeded), so this is the
 * Cholesky of the m x m Schur complement C_pp - V^T V on the solved right-hand sides that ck_predict left on the
 * device (the reference factorises the (m + N) x (m + N) matrix).  info = 0: positive definite; > 0: LAPACK-style
 * index of the failing leading minor among the prediction sites -- the reference then warns
 * "Prediction joint covariance matrix is not positive definte".  The index counts the sites in the order the library
 * laid them out (for m >= 256 with option site_order = 1 that is a Hilbert-curve order, not the caller's): use it as
 * a verdict (zero / non-zero), as the reference does.  Only valid directly after the ck_predict whose sites are meant:
 * ck_set_model, ck_set_metric, ck_assemble_joint and ck_factor invalidate the solved right-hand sides and this call then
 * fails.  Consumes the data row of the right-hand sides (a second call gives the same verdict; ck_aux_finish must
 * not be repeated after it).  Needs m (m + 512) / 2 more doubles of device memory. */
int ck_verify_model(ck_handle* h, int64_t* info);

/* Block (areal) cokriging of process i on the resident factor (needs ck_factor; single-process form).
 * block[a] in [0, r) names the block of site a, every block non-empty; weight[a] finite.
 * pred / pred_err: r values; cov: r x r row-major A S A^T, or NULL to skip it.
 * A is the r x m matrix A[b, a] = weight[a] for the sites a of block b, S = C_pp - c0^T Sigma^-1 c0 the posterior covariance
 * of the point predictions (nugget where h == 0, as ck_predict / ck_verify_model):  pred_b = sum_a w_a pred_a,
 * pred_err_b = nan_to_num(sqrt((A S A^T)_bb)).  A block of one site with weight 1 is that site's ck_predict.
 * The point right-hand sides (K2) are folded into r block rows, so the forward sweep runs over r + 1 rows instead of m + 1;
 * the sites are assembled in chunks of option "block_chunk" sites (0, default: from the device memory the handle may use)
 * and every block's members are summed in the caller's order whatever the chunking: repeated calls give the same bits.
 * cov is refused for r > 65 536 blocks.  The prior covariance of the blocks costs sum_b n_b^2 exact covariance
 * evaluations (with cov: m^2 / 2 + O(m)), spread over the chip in pieces of 512 pairs whatever the block sizes.
 * Needs (roundup(r + 1, 256) N + O(m)) doubles of device memory besides the point rows of one chunk, and with cov the
 * r (r + 512) / 2 doubles of ck_verify_model's Schur buffers plus r (r + 1) / 2 piece offsets (8 bytes each, on the host
 * and the device).  Afterwards -- also after a call that failed once it had started -- ck_verify_model and ck_aux_finish
 * fail until the next ck_predict / ck_aux_begin (the rows are block sums).  ck_timings [16 ..] describe the call (slots 0 .. 15 are left as they were). */
int ck_predict_blocks(ck_handle* h, int i, const double* pcoords_host, int64_t m, const int32_t* block_host,
                      const double* weight_host, int32_t r, double* pred_host, double* pred_err_host, double* cov_host);

/* Leave-one-out cross-validation of process i at all its data sites from ONE factorisation
 * (Predictor.cross_validation, src/joint_prediction.py:207-257, which re-solves per datum):
 * pred_q = z_q - (Sigma^-1 z)_q / (Sigma^-1)_qq, pred_err_q = sqrt(1 / (Sigma^-1)_qq); n_i values
 * each.  Needs ck_factor.  With ck_set_noise the withheld OBSERVATION is predicted: 1 / (Sigma^-1)_qq contains s d_q. */
int ck_loocv(ck_handle* h, int i, double* pred_host, double* pred_err_host);

/* Leave-group-out cross-validation of process i from ONE factorisation: fold f withholds every datum of EITHER process
 * labelled f -- a track, a spatial block, a random tenth (K-fold), a datum together with its co-located partner -- and the
 * withheld data of process i are predicted from all the rest.  With S the withheld positions, Q = Sigma^-1, alpha = Sigma^-1 z:
 *     E[z_S | z_rest] = z_S - Q_SS^-1 alpha_S,      Cov[z_S | z_rest] = Q_SS^-1
 * (ck_loocv is the case of singleton folds; with ck_set_noise Sigma carries s d on its diagonal, so Q_SS^-1 is the covariance of
 * the withheld OBSERVATIONS and contains their s d_q).  With W = the solved unit right-hand-side rows (row of site a = (L^-1 e_a)^T) and
 * y = L^-1 z:  Q_SS = W_S W_S^T, alpha_S = W_S y -- one sweep of the unit rows, the Gram matrices of the folds' rows, one small
 * dense solve per fold.
 * Inputs: fold_k[a], in the caller's order of ck_set_data of process k, is the fold of datum a; -1: never withheld.
 * fold1_host may be NULL (nothing of the other process is withheld); the array of the predicted process must not be.  With
 * one process the other array is ignored.  Every fold in [0, n_folds) must hold at least one datum of process i.
 * Outputs: pred / pred_err: n_i values in the caller's order, pred_q = z_q - (Q_SS^-1 alpha_S)_q, pred_err_q =
 * nan_to_num(sqrt((Q_SS^-1)_qq)); NaN for a datum labelled -1.  fold_stats: n_folds x 3 row-major, or NULL: [0] the fold's
 * size (both processes counted), [1] log|Q_SS|, [2] alpha_S^T Q_SS^-1 alpha_S -- the joint negative log predictive density of
 * the withheld values is 1/2 (s log 2 pi - [1] + [2]).  info: 0, or 1 + the index of the first fold whose Q_SS failed to factor;
 * that fold's outputs are NaN, the other folds are valid, and the call returns 0.
 * Device path: right-hand sides in ck_loocv's layout (row 0 = z, unit rows in the internal site order) from the first withheld
 * internal position to the last (fold1_host NULL: ck_loocv's rows of process i), swept on the growing prefix of live rows;
 * every fold's lower triangle of Q_SS in ONE launch on the matrix cores, the rows gathered by index (a tile map over the
 * within-fold tiles only, each tile starting at the panel of its first position: sum_f s_f^2 N work); folds of up to 64
 * members solved in LDS, one workgroup each; larger ones batched, 64 columns per step, with the updates on the matrix cores.
 * Every reduction has a fixed order and there are no atomics: repeated calls give the same bits.
 * Single-process form, needs ck_factor.  Refused through ck_last_error, with the amounts and the fold: a label outside
 * [-1, n_folds), an empty fold, a fold of more than CK_FOLD_MAX data, too little device memory ((pmax - pmin + 2 rounded up to
 * 256) rows of Npad doubles, 128 x 128 doubles per tile of small folds and (2 s + 192)^2 doubles per larger fold of s data).
 * Afterwards the handle is as after ck_loocv: the factor stays resident, ck_predict gives the same bits as without the call;
 * ck_verify_model / ck_aux_finish refuse until the next ck_predict / ck_aux_begin.  ck_timings [56 ..] describe the call. */
#define CK_FOLD_MAX 4096
int ck_cv_folds(ck_handle* h, int i, const int32_t* fold0_host, const int32_t* fold1_host, int32_t n_folds, double* pred_host,
                double* pred_err_host, double* fold_stats_host, int64_t* info);

/* Gaussian log-likelihood of the data of every process under the model (zero mean, as simple cokriging), with Sigma assembled
 * exactly as ck_assemble_joint builds it (same metric, table path, nugget rule at h == 0):
 *     l = -1/2 (N log 2 pi + log|Sigma| + z^T Sigma^-1 z),   out3 = (l, log|Sigma|, z^T Sigma^-1 z).
 * want_grad != 0: grad[k] = dl/dtheta_k = 1/2 sum_pq G_pq (dSigma/dtheta_k)_pq, G = alpha alpha^T - Sigma^-1, alpha = Sigma^-1 z,
 * in the flat parameter order sigma_11 sigma_22 nu_11 nu_12 nu_22 len_11 len_12 len_22 nugget_11 nugget_22 rho_12 (11 values;
 * one process: sigma nu len nugget, 4 values).  dSigma comes from the exact Matern evaluator (derivative in len scale closed
 * form, in nu a fourth-order difference of the evaluator at a fixed scaled lag); it is 0 where the correlation is 1, clamped
 * or set to 0.  Reductions in a fixed order, no atomics: repeated calls give the same bits.
 * Input: a handle after ck_assemble_joint; the call factors Sigma itself (or uses the factor of a preceding ck_factor).
 * info = 0, or -- Sigma not positive definite -- the 1-based leading minor as ck_factor reports it; out3 / grad are then NaN
 * and the handle needs ck_assemble_joint again.  Single-process form (a partitioned handle is refused).  The gradient needs
 * (N + 1) rows of Npad doubles (roundup(Npad + 1, 256) x Npad for the unit right-hand sides of all data sites) and the lower
 * triangle of G (the packed panels of ck_verify_model's Schur buffers) on the device; the call refuses, stating the amount,
 * when they do not fit.  Costs N^3 / 3 flop for the unit-row sweep and N^3 / 3 for G on top of the factorisation.
 * Afterwards the factor stays resident (ck_predict gives the same bits as without the call); ck_verify_model and ck_aux_finish
 * fail until the next ck_predict / ck_aux_begin.  ck_timings [24 ..] describe the call. */
int ck_loglik(ck_handle* h, int want_grad, double* out3, double* grad, int64_t* info);

/* ---- universal cokriging: an unknown trend estimated by GLS jointly with the kriging ------------------------------
 * Regressors of process k at its data sites: F_k (n_k x p_k).  X (N x p, p = p_0 + p_1) is block diagonal: the rows of process
 * k carry F_k in the columns of block k (process 0's columns first) and zeros elsewhere; z the data, Sigma = L L^T.
 *   y = L^-1 z,  U = L^-1 X,  V_s = L^-1 c0_s,  A = U^T U = X^T Sigma^-1 X,  b = U^T y,  beta = A^-1 b,  Cov(beta) = A^-1,
 *   x0_s = the regressors of process i at site s in the columns of block i (zeros elsewhere),  r_s = x0_s - U^T V_s,
 *   pred_s = V_s . y + r_s^T beta,   pred_err_s = nan_to_num(sqrt(sigma_i^2 + nugget_i - |V_s|^2 + r_s^T A^-1 r_s)).
 * This is the bordered (Lagrange) universal-kriging system [[Sigma, X], [X^T, 0]] (Cressie 1993, section 3.4.5); one constant
 * column per process is ordinary cokriging (the weights on process i sum to 1, those on the other process to 0).
 *
 * ck_set_trend: F (n_k x p_k, row-major) in the caller's order of ck_set_data of process k; p_k = 0 clears the trend of
 * process k, and so does ck_set_data of process k.  Refused: p_k > CK_TREND_PMAX, n_k != that process's data count, n_k < p_k,
 * a non-finite entry.  The library keeps F on the host and lays it out along its site order whenever the sites are laid out
 * (also again: ck_factor's retry in the caller's order, option "site_order", ck_set_metric); a new trend needs no new
 * factorisation. */
#define CK_TREND_PMAX 8
int ck_set_trend(ck_handle* h, int k, const double* F_host, int64_t n_k, int p_k);
/* Universal cokriging of process i at pcoords (m x 2) on the resident factor (needs ck_factor; single-process form).
 * f0: m x p_i regressors of process i at the prediction sites (the caller's order; NULL when p_i = 0), finite.  pred / pred_err:
 * m values in the caller's order; beta: p values, beta_cov: p x p (either may be NULL).  The right-hand sides are ck_predict's
 * with the p rows X^T behind the data row (roundup(m + 1 + p, 256) rows of Npad doubles); one pass (k_reduce_univ) dots every
 * solved row with [y; U] in a fixed order: repeated calls and any chunking of the sites give the same bits.  A is factored on
 * the host with a relative pivot threshold of 1e-10: a rank-deficient design (a repeated column, a constant column twice for
 * one process, fewer distinct sites than regressors) is refused with a message naming the process and the regressor.
 * With no trend set (p = 0) the call is ck_predict (the same bits; beta / beta_cov untouched).  Afterwards the factor stays
 * resident (ck_predict gives the same bits as without the call); ck_verify_model and ck_aux_finish fail until the next
 * ck_predict / ck_aux_begin (the simple-kriging verdict does not apply).  ck_timings [40 ..] describe the call. */
int ck_predict_universal(ck_handle* h, int i, const double* pcoords_host, int64_t m, const double* f0_host, double* pred_host,
                         double* pred_err_host, double* beta_host, double* beta_cov_host);
/* Restricted (REML) log-likelihood for the trend of ck_set_trend:
 *     l_R = -1/2 [(N - p) log 2 pi + log|Sigma| + log|X^T Sigma^-1 X| + z^T P z],  P = Sigma^-1 - Sigma^-1 X A^-1 X^T Sigma^-1,
 *     out4 = (l_R, log|Sigma|, log|X^T Sigma^-1 X|, z^T P z).
 * Convention: no log|X^T X| term (it does not depend on the parameters).  want_grad: grad[k] = 1/2 sum_pq (G_R)_pq
 * (dSigma/dtheta_k)_pq with G_R = alpha_R alpha_R^T + C C^T - Sigma^-1, alpha_R = Sigma^-1 (z - X beta), C = Sigma^-1 X R^-T
 * (A = R R^T), in ck_loglik's parameter order.  Inputs, memory (p more right-hand-side rows), refusals, info and the handle's
 * state afterwards as ck_loglik; a rank-deficient design is refused as in ck_predict_universal.  With p = 0 the call is
 * ck_loglik, bit for bit (out4[2] = 0). */
int ck_loglik_reml(ck_handle* h, int want_grad, double* out4, double* grad, int64_t* info);

/* ---- per-observation measurement-error variances ---------------------------------------------------------------------
 * The reference's loaders carry a variance for every datum (xco2_var, sif_var: src/data_utils.py:28-87, "the variance of the
 * measurement error which will be added to the diagonals of the covariance matrix"; Field.variance_estimate, src/fields.py:88;
 * the line that would use it is commented out at src/point_prediction.py:109-110).  With d_a >= 0 the variance of datum a of
 * process k and s_k >= 0 a scale per process:
 *     Sigma_noise = Sigma + diag(s_k(a) d_a)
 * on the TRUE diagonal, by datum index -- not "where h == 0": two data at identical coordinates keep the nugget on their
 * off-diagonal entry and get no measurement error there.  Nothing else changes: c0, the prior variance sigma_i^2 + nugget_i of
 * pred_err and C_pp of the Schur complement are the field's, so the predictors filter the measurement error out.  Everything
 * that works on the factor follows: ck_predict, ck_factor_predict, ck_predict_universal, ck_predict_blocks, ck_verify_model,
 * ck_conditional_draws (a site on a datum with s d > 0 has S_kk > 0 and is not deflated), ck_sample (draws noisy observations),
 * ck_loglik / ck_loglik_reml (their gradients keep formulas and order: dSigma/dtheta does not involve d), and ck_loocv /
 * ck_cv_folds -- these predict the withheld OBSERVATION, so their variance 1 / Q_qq (Q_SS^-1) contains s d_q.  ck_predict_local
 * and ck_predict_local_universal add the neighbour's s d to the diagonal of every local system, in every size class; the cv
 * rule, the NaN rules and the counters are unchanged.
 *
 * ck_set_noise: var (n_k values) in the caller's order of ck_set_data of process k; var == NULL or n_k == 0 clears the noise
 * of process k, and so does ck_set_data of process k.  Allowed after the sites are laid out: the library keeps the vector on
 * the host and lays it along its site order whenever the sites are laid out (also again: ck_factor's retry in the caller's
 * order, option "site_order", ck_set_metric).  Invalidates the assembled Sigma, the factor and the solved right-hand sides, as
 * ck_set_model does (ck_predict_local needs neither).  Refused through ck_last_error, naming the process and the datum: a
 * count other than that process's data count, a negative or non-finite variance, a negative or non-finite scale, a
 * partitioned handle.  A vector of zeros, a scale of 0 and a cleared vector behave bit for bit like a handle that never saw
 * the call (no kernel is then launched or handed the vector). */
int ck_set_noise(ck_handle* h, int k, const double* var_host, int64_t n_k, double scale);
/* out2 = (dl/ds_0, dl/ds_1) of the last ck_loglik / ck_loglik_reml called with want_grad != 0 on this handle:
 *     dl/ds_k = 1/2 sum_{a in k} G_aa d_a,   G (G_R for REML) the matrix those calls contract,
 * reduced over the packed G tiles in a fixed order (no atomics: repeated calls give the same bits) inside that call.  A process
 * without noise gives 0 (a scale of 0 does not: d is still there).  Refused when no such call has succeeded since the last
 * ck_assemble_joint. */
int ck_loglik_noise_grad(ck_handle* h, double* out2);

/* Expected (Fisher) information of the likelihood at the model's parameters:
 *     I_jk = 1/2 tr(Sigma^-1 D_j Sigma^-1 D_k),   D_k = dSigma / dtheta_k      (reml != 0: P = Sigma^-1 - H A^-1 H^T in place of
 *     Sigma^-1, H = Sigma^-1 X, A = X^T Sigma^-1 X, with the trend of ck_set_trend),
 * exact (no trace estimation) and positive semi-definite.  Slots: the 11 model parameters in ck_loglik's flat order (one process:
 * the first 4), then the measurement-noise scales s_0, s_1 of ck_set_noise (D = diag(d_a) on that process): CK_FISHER_NPAR = 13.
 * A slot is live when the parameter exists (s_k: process k has variances) and free13[slot] != 0 (NULL: all); fisher_host (13 x
 * 13, row-major) is 0 in the rows and columns of the others and symmetric to the bit.  D_k is, entry for entry, the matrix
 * whose contraction with G gives ck_loglik's gradient (the same evaluator, distance and h == 0 test).  Fixed-order reductions,
 * no atomics: repeated calls give the same bits.
 * Preconditions and refusals as ck_loglik (assembled, single-process form).  The call factors if no factor is resident; info
 * != 0 (Sigma not positive definite): fisher_host is NaN and the handle needs ck_assemble_joint again.  On the device it needs
 * what ck_loglik's gradient needs, Sigma^-1 in full (Npad^2 doubles), the derivative operands (about 3.5 Npad^2 doubles for
 * two processes) and their products with Sigma^-1 (about 7 Npad^2); when the products do not fit at once they are formed in
 * groups, and the call refuses, stating the bytes needed and available, when two of them do not fit.  About 7 N^3 flop on the
 * FP64 matrix pipe for two processes of equal size with every parameter live.  Afterwards the factor stays resident (ck_predict
 * gives the same bits as without the call) and the handle is in ck_loglik's state.  ck_timings [64 ..]: derivative assembly,
 * products, contraction, total (ms), the flop of the products, the number of groups. */
#define CK_FISHER_NPAR 13
int ck_loglik_fisher(ck_handle* h, int reml, const int32_t* free13, double* fisher_host, int64_t* info);

/* Vecchia's approximation of the log-likelihood on the local solver: the joint density as a product of conditionals, every
 * datum conditioned on a small set of data that come earlier in a fixed ordering -- a likelihood where Sigma does not fit.
 * The N data of all processes carry distinct integer ranks (rank_host, stacked: process 0 then 1; any distinct integers).  For
 * datum t (process i_t, value z_t, rank rho_t) and process q:
 *   - the candidates C_tq are the sites s of process q with rho_s < rho_t and d(s, t) <= max_dist, d the distance the local
 *     kernels compute on the device.  d = 0 is allowed: a co-located partner of the other process, or an earlier duplicate of
 *     the same process, is a legitimate conditioning datum;
 *   - the cap is the handle's ck_set_local_neighbours(nmax0, nmax1), its rule unchanged: with nmax_q > 0 and |C_tq| > nmax_q,
 *     r_tq = the nmax_q-th smallest d over C_tq and the set is {s in C_tq : d <= r_tq} (ties kept); otherwise all of C_tq.
 *     (0, 0): every earlier datum within max_dist;
 *   - with c(t) the union over q, the local system of ck_predict_local for prediction process i_t at the datum's own
 *     coordinates: Sigma_loc = L L^T (ck_set_noise's s d on its diagonal when noise is on), v = L^-1 c, y = L^-1 z_c;
 *   - mu_t = v . y,  s_t^2 = sigma_i^2 + nugget_i + (s_i d_t if noise is on) - v . v: the variance of the OBSERVATION, raw (not
 *     ck_predict_local's clamped square root).  An empty set gives mu_t = 0 and s_t^2 = the prior observation variance; it is
 *     counted (stats3[0]) and is not an error.
 * out3 = (l, sum_t log s_t^2, sum_t (z_t - mu_t)^2 / s_t^2),  l = -1/2 (N log 2 pi + out3[1] + out3[2]): ck_loglik's three slots
 * on purpose -- when every earlier datum is in every set the three numbers equal the dense ones whatever the ordering
 * (sum_t log s_t^2 = log|Sigma|, and the quadratic forms agree).
 * A datum whose local system is not positive definite, or whose s_t^2 is not > 0, makes out3 NaN and *info = 1 + that datum's
 * index in the caller's stacked order (the first such datum); the call still returns 0 and the per-datum outputs stay valid
 * for every other datum.  *info = 0 otherwise.
 * mean_host, var_host (N, or NULL): mu_t and s_t^2;  count_host (N x 2, or NULL): the set's sizes per process;  stats3 (or NULL):
 * data with an empty set, the largest set, data where a cap bound.  All in the caller's stacked order.
 * The result depends on the ranks, the distances and the caps -- not on option "site_order", on chunking or on the order of
 * ck_set_data, beyond rounding.  Every sum has a fixed order: the N terms are reduced in the caller's stacked order by a fixed
 * tree (256 consecutive terms per workgroup, then the workgroups' sums), no atomics; repeated calls give the same bits.
 * Needs ck_set_model / ck_set_data only, plus ck_set_noise and the caps if wanted.  It never allocates Sigma panels and
 * invalidates nothing: a resident factor, the solved right-hand sides and ck_predict's bits are as before the call.  The ranks
 * are permuted to the internal site order inside the call and kept nowhere.  The data of process i are the points of one pass
 * of the local solver with i_pred = i (select pass, then both size classes as in ck_predict_local), one pass per process.
 * Refused through ck_last_error: a partitioned handle; a trend set on the handle (ck_loglik_vecchia_trend takes one); two equal ranks
 * (both data are named); a non-finite or negative max_dist; NULL rank_host or out3.
 * ck_timings [72 ..]: the select pass, the solves of both size classes, the term reduction, host wall clock (ms), the number of
 * data whose set fits the LDS class (<= 64, the empty ones among them) and the number beyond it; [60 ..] hold the select
 * pass's counters summed over both passes. */
int ck_loglik_vecchia(ck_handle* h, const int64_t* rank_host /* N, stacked: process 0 then 1 */, double max_dist,
                      double* out3, double* mean_host /* N or NULL */, double* var_host /* N or NULL */,
                      int32_t* count_host /* N x 2 or NULL */, int64_t* stats3 /* n_empty, k_max, n_capped */, int64_t* info);

/* The Vecchia likelihood with its analytic gradient, for conditioning sets of at most 64 data (the LDS class of the local
 * solver).  For datum t with set c: w = Sigma_loc^-1 c, alpha = Sigma_loc^-1 z_c, b = (-w, 1) and a = (alpha, 0) over the set plus
 * the datum, e = z_t - mu_t, and
 *   dl/dtheta = 1/2 sum_t sum_pq M_t[p, q] dC_t[p, q]/dtheta,   M_t = (e^2 / s_t^4 - 1 / s_t^2) b b^T + (e / s_t^2) (b a^T + a b^T),
 * C_t the (k + 1) x (k + 1) covariance of the set and the OBSERVATION (ck_set_noise's s d on its diagonal, the datum's own
 * included), its derivatives those of ck_loglik's gradient (exact evaluator, the distance of the exact path).  The sets are held
 * fixed: this is the derivative of the value ck_loglik_vecchia returns for these ranks, max_dist and caps wherever no cap's cut
 * changes with theta -- it never does: the sets depend on the distances alone.  An empty set is the one-entry system b = (1),
 * a = (0), e = z_t: it contributes the derivative of the prior observation variance (slots sigma_i, nugget_i, s_i).
 * out3, stats3, info: as ck_loglik_vecchia; out3 has the bits that call gives on the same handle and inputs.
 * grad13: the slots of ck_loglik_fisher (CK_FISHER_NPAR: the 11 model parameters in ck_loglik's flat order -- one process: the
 * first 4 -- then s_0, s_1).  free13 (or NULL: all): a slot is live when its flag is set and its parameter exists; slots that
 * are not live are exact 0, and masking a slot does not change a bit of the live ones.  When no nu slot of a block is live the
 * four shifted evaluations of its nu difference are skipped.
 * score_host (N x 13 or NULL): the per-datum contributions in the caller's stacked order (the kernel's output before the
 * reduction; asking for them costs their download).  A datum whose local system is not positive definite or whose s_t^2 is not
 * > 0 has NaN in its live slots; then *info names the first such datum, grad13 is NaN and every other datum's score is valid.
 * The N scores are summed column by column by the fixed tree of the terms; no atomics; repeated calls give the same bits.
 * State: as ck_loglik_vecchia -- no Sigma panels, nothing invalidated.
 * Refused through ck_last_error: what ck_loglik_vecchia refuses, NULL grad13, and -- after the select passes of both processes,
 * before any solve -- any conditioning set of more than 64 data (the message names how many data have one and the largest
 * set): the tiled path of larger systems has no back substitution.  Use the caps, or difference ck_loglik_vecchia.
 * ck_timings [80 ..]: the select passes, solve + back substitution + contraction (k_vecchia_grad), the reductions (terms and
 * scores), host wall clock (ms), the data solved and the pairs contracted; [72 ..] hold what ck_loglik_vecchia would report. */
int ck_loglik_vecchia_grad(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13 /* or NULL: all */,
                           double* out3, double* grad13, double* score_host /* N x 13 or NULL */,
                           int64_t* stats3 /* n_empty, k_max, n_capped */, int64_t* info);

/* The expected information of the Vecchia likelihood, for conditioning sets of at most 64 data: the uncertainty that goes with a
 * Vecchia fit.  The Vecchia value is sum_t [log p(z_S) - log p(z_c)], c = c(t) the set of datum t and S = c + {t}; every term is a
 * Gaussian marginal of the exact model, so the expected negative Hessian of the value under the model is
 *     I^V = sum_t [I(S_t) - I(c_t)],   I(A)_jk = 1/2 tr(C_A^-1 D_j,A C_A^-1 D_k,A),   D_j = dC_t / dtheta_j,
 * C_t the (k + 1) x (k + 1) covariance of the set and the OBSERVATION (ck_set_noise's s d on its diagonal, the datum's own
 * included).  This is the expected information of the Vecchia OBJECTIVE under the exact model -- what GpGp reports with its
 * fits -- and not a Godambe sandwich: that needs the covariances of the scores across data (score_host of
 * ck_loglik_vecchia_grad serves an empirical version).  The datum is the last row of S_t, so the difference collapses onto the
 * last row of L_t^-1 D_j L_t^-T: with Sigma_loc = L L^T, w = Sigma_loc^-1 c, b = (-w, 1) and s_t^2 of ck_loglik_vecchia,
 *     g_j = (D_j b)[c],   q_j = b^T D_j b (= ds_t^2 / dtheta_j),   y_j = L^-1 g_j,
 *     I_t[j, k] = (y_j . y_k) / s_t^2 + 1/2 q_j q_k / s_t^4;     an empty set: 1/2 q_j q_k / s_t^4, q_j the derivative of the
 * prior observation variance.  Every I_t is a Gram matrix plus a rank-one term, so the sum is positive semi-definite; when every
 * earlier datum is in every set it telescopes to ck_loglik_fisher's matrix, whatever the ordering.  D_j is, entry for entry,
 * the matrix whose contraction gives ck_loglik_vecchia_grad's gradient (the same pair rule: evaluator, distance, h == 0 test).
 * The result does not depend on the values of the data.
 * fisher_host (13 x 13, row-major): the slots, free13 and the rule for slots that are not live are ck_loglik_fisher's: rows and
 * columns of slots that are not live are exact 0, the matrix is symmetric to the bit, masking a slot changes no bit of the
 * others, and when no nu slot of a block is live the four shifted evaluations of its nu difference are skipped.
 * The sets are those of ck_loglik_vecchia for the same ranks, max_dist and caps; stats3 as there.  A datum whose local system is
 * not positive definite or whose s_t^2 is not > 0 has no term: the live block of fisher_host is NaN, *info = 1 + the first such
 * datum in the caller's stacked order, and the call returns 0.  *info = 0 otherwise.
 * Sums: a workgroup adds the terms of 8 consecutive data of a process in their order (a constant of the layout, not of the
 * device), the workgroups' 91 sums (the lower triangle) are added by the fixed tree of the scores; no atomics; repeated calls
 * give the same bits.  No N x 91 array exists.
 * State: as ck_loglik_vecchia -- no Sigma panels, nothing invalidated, ck_predict's bits unchanged.
 * Refused through ck_last_error: what ck_loglik_vecchia_grad refuses (NULL rank_host or fisher_host here), and -- after the
 * select passes of both processes, before any solve -- any conditioning set of more than 64 data, with that call's message.
 * ck_timings [88 ..]: the select passes, k_vecchia_info (both processes), the reductions, host wall clock (ms), the data solved
 * and the entries evaluated (sum over the data of (k + 1)^2); [72 ..] and [60 ..] as after ck_loglik_vecchia (no terms: [74] is 0). */
int ck_loglik_vecchia_fisher(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13 /* or NULL: all */,
                             double* fisher_host /* 13 x 13 */, int64_t* stats3 /* n_empty, k_max, n_capped */, int64_t* info);

/* The Vecchia likelihood with an unknown trend X beta estimated by GLS inside it: the profile likelihood and its restricted
 * (REML) form, for conditioning sets of at most 64 data (the LDS class of the local solver).  X is ck_set_trend's block-diagonal
 * N x p design, p = p_0 + p_1 <= 16, x_t its row at datum t.  For datum t with set c and Sigma_loc = L L^T as in
 * ck_loglik_vecchia (ck_set_noise's s d on the diagonal):
 *   v = L^-1 c,  y = L^-1 z_c,  U = L^-1 X_c,     s_t^2 = prior + own - v . v  (unchanged),
 *   e_t = z_t - v . y,  f_t = x_t - U^T v,        r_t = (e_t, f_t) / s_t       (an empty set: r_t = (z_t, x_t) / s_t),
 *   G = sum_t r_t r_t^T = [[yy, b^T], [b, A]],    beta = A^-1 b,  Cov(beta) = A^-1,  Q = yy - b^T beta,
 *   profile ML:  l_P = -1/2 [N log 2 pi + sum_t log s_t^2 + Q],
 *   REML:        l_R = -1/2 [(N - p) log 2 pi + sum_t log s_t^2 + log|A| + Q]      (ck_loglik_reml's convention: no log|X^T X|).
 * This is the likelihood of the Vecchia model with mean X beta maximised over (profile) or integrated against (REML) beta --
 * what GpGp profiles out of its fits.  When every earlier datum is in every set, A = X^T Sigma^-1 X, b = X^T Sigma^-1 z and
 * sum_t log s_t^2 = log|Sigma| exactly, whatever the ordering: out5 and beta are ck_loglik_reml's and ck_predict_universal's.
 * out5 = (l, sum_t log s_t^2, log|A|, Q, yy);  beta_host (p, or NULL), beta_cov_host (p x p, or NULL).
 * mean_host (N or NULL): mu_t + f_t^T beta, the conditional mean of the observation under the fitted trend;  var_host, count_host,
 * stats3: as ck_loglik_vecchia, var and count bit for bit those of that call on a handle without the trend -- the p trend rows
 * ride along the factorisation behind c and z (k_vecchia_trend) and change no operation on them.
 * Sums: every dot of the solve in a fixed order; G by a fixed tree (256 consecutive data per workgroup, each entry of the lower
 * triangle summed over them in order, then the workgroups' triangles in the partial-sum order of the scores); no atomics;
 * repeated calls give the same bits.  A is factored on the host with ck_predict_universal's relative pivot threshold of 1e-10:
 * a rank-deficient design is refused with a message naming the process and the regressor.
 * A datum whose local system is not positive definite or whose s_t^2 is not > 0 adds nothing to G: out5, beta and beta_cov are
 * NaN and *info = 1 + that datum (the first such) in the caller's stacked order; the call still returns 0.
 * With no trend set (p = 0) the call is ck_loglik_vecchia: its bits in out5[0], [1], [3] and [4], log|A| = 0, larger sets allowed.
 * State: as ck_loglik_vecchia -- no Sigma panels, nothing invalidated.  Refused through ck_last_error: what ck_loglik_vecchia
 * refuses except the trend, NULL rank_host or out5, and -- after the select passes of both processes, before any solve -- any
 * conditioning set of more than 64 data.  ck_loglik_vecchia, ck_loglik_vecchia_grad and ck_loglik_vecchia_fisher keep refusing
 * a handle with a trend.
 * ck_timings [96 ..]: the select passes, k_vecchia_trend (both processes), the terms and the Gram matrix, residual + gradient
 * (0 here), host wall clock (ms), the data solved and p; [72 ..] and [60 ..] as after ck_loglik_vecchia. */
int ck_loglik_vecchia_trend(ck_handle* h, const int64_t* rank_host, double max_dist, int reml,
                            double* out5 /* l, sum log s^2, log|A|, Q, yy */, double* beta_host /* p or NULL */,
                            double* beta_cov_host /* p x p or NULL */, double* mean_host /* N or NULL */,
                            double* var_host /* N or NULL */, int32_t* count_host /* N x 2 or NULL */,
                            int64_t* stats3 /* n_empty, k_max, n_capped */, int64_t* info);
/* The profile form with its analytic gradient: dl_P/dtheta = dl(theta, beta)/dtheta at beta = beta-hat (the envelope theorem:
 * the derivative through beta-hat vanishes at the maximum), which is ck_loglik_vecchia_grad's formula on the residual
 * z - X beta-hat.  The call runs the stages of ck_loglik_vecchia_trend, forms the residual over the sites (k_vecchia_residual)
 * and launches that call's kernel on it: every value it reads, the datum's own included, is the residual.
 * out5, beta_host, beta_cov_host: the bits of ck_loglik_vecchia_trend(reml = 0).  grad13, free13, score_host (the per-datum
 * dl_t/dtheta at beta-hat), stats3, info: the slots, the masking and the rules of ck_loglik_vecchia_grad; with *info != 0 there
 * is no beta-hat and every score is NaN.  The REML form has no analytic gradient (it needs d log|A| / dtheta): difference
 * ck_loglik_vecchia_trend(reml = 1).  With no trend set the call is ck_loglik_vecchia_grad.
 * ck_timings [96 ..] as ck_loglik_vecchia_trend, [99] the residual, k_vecchia_grad and the score sums. */
int ck_loglik_vecchia_trend_grad(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13 /* or NULL: all */,
                                 double* out5, double* beta_host /* p or NULL */, double* beta_cov_host /* p x p or NULL */,
                                 double* grad13, double* score_host /* N x 13 or NULL */,
                                 int64_t* stats3 /* n_empty, k_max, n_capped */, int64_t* info);
/* The per-datum solve of the two calls above, alone: mu_t = v . y, v . v and g_t = U^T v (N x p) in the caller's stacked order,
 * zeros where the set is empty, NaN where the local system is not positive definite; the test surface of k_vecchia_trend. */
int ck_debug_vecchia_trend(ck_handle* h, const int64_t* rank_host, double max_dist, double* mu_host, double* vv_host,
                           double* g_host /* N x p */);

/* Simulation draw z = L eps in the caller's stacked order (process 0 sites, then process 1):
 * sim.BivariateRandomField._simulate (src/sim.py:52-54: cholesky(cmat, lower=True) @ noise).
 * n = number of observations; needs ck_factor. */
int ck_sample(ck_handle* h, const double* noise_host, double* out_host, int64_t n);

/* Conditional simulation of process i at pcoords (m x 2) on the resident factor (needs ck_factor; single-process form):
 * draws[d, k] = pred[k] + (L_S eps_d)[k],  S = C_pp - c0^T Sigma^-1 c0 (the S of ck_verify_model / ck_predict_blocks),
 * L_S the Cholesky of S after deflation.  Outputs in the caller's site order.
 *   1. pred / pred_err (m values each) are those of ck_predict on the same handle, bit for bit (the call runs it).
 *   2. S is built in ck_verify_model's Schur buffers by the same code.
 *   3. Deflation: site k with S_kk <= tol (sigma_i^2 + nugget_i) gets its row and column of S set to zero and S_kk = 1 -- a
 *      site on a datum of process i has S_kk = 0, and for a positive semi-definite S its whole row is then zero, so removing
 *      it is exact: its draws equal pred.  Every other S_kk gets jitter (sigma_i^2 + nugget_i) added.  deflated[k] (m bytes)
 *      is 1 for a deflated site.
 *   4. S is factored by the blocked Cholesky of the point path.  info = 0, or 1 + the caller's index of the site at whose
 *      pivot the factorisation stopped; the call then returns 0 and leaves draws untouched (pred, pred_err, deflated are
 *      valid).  Two sites with identical coordinates that are not deflated give identical rows of S: info names the later
 *      of them (the library's internal order) without factoring.
 *   5. noise (n_draws x m row-major, the caller's order) is used as given; NULL: normals from Philox4x32-10 with key = seed
 *      and counter = (caller's site index k, d / 2, 0, 0), two 53-bit uniforms, FP64 Box-Muller (r cos t for even d,
 *      r sin t for odd d).  Draw d therefore does not depend on n_draws, on the chunking or on the internal site order.
 *      The noise of deflated sites is zeroed.
 *   6. X = E L_S^T on the matrix cores over the lower tiles (m^2 n_draws flop), in chunks of option "draw_chunk" draws
 *      (0, default: from the free device memory); every element sums in a fixed order: the same bits whatever the chunk.
 * Refused (through ck_last_error): a partitioned handle, no factor, m outside 1 .. 65 536, n_draws < 1, tol or jitter
 * negative or NaN, too little device memory (the message states the amount).  Needs m (m + 512) / 2 doubles of Schur
 * buffers (as ck_verify_model) and (roundup(chunk, 128) roundup(m, 512) + 2 chunk m) doubles for a chunk.
 * Afterwards the handle is as after ck_predict of these sites followed by ck_verify_model: the factor of Sigma stays
 * resident, ck_predict gives the same bits as without the call, ck_verify_model the verdict it gives after ck_predict.
 * ck_timings [30 ..] describe the call. */
int ck_conditional_draws(ck_handle* h, int i, const double* pcoords_host, int64_t m, int64_t n_draws, uint64_t seed,
                         const double* noise_host, double tol, double jitter, double* draws_host, double* pred_host,
                         double* pred_err_host, uint8_t* deflated_host, int64_t* info);

/* Joint prediction of BOTH processes on the resident factor (needs ck_factor and a model of two processes; single-process
 * form; simple cokriging -- no trend, no blocks).  pcoords0 (m0 x 2): the sites of process 0; pcoords1 (m1 x 2): those of
 * process 1; either count may be 0.
 *   pred0 / pred_err0 (m0 values) are what ck_predict(h, 0, pcoords0, m0, ..) gives, pred1 / pred_err1 (m1 values) what
 *   ck_predict(h, 1, pcoords1, m1, ..) gives -- from ONE forward sweep over the stacked right-hand sides
 *   [c0(sites of 0)^T; c0(sites of 1)^T; z^T] (a row's result does not depend on its neighbours).
 *   pair_cov[t] (q values, or NULL: none wanted) = S[a_t, m0 + b_t] for the pairs (a_t, b_t) = pairs[2 t], pairs[2 t + 1]
 *   (a: index into pcoords0, b: index into pcoords1), S = C_pp - c0^T Sigma^-1 c0 the posterior covariance of the stacked
 *   sites, C_pp = [[C00, C01], [C01^T, C11]]: the auto blocks carry the nugget where h == 0 (as in ck_predict and
 *   ck_verify_model), the cross block cross_covariance(0, 1, h) carries none, and ck_set_noise's variances enter through
 *   Sigma only.  One value is C01(d(a, b)) - V_a . V_b: an exact covariance evaluation and the dot product of two solved
 *   rows in a fixed order.
 * Internal order of the stacked sites (it fixes the Cholesky order of ck_conditional_draws_pair): the sites of process 0 first,
 * then those of process 1; each set along its own Hilbert curve (ck_hilbert_order of that set) when option "site_order" is on
 * and the set has at least 256 sites, else in the caller's order.  (On the device the process-1 rows start at roundup(m0, 64);
 * the rows between are zeros and take no part in anything.)
 * Refused (through ck_last_error, the message starts with the call's name): no factor, a partitioned handle, a model of
 * one process, a pair index out of range, a null argument that is needed.
 * Afterwards the factor of Sigma stays resident and ck_predict gives its usual bits; the right-hand sides hold the stacked
 * rows, so ck_verify_model and ck_aux_finish fail ("the last call was ck_predict_pair") until the next ck_predict /
 * ck_aux_begin.  ck_timings [134 ..] describe the call (slots 0 .. 15 are left as they were). */
int ck_predict_pair(ck_handle* h, const double* pcoords0_host, int64_t m0, const double* pcoords1_host, int64_t m1,
                    double* pred0_host, double* pred_err0_host, double* pred1_host, double* pred_err1_host,
                    const int64_t* pairs_host /* q x 2 */, int64_t q, double* pair_cov_host /* q, or NULL */);

/* Co-simulation: ck_conditional_draws on the stacked sites of both processes (needs what ck_predict_pair needs).  The
 * caller's STACKED index of a site is k for site k of pcoords0 and m0 + k for site k of pcoords1: draws (n_draws x (m0 + m1)
 * row-major) holds process 0 in its columns [0, m0) and process 1 in [m0, m0 + m1); pred, pred_err, deflated (m0 + m1 each)
 * and noise (n_draws x (m0 + m1), or NULL) are stacked the same way.
 *   1. pred / pred_err are ck_predict_pair's, bit for bit (the call runs its stages).
 *   2. S = C_pp - V^T V of the stacked sites (ck_predict_pair has the definition) in the Schur buffers.
 *   3. Deflation and jitter as in ck_conditional_draws with EACH ROW'S OWN process: a site of process i is deflated when
 *      S_kk <= tol (sigma_i^2 + nugget_i), every other diagonal entry gets jitter (sigma_i^2 + nugget_i).  A site of process 0 on
 *      a datum of process 1 only keeps a positive variance and is not deflated.
 *   4. The factor of S in the internal order given at ck_predict_pair.  info = 0, or 1 + the stacked index of the site at
 *      whose pivot the factorisation stopped.  Two sites OF THE SAME PROCESS with identical coordinates that are not deflated
 *      stop it at the later of them (internal order) without factoring; the two processes at one location are two random
 *      variables -- S is positive definite there for |rho12| < 1 -- and stop nothing.
 *   5. / 6. as ck_conditional_draws; the Philox counter is (stacked index, d / 2, 0, 0).
 * Refused: as ck_predict_pair, and m0 + m1 outside 1 .. 65 536, n_draws < 1, tol or jitter negative or NaN, too little
 * device memory (the message states the bytes).  Afterwards the handle is as after ck_predict_pair.
 * ck_timings [124 .. 133] describe the call, laid out as ck_conditional_draws' [30 .. 39]. */
int ck_conditional_draws_pair(ck_handle* h, const double* pcoords0_host, int64_t m0, const double* pcoords1_host, int64_t m1,
                              int64_t n_draws, uint64_t seed, const double* noise_host, double tol, double jitter,
                              double* draws_host, double* pred_host, double* pred_err_host, uint8_t* deflated_host,
                              int64_t* info);

/* ---- step-wise form (multi-GPU, fused solve) ------------------------------ */
int ck_num_panels(ck_handle* h, int* n_panels, int* panel_width, int64_t* n_padded);
int ck_panel_owner(ck_handle* h, int K, int* owner_rank);
/* Right-hand-side rows for prediction of process i at pcoords (this rank's shard):
 * assembles c0^T rows and the data row z^T (K2). */
int ck_aux_begin(ck_handle* h, int i, const double* pcoords_host, int64_t m);
/* Factor block column K in place (owner only): diagonal blocks, panel solve. */
int ck_panel_factor(ck_handle* h, int K);
/* Device address / size of the packed panel K: the owner's storage, or this rank's
 * receive buffer (the host broadcasts owner -> all between factor and apply). */
int ck_panel_buffer(ck_handle* h, int K, void** dev_ptr, int64_t* nbytes);
/* Apply panel K to the local trailing block columns (CK_APPLY_SIGMA) and/or to the
 * right-hand-side rows (CK_APPLY_AUX). */
int ck_panel_apply(ck_handle* h, int K, int what);
/* The CK_APPLY_SIGMA part restricted to the locally owned block columns J in [J_lo, J_hi] (clipped to
 * K + 1 .. n_panels - 1).  With it the host can run the classical look-ahead: update column K + 1 first,
 * factor it, start its broadcast, and update the remaining columns under the broadcast. */
int ck_panel_apply_sigma(ck_handle* h, int K, int J_lo, int J_hi);
/* Grouped form (world >= 1): the panels K0 .. K0 + np - 1 -- all readable on this rank, in their owner's storage or in a
 * receive slot (remote panel K lands in slot K % recv_slots, option "recv_slots", default 2; at most recv_slots remote
 * panels are alive at a time) -- applied in ONE pass with the contraction dimension 512 np, i.e. a np-th of the
 * read-modify-write traffic of np calls of ck_panel_apply (single process: what ck_factor / ck_predict do for groups of 3).
 *   what & CK_APPLY_SIGMA: the locally owned block columns J of [max(J_lo, K0 + np), J_hi], every n_phase-th of them
 *                          starting with the phase-th (so that the host can split one group update into n_phase pieces
 *                          and start the next panels' steps and exchanges in between);
 *   what & CK_APPLY_AUX:   the update part only (no substitution) of the right-hand-side block columns of the same
 *                          range, piece `phase` of n_phase contiguous pieces.
 * ck_panel_aux_solve(K): the substitution of right-hand-side block column K with the diagonal block of panel K
 * (ck_panel_apply(K, CK_APPLY_AUX) = ck_panel_aux_solve(K) + the update of the block columns beyond K). */
int ck_panel_apply_group(ck_handle* h, int K0, int np, int what, int J_lo, int J_hi, int phase, int n_phase);
int ck_panel_aux_solve(ck_handle* h, int K);
/* pred / pred_err of the local shard after all panels were applied to the aux rows. */
int ck_aux_finish(ck_handle* h, double* pred_host, double* pred_err_host);
/* info flag of the factorisation so far (synchronises). */
int ck_factor_info(ck_handle* h, int64_t* info);

/* ---- local-neighbourhood cokriging: src/point_prediction.py:45-249 ------------------------- */
/* Prediction and standard error of process i at pcoords (m x 2) from the observations within
 * max_dist of each point (cv != 0: observations of process i at distance 0 are withheld,
 * src/point_prediction.py:141-143).  One workgroup per point: radius search, local covariance,
 * Cholesky with c and z as extra rows.  Points with no observation in range, or whose local
 * covariance is not positive definite, get NaN in both outputs (:218-233); their numbers and the
 * largest neighbourhood size are returned for the caller's warnings.  Needs ck_set_model /
 * ck_set_data only. */
int ck_predict_local(ck_handle* h, int i, const double* pcoords_host, int64_t m, double max_dist, int cv,
                     double* pred_host, double* pred_err_host, int64_t* n_empty, int64_t* n_not_pd,
                     int64_t* k_max);
/* The reference builds the local predictor's state once, in its constructor (src/point_prediction.py:24-43: the Sigma blocks
 * the neighbourhoods are gathered from).  Here that state is the scratch slab of the large-neighbourhood paths: nbytes > 0
 * reserves at least that much, 0 the automatic budget of ck_predict_local (a quarter of the free device memory, at most
 * 32 GiB; option "local_slab_mb" if set).  Afterwards no ck_predict_local whose batches fit pays a hipMalloc (tens of GiB
 * right after smaller buffers were freed: up to seconds -- ck_timings [14] shows what a call spent growing the slab). */
int ck_local_reserve(ck_handle* h, int64_t nbytes);
/* A nearest-neighbour cap per process for ck_predict_local / ck_predict_local_universal (gstat's nmax, per variable).  The rule,
 * for prediction point p and process q:
 *   - the candidates C_pq are the sites of process q that pass the radius predicate: d <= max_dist, and with cv != 0 and
 *     q == i also d > 0; d is the distance the local kernels compute on the device;
 *   - with nmax_q > 0 and |C_pq| > nmax_q, r_pq = the nmax_q-th smallest d over C_pq; otherwise r_pq = max_dist;
 *   - the neighbours of p are the candidates with d <= r_pq.
 * Every candidate at exactly the cut distance is kept, so a neighbourhood may hold more than nmax_q sites of process q: the
 * neighbour set is a function of the distances alone -- not of the internal site order (option "site_order"), of chunking or
 * of the order of ck_set_data.  Size classes, batches and k_max follow the final counts; nothing assumes k <= nmax0 + nmax1.
 * Everything behind the neighbour list (its order, the local system, trend rows, noise, the NaN rules and counters) is as
 * without a cap.  The cap is per process because a joint nearest-k list on data of unequal density often holds no datum of
 * the sparser process at all.
 * Handle state: 0 = no cap for that process, the default is (0, 0); a negative value is refused through ck_last_error; with
 * one process nmax1 is ignored.  It invalidates nothing (no Sigma, factor or layout) and, like ck_set_trend, acts on the next
 * local call; a partitioned handle accepts it.  With (0, 0) the local calls take exactly the uncapped path (no further kernel,
 * the same bits).  With a cap set, a select pass (k_local_select, one workgroup per point: an 8-round radix select over the
 * distances' bit patterns, integer histograms in LDS, no floating-point sums -- repeated calls give the same bits) replaces
 * the counting pass and leaves every point its cut distances and the chord of max(r_p0, r_p1), against which the later
 * kernels cull chunks of sites; a cap that binds nowhere (>= the data counts) gives the bits of the uncapped call.
 * ck_timings [60 ..] describe the pass. */
int ck_set_local_neighbours(ck_handle* h, int64_t nmax0, int64_t nmax1);
/* The select pass alone, with the handle's caps: count (m x 2) the final number of neighbours of process 0 / 1 of every point,
 * rcut (m x 2) r_pq, both in the caller's point order.  With (0, 0): the candidate counts and max_dist.  Answers "how far did
 * the cap reach here"; the test surface of the selection kernel.  Sets ck_timings [60 ..]. */
int ck_debug_local_neighbours(ck_handle* h, int i, const double* pcoords_host, int64_t m, double max_dist, int cv,
                              int32_t* count_host /* m x 2 */, double* rcut_host /* m x 2 */);
/* Universal cokriging in the moving neighbourhood: ck_predict_local with the trend of ck_set_trend estimated by GLS in every
 * neighbourhood (one constant column per process: ordinary cokriging in a moving window).  The formulation is that of
 * ck_predict_universal applied to one point's k neighbours, Sigma_loc = L L^T, c and z as in ck_predict_local:
 *   X_loc (k x p, p = p_0 + p_1 <= 2 CK_TREND_PMAX): the columns of process q carry F_q at that process's neighbours,
 *   v = L^-1 c,  y = L^-1 z,  U = L^-1 X_loc,  A = U^T U,  b = U^T y,  r = x0 - U^T v,  beta = A^-1 b,
 *   pred = v . y + r^T beta,  pred_err = nan_to_num(sqrt(sigma_i^2 + nugget_i - v . v + r^T A^-1 r)), clamped at 0,
 * x0 = the regressors of process i at the point in the columns of block i, zeros elsewhere.  The p trend rows ride along the
 * local factorisation as c and z do; every sum has a fixed order (no atomics): repeated calls give the same bits.
 * f0: m x p_i regressors of process i at pcoords (NULL when p_i = 0).  beta (m x p, or NULL): every point's local GLS
 * coefficients, NaN in dropped columns (rule 3) and in the whole row where the prediction is NaN.
 * Degenerate cases, per point:
 *   1. empty neighbourhood: NaN, counted in n_empty;
 *   2. local Sigma not positive definite: NaN, counted in n_not_pd;
 *   3. a process with regressors but no neighbour in range has identically zero columns of X_loc.  If it is not process i its
 *      columns are dropped and the result is the universal prediction from the remaining columns; if it is process i
 *      (p_i > 0) the unbiasedness constraint cannot be met: NaN, counted in n_rank_def;
 *   4. A is then factored with the relative pivot threshold of the joint path (1e-10): a rank-deficient design (fewer
 *      neighbours of a process than it has regressors, collinear columns) gives NaN, counted in n_rank_def -- it never fails
 *      the call, being a property of single points;
 *   5. a non-finite regressor in a row of f0: both outputs NaN, the point is in none of the three counters;
 *   6. no trend set (p = 0): the call is ck_predict_local, bit for bit (n_rank_def = 0, beta untouched).
 * Needs ck_set_model / ck_set_data / ck_set_trend only (no Sigma panels).  Refused through ck_last_error: a partitioned
 * handle, f0 == NULL with p_i > 0.  Neighbourhoods of up to 64 sites are solved in LDS ((64 + 2 + p) x 64 doubles), larger
 * ones on the tiled path with roundup(k + 2 + p, 64) rows; the scratch slab (ck_local_reserve) is shared with ck_predict_local
 * and batches are sized with the p extra rows.  ck_timings [48 ..] describe the call. */
int ck_predict_local_universal(ck_handle* h, int i, const double* pcoords_host, int64_t m, const double* f0_host,
                               double max_dist, int cv, double* pred_host, double* pred_err_host, double* beta_host,
                               int64_t* n_empty, int64_t* n_not_pd, int64_t* n_rank_def, int64_t* k_max);
/* Block cokriging in the moving neighbourhood (gstat's block= with nmax / maxdist): the weighted mean of process i over the
 * member sites of each of r blocks, with the standard error of that mean, from the observations around the block -- no Sigma.
 * Block b: members x_a with weights w_a (block[a] == b; pcoords m x 2, weight m; weights need not sum to 1 and may be
 * negative) and a search centre c_b (centres r x 2).  The neighbourhood of the block is that of the POINT c_b, by the rules
 * of ck_predict_local with cv = 0: the radius max_dist, the caps of ck_set_local_neighbours with ties kept, the internal site
 * order of the neighbour list.  It is not the union of the members' neighbourhoods, and there is no cross-validation of
 * blocks.  With the k neighbours s_g and Sigma_loc = L L^T exactly as in ck_predict_local (ck_set_noise on its diagonal):
 *   cbar_g   = sum_a w_a C_{i, proc(g)}(x_a, s_g), every term the c entry of ck_predict_local for the point x_a (the nugget
 *              of process i where h = 0), summed in the caller's member order;
 *   sigma_BB = sum_{a, a'} w_a w_a' C_ii(x_a, x_a') with the nugget where h = 0 (the prior term of ck_predict_blocks);
 *   no trend:  v = L^-1 cbar, y = L^-1 z, pred = v . y, pred_err = nan_to_num(sqrt(sigma_BB - v . v)), clamped at 0;
 *   a trend (ck_set_trend): the formulas of ck_predict_local_universal with c -> cbar, sigma_i^2 + nugget_i -> sigma_BB and
 *              x0 -> f0[b] = sum_a w_a f_i(x_a), supplied by the caller (r x p_i; NULL when p_i = 0); beta (r x p, or NULL)
 *              as there.  The degenerate-case rules 1 to 5 of ck_predict_local_universal hold with "point" read as "block":
 *              an empty neighbourhood of the centre (n_empty), a local Sigma that is not positive definite (n_not_pd), a
 *              design that cannot be met (n_rank_def), a non-finite row of f0 (NaN, in no counter).
 * No covariance BETWEEN blocks is offered: different blocks have different neighbourhoods, so such a matrix would be no
 * posterior covariance of anything (ck_predict_blocks on a factored Sigma gives one).
 * Identity: with r = m, block[a] = a, weight 1 and centres = pcoords the outputs are those of ck_predict_local_universal
 * (cv = 0) bit for bit wherever both calls solve a neighbourhood in the same size class -- always with a trend set and, without
 * one, under the default "local_tile_min" (64) or 0; the block call has no slab kernel.
 * Every sum has a fixed order (the members of cbar in slices of consecutive members combined in ascending order, sigma_BB in
 * pieces of 512 pairs; no atomics): repeated calls give the same bits, whatever the batching and the order in which the
 * caller interleaves the members of different blocks.
 * Needs ck_set_model / ck_set_data; optional ck_set_trend, ck_set_noise, ck_set_local_neighbours.  Refused through
 * ck_last_error, with the offending index and value: a partitioned handle; r < 1 or m outside [1, 2^31); a label outside
 * [0, r); a block without a member; a weight, centre or member coordinate that is not finite; f0 == NULL with p_i > 0.
 * k_max: the largest neighbourhood.  ck_timings [104 ..] describe the call. */
int ck_predict_local_blocks(ck_handle* h, int i, const double* centres_host /* r x 2 */, int32_t r,
                            const double* pcoords_host /* m x 2 member sites */, int64_t m,
                            const int32_t* block_host /* m, in [0, r) */, const double* weight_host /* m */,
                            const double* f0_host /* r x p_i block regressors, NULL when p_i = 0 */, double max_dist,
                            double* pred_host, double* pred_err_host, double* beta_host /* r x p or NULL */,
                            int64_t* n_empty, int64_t* n_not_pd, int64_t* n_rank_def, int64_t* k_max);
/* Both processes at every point from ONE local system: ck_predict_pair's question -- how are the two prediction errors at a
 * site correlated -- for data whose Sigma does not fit.  With cv = 0 the neighbourhood of a point does not depend on the
 * predicted process (neither the radius predicate nor the caps of ck_set_local_neighbours look at it; only the c row and the
 * prior variance do), so both processes share one search, one Sigma_loc and one Cholesky; the second process is one more row
 * riding along the factorisation and the cross-covariance one more dot product of two solved rows.  Per point:
 *   the neighbour list is exactly that of ck_predict_local(cv = 0): the radius, the caps with ties kept, the internal site order;
 *   Sigma_loc = L L^T with ck_set_noise's terms on its diagonal;
 *   c^q = the point's covariances with the neighbours as process q, the c row of ck_predict_local(q) (the nugget where h = 0
 *         and the neighbour's process is q);  v_q = L^-1 c^q,  y = L^-1 z;
 *   pred_q = v_q . y,  pred_err_q = nanmax(sqrt(sigma_q^2 + nugget_q - v_q . v_q), 0);
 *   pred_cov = C_01(0) - v_0 . v_1, C_01(0) the model's cross-covariance at h = 0 from the exact evaluator (no nugget, as in
 *         ck_predict_pair).
 * Because the neighbourhood is shared, (pred_0, pred_1) is the simple-cokriging predictor of both processes from ONE data
 * subset, and [[pred_err_0^2, pred_cov], [pred_cov, pred_err_1^2]] is a genuine conditional covariance: that of the two
 * processes at the point given the data of the neighbourhood (positive semi-definite, |pred_cov| <= pred_err_0 pred_err_1).
 * No covariance between DIFFERENT points is offered: their neighbourhoods differ, so such a matrix would be no posterior
 * covariance of anything -- the argument of ck_predict_local_blocks (ck_predict_pair on a factored Sigma gives one).
 * An empty neighbourhood, or a local Sigma that is not positive definite, gives NaN in all five outputs; each is counted once
 * per point (n_empty, n_not_pd).  pred_cov may be NULL.  There is no cv argument: cross-validation of pairs is not offered.
 * pred_q / pred_err_q carry the bits of ck_predict_local(q, cv = 0) on the same handle: the same steps on the same system, the
 * sums by the same tree.  One exception, in the tiled class only: at k = 62 (mod 64) neighbours the padded height
 * roundup(k + 3, 64) is 64 more than the single call's roundup(k + 2, 64), the rows ride through one more 64-column block, and
 * the last bits may differ (measured: at most 9e-16 absolute on values of order 1).  Every sum has a fixed order (no atomics):
 * repeated calls give the same bits, whatever the batching.
 * Device path: k <= 64 neighbours in LDS (k_local_solve_pair, a (k + 3) x k matrix, 34 304 B: four workgroups per CU as
 * k_local_solve); larger ones on the tiled path with kq = roundup(k + 3, 64) rows -- kq - 3, kq - 2, kq - 1 hold c^0, c^1, z --
 * whatever "local_tile_min" says (no slab kernel, as the block call); batches and the slab budget count the third row.
 * Nothing on the handle is invalidated: a resident factor and the bits of ck_predict / ck_predict_local before and after are
 * unchanged.  Needs ck_set_model / ck_set_data; optional ck_set_noise, ck_set_local_neighbours.  Refused through ck_last_error,
 * with the call's name: a partitioned handle; a model of one process; a trend set on the handle (clear it with ck_set_trend:
 * the GLS cross term is not part of this call); m < 1; a non-finite or negative max_dist; NULL for any pointer but pred_cov.
 * ck_timings [138 ..] describe the call. */
int ck_predict_local_pair(ck_handle* h, const double* pcoords_host, int64_t m, double max_dist, double* pred0, double* pred_err0,
                          double* pred1, double* pred_err1, double* pred_cov /* m, or NULL */, int64_t* n_empty,
                          int64_t* n_not_pd, int64_t* k_max);

/* Leave-group-out and buffer cross-validation in the moving neighbourhood: ck_cv_folds' question for data whose Sigma does not
 * fit -- leave-track-out, spatial blocks, K-fold, a buffer around the withheld datum -- answered by the local predictor.  Every
 * predicted datum of process i is the point of one local prediction from which some sites are WITHHELD; two conditions, both
 * evaluated where the radius predicate d <= max_dist is, with d the distance the local kernels compute on the device:
 *   fold    site g of either process is withheld from datum a when label(g) >= 0 and label(g) == label(a).  fold_k[b], in the
 *           caller's order of ck_set_data of process k, is the label of datum b; -1: never withheld, a neighbour of everything;
 *   buffer  a site of process q with d <= buffer2[q] is withheld (buffer2[q] < 0: off; buffer2 NULL: both off).  The cv flag
 *           of ck_predict_local is the case buffer2[i] = 0, other process off.
 * The cap of ck_set_local_neighbours applies AFTER withholding: per process the nmax_q nearest remaining candidates, ties at
 * the cut kept.  Everything behind the neighbour list is ck_predict_local's and, with a trend set, ck_predict_local_universal's
 * (f0: n_i x p_i regressors of process i at ITS DATA in the caller's order, NULL when p_i = 0): the local system, ck_set_noise
 * on its diagonal, the size classes, the NaN rules and the counters.  A fold that empties a neighbourhood is counted in n_empty
 * and is no error.  There is no limit on a fold's size.
 * The predicted data are those of process i with a label >= 0.  The array of process i may be NULL: then every datum of the
 * process is predicted, which is admitted only with buffer2[i] >= 0 so that no datum ever predicts itself.  The other process's
 * array may be NULL (nothing of it is withheld by label); with one process it is ignored.  Every fold in [0, n_folds) must hold
 * at least one datum of process i; n_folds = 0 is the buffer-only call (every label given must then be -1).
 * Outputs, in the caller's order of process i, NaN for a datum that is never withheld: pred, pred_err (n_i), beta (n_i x p or
 * NULL).  counters4: n_empty, n_not_pd, n_rank_def, k_max.
 * Scores.  Per scored datum e = z - pred and v = pred_err^2 + s_i d_a: the predictive variance of the withheld OBSERVATION --
 * the local predictor filters measurement error out of pred_err, so the datum's own ck_set_noise term is added back, as
 * ck_cv_folds has it inside Q_SS^-1.  A datum whose pred is not finite or whose v is not > 0 is skipped and not counted.
 * fold_stats (n_folds x 6 row-major, or NULL): [0] data withheld, both processes counted; [1] data of process i scored; [2] sum
 * e; [3] sum e^2; [4] sum e^2 / v; [5] sum log v.  score5 (or NULL): columns [1 .. 5] over all predicted data, the folds' sums
 * added in fold order.  The negative log predictive density these give, 1/2 (n log 2 pi + [5] + [4]), is the sum of MARGINAL
 * densities: different data have different neighbourhoods, which define no joint law of a fold (ck_cv_folds reports the joint one).
 * Device path: the labels of both processes are laid out in the internal site order (k_cv_labels); the counting pass, the select
 * pass of a capped call and every solve kernel take the two conditions from the call's one descriptor; a fold's sums come from
 * one workgroup (k_cv_fold_scores: a strided sum per thread, a fixed 256-wide tree).  No atomics in any floating-point sum:
 * repeated calls give the same bits.  Identities: singleton folds on data without coincident sites, and buffer2 = (0, off)
 * without labels on any data, give ck_predict_local(cv = 1) at the data, bit for bit.
 * Nothing on the handle is invalidated: a resident factor and the bits of ck_predict / ck_predict_local before and after are
 * unchanged.  Needs ck_set_model / ck_set_data; optional ck_set_trend, ck_set_noise, ck_set_local_neighbours.
 * Refused through ck_last_error, naming the process, the datum and the value where there is one: a partitioned handle; a label
 * outside [-1, n_folds); a fold without a datum of process i; n_folds < 0; a non-finite buffer; the array of process i NULL with
 * buffer2[i] off; f0 == NULL with p_i > 0; a non-finite or negative max_dist.  ck_timings [118 ..] describe the call. */
int ck_cv_local_folds(ck_handle* h, int i, const int32_t* fold0_host, const int32_t* fold1_host, int32_t n_folds,
                      const double* buffer2 /* per process, < 0 = off; NULL = both off */,
                      const double* f0_host /* n_i x p_i regressors at the data of process i, NULL when p_i = 0 */,
                      double max_dist, double* pred_host, double* pred_err_host, double* beta_host /* n_i x p or NULL */,
                      double* fold_stats_host /* n_folds x 6 or NULL */, double* score5 /* or NULL */,
                      int64_t* counters4 /* n_empty, n_not_pd, n_rank_def, k_max; or NULL */);
/* The select pass of ck_cv_local_folds alone, with the handle's caps: count (n_i x 2) the final number of neighbours of process
 * 0 / 1 of every predicted datum, rcut (n_i x 2) its cut distances, in the caller's order; (0, NaN) rows for a datum that is
 * never withheld.  The test surface of the withholding conditions.  Sets ck_timings [60 ..]. */
int ck_debug_local_cv_neighbours(ck_handle* h, int i, const int32_t* fold0_host, const int32_t* fold1_host, int32_t n_folds,
                                 const double* buffer2, double max_dist, int32_t* count_host /* n_i x 2 */,
                                 double* rcut_host /* n_i x 2 */);

/* Conditional simulation in the moving neighbourhood (gstat's nsim with nmax / maxdist: sequential Gaussian simulation): draws of
 * process i at m sites from the data around each site and the sites drawn before it -- no Sigma, no limit on m but memory.
 * Definition.  The m sites carry distinct integer ranks (rank_host; only their order counts).  Stack the sites behind the data
 * of process i as noise-free pseudo-data: every datum precedes every site, site t precedes site u iff rho_t < rho_u.  The
 * conditioning set of site t is that of ck_loglik_vecchia on this augmented data set: per process q the candidates are the
 * earlier members within max_dist -- for q = i data AND earlier sites together, for q != i data only -- cut by the cap nmax_q
 * of ck_set_local_neighbours with ties kept (the cap counts data and already simulated sites alike, gstat's rule).  A site
 * behaves exactly like a noise-free datum of process i: C(0) = sigma_i^2 + nugget_i.  The local system:
 *   Sigma_loc = L L^T over the set (ck_set_noise's s d on the data's diagonal, nothing on the sites'), c = the covariances with
 *   site t, w = Sigma_loc^-1 c, s_t^2 = sigma_i^2 + nugget_i - c . w (raw), mu_t^data = sum over the DATA of the set of w_a z_a;
 *   Y[d, t] = mu_t^data + sum over the earlier SITES u of the set of w_u Y[d, u] + s_t eps[d, t].
 * An empty set gives Y = sqrt(sigma_i^2 + nugget_i) eps; empty sets are counted (stats4[0]) and are not an error.
 * eps: noise_host (n_draws x m, the caller's site order) when given, else ck_conditional_draws' normals: Philox4x32-10, key =
 * seed, counter = (the caller's site index, d / 2, 0, 0), cos for even d and sin for odd d -- draw d depends on (seed, site, d)
 * only, not on n_draws, on the draw chunking (option "draw_chunk") or on the internal order.
 * When every datum and every earlier site is in every set, Y = pred + L_S eps with L_S the Cholesky factor of the dense posterior
 * covariance taken in rank order: the joint predictor's law.  Otherwise the ensemble mean is not ck_predict_local's pred.
 * draws_host: n_draws x m, the caller's order.  mean_host, var_host (m, or NULL): mu_t^data and s_t^2.  count_host (m x 3, or
 * NULL): data of process 0, data of process 1, earlier sites of the set.  stats4: sites with an empty set, the largest set,
 * sites where a cap bound, the number of levels of the recursion (level(t) = 1 + the largest level among the earlier sites of
 * its set; one launch per level).
 * A site whose local system is not positive definite, or whose s_t^2 is not > 0, makes its every draw NaN, and so those of the
 * sites that condition on it; *info = 1 + the first such site in the caller's order (0: none).  The call still returns 0 and
 * mean / var / count stay valid for the other sites: a singular local system is reported, not repaired (two sites at the same
 * coordinates, or a site on a noise-free datum of process i, are the caller's to set aside).
 * Every sum has a fixed order (the data's share of the mean and the recursion in the order of the set's list, no atomics):
 * repeated calls give the same bits.  Nothing on the handle is invalidated: the search runs on an internal copy of the data
 * with the sites appended, built and released inside the call; a resident factor, the solved right-hand sides and the bits of
 * ck_predict / ck_predict_local are as before.  Needs ck_set_model / ck_set_data; optional ck_set_noise, ck_set_local_neighbours.
 * Two consequences of the internal copy: its buffers (the N + m sites, their tables, the call's temporaries) come from the
 * device allocator, not from an arena given with ck_set_arena; and its covariance tables are built over the bounding box of
 * data AND sites, so for a site without earlier sites in its set mu_t^data and s_t^2 equal ck_predict_local's pred and
 * pred_err^2 to the tables' tolerance (2e-13 relative), not bit for bit.
 * Refused through ck_last_error: a partitioned handle; a trend set on the handle; m < 1 or n_draws < 1; two equal ranks (both
 * sites are named); a non-finite or negative max_dist; NULL pcoords_host, rank_host, draws_host, stats4 or info; after the
 * select pass and before any solve, any conditioning set of more than 64 members (the message names how many sites have one
 * and the largest set); too little device memory, for the weights (1 556 bytes per site) or for a chunk of two draws (the
 * message states the amount needed and the amount free; option "sim_free_bytes" sets the latter).
 * ck_timings [110 ..] describe the call. */
int ck_simulate_local(ck_handle* h, int i, const double* pcoords_host, int64_t m, const int64_t* rank_host /* m, distinct */,
                      double max_dist, int64_t n_draws, uint64_t seed, const double* noise_host /* n_draws x m or NULL */,
                      double* draws_host /* n_draws x m, caller's order */, double* mean_host /* m or NULL: mu_t^data */,
                      double* var_host /* m or NULL: s_t^2 */,
                      int32_t* count_host /* m x 3 or NULL: data of 0, data of 1, earlier sites */,
                      int64_t* stats4 /* n_empty, k_max, n_capped, n_levels */, int64_t* info);
/* The weight kernel of ck_simulate_local alone: per site the set's members as stacked caller indices (data 0 .. N - 1, process 0
 * then 1; a site is N + its caller index), sorted ascending on the host and padded with -1, and the weights w in the same order
 * (0 in the padding; NaN where the local system is not positive definite). */
int ck_debug_simulate_local_weights(ck_handle* h, int i, const double* pcoords_host, int64_t m, const int64_t* rank_host,
                                    double max_dist, int64_t* idx_host /* m x 64 */, double* w_host /* m x 64 */);
/* Sequential Gaussian CO-simulation in the moving neighbourhood: ck_simulate_local with the sites of BOTH processes stacked
 * behind the data, so that every draw is a jointly consistent pair of maps (two ck_simulate_local calls give two independent
 * ensembles).  The stacked index is k for site k of pcoords0 and m0 + k for site k of pcoords1, as in
 * ck_conditional_draws_pair; rank_host, noise_host, draws_host, mean_host, var_host, count_host and *info speak of stacked sites.
 * Definition: ck_simulate_local's, on the augmented set in which the sites of process 0 are appended to process 0's data and
 * those of process 1 to process 1's, as noise-free pseudo-data.  Every datum precedes every site; the sites are ordered by rank
 * ACROSS both processes.  The conditioning set of a stacked site is, per process q, the earlier members within max_dist -- data
 * and earlier sites of process q alike -- cut by the cap nmax_q with ties kept.  A site of process q has C(0) = sigma_q^2 +
 * nugget_q; its covariance with a member is the c entry of ck_predict_local for the site's OWN process (a co-located site of
 * the other process contributes C_01(0), no nugget).  The local system, the recursion, the level rule, the NaN and info rules
 * and stats4 are ck_simulate_local's.  count_host has four columns: data of process 0, data of process 1, earlier sites of
 * process 0, earlier sites of process 1.  Philox counter: (stacked index, d / 2, 0, 0).
 * Two sites of the SAME process at one location are reported through info, as in ck_simulate_local; the two processes at one
 * location are two random variables and stop nothing, provided |rho_12| < 1.
 * Identities: with m1 = 0 the call is ck_simulate_local(0), bit for bit, and with m0 = 0 it is ck_simulate_local(1); when every
 * datum and every earlier stacked site is in every set, Y = pred + L_S eps with L_S the factor of the dense posterior covariance
 * of the stacked sites in rank order -- ck_conditional_draws_pair's law.
 * Device path: one select pass over the stacked sites (with cv = 0 the search does not look at the process), the weights in one
 * launch of k_local_sim_weights per process's sites, then ck_simulate_local's levels, recursion and chunking on the stacked
 * set.  Every sum has a fixed order: repeated calls give the same bits.  Nothing on the handle is invalidated.
 * Refused through ck_last_error, with the call's name: what ck_simulate_local refuses (m read as m0 + m1), and a model of one
 * process; m0 < 0 or m1 < 0; NULL coordinates of a non-empty site set; N + m0 + m1 > 2^31 - 1; any conditioning set of more
 * than 64 members, before any solve.  ck_timings [110 ..] describe the call as they do ck_simulate_local. */
int ck_simulate_local_pair(ck_handle* h, const double* pcoords0_host, int64_t m0, const double* pcoords1_host, int64_t m1,
                           const int64_t* rank_host /* m0 + m1, stacked, distinct */, double max_dist, int64_t n_draws,
                           uint64_t seed, const double* noise_host /* n_draws x (m0 + m1) or NULL */,
                           double* draws_host /* n_draws x (m0 + m1) */, double* mean_host /* m0 + m1 or NULL */,
                           double* var_host /* m0 + m1 or NULL */, int32_t* count_host /* (m0 + m1) x 4 or NULL */,
                           int64_t* stats4 /* n_empty, k_max, n_capped, n_levels */, int64_t* info);
/* ck_debug_simulate_local_weights for the stacked sites of both processes: a site is N + its stacked index. */
int ck_debug_simulate_local_pair_weights(ck_handle* h, const double* pcoords0_host, int64_t m0, const double* pcoords1_host,
                                         int64_t m1, const int64_t* rank_host, double max_dist,
                                         int64_t* idx_host /* (m0 + m1) x 64 */, double* w_host /* (m0 + m1) x 64 */);

/* ---- empirical (cross-)semivariogram / covariogram: src/fields.py:192-232, 378-403 ----- */
/* Fields i and j: coords (n x 2), residuals = values minus their mean (src/fields.py:380).
 * same != 0: marginal variogram, strict upper triangle of the i-i pairs (:195-199; j args ignored);
 * else all n_i * n_j pairs (:200-203).  Uses the handle's metric.  At most 2^28 - 1 points per field. */
int ck_vario_begin(ck_handle* h, const double* coords_i_host, const double* resid_i_host, int64_t n_i,
                   const double* coords_j_host, const double* resid_j_host, int64_t n_j, int same);
/* Pass 1: lo = smallest positive and hi = largest pair distance among pairs with d <= max_dist
 * (src/fields.py:212, 394-395); n_positive = 0 if there is no such pair (lo, hi = NaN). */
int ck_vario_extent(ck_handle* h, double max_dist, double* lo, double* hi, int64_t* n_positive);
/* With ck_set_partition(rank, world), world > 1, both passes visit only this rank's share of the pair
 * tiles (tile t belongs to rank t mod world): the host combines the ranks' results -- MIN of lo / MAX of hi
 * over the ranks that found a pair, SUM of the per-bin sums and counts (distributed.DistributedVariogram). */
/* Pass 2: per-bin sum of cloud values and pair count for bins (e_b, e_b+1], first bin [0, e_1]
 * (pd.cut(include_lowest=True), :214-222); edges[0] must be 0; at most 60 bins.
 * cloud = 0.5 (a - b)^2, or a * b when covariogram != 0 (:378-386). */
int ck_vario_bin(ck_handle* h, double max_dist, const double* edges_host, int n_edges, int covariogram,
                 double* sums_host, int64_t* counts_host);
int ck_vario_end(ck_handle* h);
/* Counters of the last ck_vario_extent / ck_vario_bin: [0] pairs of the extent pass decided on the host,
 * [1] pairs of the binning pass decided on the host, [2] pairs the binning pass visited (tiles that cannot hold a
 * retained pair are skipped), [3] extra rounds of the extent pass. */
int ck_vario_stats(ck_handle* h, int64_t* out4, int n);
/* How the variogram passes decide ties.  The reference decides on the rounded distance d (`d <= max_dist`, pd.cut on
 * the edges: src/fields.py:212-216); the kernels compare a monotone function of d and hand every pair within the
 * rounding band of a threshold to the reference's own formula: Euclidean on the device (bit-identical to scipy's
 * cdist), haversine on the host through libm -- bit for bit sklearn's haversine_distances(np.radians(X)) * 6371
 * (src/fields.py:332-336), which device trigonometry is not.  That host function, for n coordinate pairs
 * (A, B: n x 2), no GPU needed: */
int ck_ref_distance(int metric, const double* A_host, const double* B_host, int64_t n, double* out_host);

/* The order in which the library lays n sites out on the device (option site_order = 1, the default, and always
 * for the variogram's points): along a Hilbert curve of order 16 through the sites' bounding box, sites of one cell
 * in the caller's order.  perm_host[k] = index of the site that comes k-th.  Host-only (no handle, no device): the
 * results of every entry point come back in the caller's order, so this is for inspection and tests. */
int ck_hilbert_order(const double* coords_host, int64_t n, int64_t* perm_host);

/* ---- diagnostics ------------------------------------------------------------- */
/* Copy the locally owned part of Sigma / L back as a dense (N x N) lower triangle
 * (upper triangle zero-filled); small N only (tests).  Rows / columns are in the handle's INTERNAL
 * site order: process 0 then process 1, each in the order ck_debug_site_order reports. */
int ck_debug_get_lower(ck_handle* h, double* out_host, int64_t n);
/* Entries (rows[e], cols[e]) of Sigma -- after ck_assemble_joint -- or of its factor L L^T = Sigma -- after ck_factor; then
 * the lower triangle, (r, c) and (c, r) both give L[max][min] -- with the indices in the CALLER's stacked order
 * (process 0 sites, then process 1), whatever the internal site order; any n (parity tests at sizes where the dense
 * matrix does not fit a host array: sampled entries of the table-path assembly, sampled rows of the factor). */
int ck_debug_get_entries(ck_handle* h, const int64_t* rows_host, const int64_t* cols_host, int64_t n, double* out_host);
/* The per-entry Matern derivatives the likelihood gradient, the Fisher information and the Vecchia gradient are made of,
 * evaluated on the device at given lags: out3_host[3 r ..] = (M, dM/dnu, dM/dlen) of block `block` (0: (1,1), 1: (1,2),
 * 2: (2,2); one process: 0) at |lags_host[r]|, M the Matern CORRELATION (no amplitude, no nugget).  The shifted orders and the
 * step of the nu difference are prepared by the code ck_loglik's gradient uses.  After ck_set_model; no data needed. */
int ck_debug_matern_grad(ck_handle* h, int block, const double* lags_host, int64_t n, double* out3_host);
/* perm_out[j] = caller's index (within process k) of the site at internal position j.  Identity
 * with option site_order = 0; a Hilbert-curve order with site_order = 1 (the default). */
int ck_debug_site_order(ck_handle* h, int k, int64_t* perm_out, int64_t n_k);
/* Phase profile of the 64 x 64 diagonal-block kernel (Cholesky + inverse, the latency-bound link of the panel chain):
 * out8[0..5] = microseconds of load | factorisation | scaling + store | inverse of the diagonal 16 x 16 blocks |
 * off-diagonal blocks of the inverse | store of the inverse; [6] / [7] = a whole launch (instrumented / product kernel). */
int ck_debug_potrf_profile(ck_handle* h, int iters, double* out8);
/* Where a link of the cooperative panel step's chain (k_panel_coop) spends its time, on a rows x 512 test panel: out64[8 b + k],
 * b = 1 .. 7 = microseconds (shader clock at 2.4 GHz) from chunk b seeing the pivot chunk's "rows final" flag to k = 1
 * accumulation done | 2 inverse flag seen | 3 rows solved and stored | 4 drained + rows flag set | 5 diagonal block updated |
 * 6 factored + inverse stored | 7 drained + flag set; out64[8 b] (b >= 2) = the period between links; out64[0] = the whole
 * launch (HIP events). */
int ck_debug_coop_profile(ck_handle* h, int64_t rows, double* out64);
/* Raw lane/register -> (row, col) map of v_mfma_f64_16x16x4_f64: out[64*4*3] ints (row, col, k-map check). */
int ck_debug_mfma_probe(ck_handle* h, int32_t* out_host);
/* FP64 MFMA issue-rate microbenchmark (v_mfma_f64_16x16x4_f64, operands in registers,
 * `waves_per_simd` waves on every SIMD of the chip): the measured ceiling the GEMM kernels are
 * compared with, next to the datasheet 78.6 TFLOP/s. */
/* Where the workgroups of a stream created with hipExtStreamCreateWithCUMask(cu_mask8[8]) run (NULL: an
 * unmasked stream): out[wg] = xcc_id << 16 | se_id << 8 | sh_id << 4 | cu_id from HW_REG_XCC_ID / HW_REG_HW_ID. */
int ck_debug_cu_probe(ck_handle* h, const uint32_t* cu_mask8, int n_wg, uint32_t* out_host);
int ck_debug_mfma_peak(ck_handle* h, int waves_per_simd, int iters, double* out3 /* TFLOP/s, shader MHz, cycles per MFMA per wave */);
/* The clock the chip holds under the Cholesky trailing-update kernel on the data of the last ck_factor (the chip lowers
 * its clock under load, by an amount that depends on the operands).  Needs option "gemm_stamps" = 1 (set after the first
 * ck_assemble_joint; the factorisation then runs a stamped instantiation of k_syrk_group_d): out6 = median, 5 % and 95 %
 * quantile of the in-kernel shader clock in MHz over the stamped workgroups, their number, a workgroup's median
 * lifetime in shader cycles and in microseconds. */
int ck_debug_gemm_clock(ck_handle* h, double* out6);
/* Diagnostic: n_side cooperative panel steps (scratch panel of `rows` rows) on the high-priority side stream against the
 * first trailing update of the factorisation on the main stream.  mode 0: the update alone, 1: the side kernels alone,
 * 2: both, released by one event, the first side kernel submitted in front of the update.  out[0] = update ms, out[1 + i] =
 * end of side kernel i after the common start in ms.  Needs an assembled, unfactored handle of >= 8 panels and destroys
 * Sigma (assemble again). */
int ck_debug_stream_overlap(ck_handle* h, int mode, int64_t rows, int n_side, double* out);
/* Host only (no device needed): the 128 x 128 tiles of one Cholesky trailing update -- block columns J0 + u Jstep, u < nJ,
 * of a matrix whose rows / columns from nvalid on are identity padding -- in the order the launch's workgroups take them
 * (csrc/ck_tilemap.h): out3[3 t .. 3 t + 2] = block column, tile row and tile column inside it, for t < min(total, cap).
 * Returns the number of tiles = the launch's grid size, or -1. */
int64_t ck_debug_tile_map(int64_t nvalid, int J0, int Jstep, int nJ, int32_t* out3, int64_t cap);
/* Host only: the same for a launch over the TALL matrix [Sigma; c0^T; z^T] (ck_factor_predict, round 4: one launch updates a
 * block column's triangle tiles and the aux_tile_rows x 4 tiles of the right-hand-side block below it):
 * out4[4 t .. 4 t + 3] = block column, tile row, tile column, 1 if the tile lies in the right-hand-side block (tile row and
 * column then count inside that block).  Returns the grid size, or -1. */
int64_t ck_debug_tall_map(int64_t nvalid, int J0, int nJ, int aux_tile_rows, int32_t* out4, int64_t cap);
/* Host only: the workgroups of a batched launch of the local predictor's tiled path over n_sys systems, largest first, with
 * counts[y] work units each (non-increasing): out2[2 b], out2[2 b + 1] = system (-1: a padding workgroup at the end of a
 * run of equal counts) and unit of workgroup b, for b < min(grid, cap).  Returns the grid size, or -1. */
int64_t ck_debug_run_map(const int32_t* counts, int n_sys, int32_t* out2, int64_t cap);
/* Raw stamps of the last stamped launch ("gemm_stamps" = 1: every launch, = 2 + K0: only the trailing update behind the
 * panel group that starts at K0): out[4 b .. 4 b + 3] = shader cycles and 100 MHz ticks of workgroup b's lifetime (0, 0 if
 * it returned at once), its start in 100 MHz ticks, XCC_ID << 32 | HW_ID; grid4 = grid x, grid y, first block column,
 * number of panels of that launch. */
int ck_debug_gemm_stamps(ck_handle* h, uint64_t* out_host, int64_t n_words, int64_t* grid4);
/* Stage timings of the last calls in milliseconds (HIP events):
 * [0] assemble Sigma, [1] factor, [2] assemble aux, [3] solve sweep, [4] reduce,
 * and, with option "time_gemm": [5]/[6] total ms / number of the Cholesky trailing-update
 * launches (k_syrk_panels) of the last ck_factor, [7]/[8] the same for the right-hand-side
 * trailing updates of the last ck_predict; [9] variogram binning pass (ck_vario_bin); [10] local prediction kernels (ck_predict_local);
 * [11] ck_verify_model (host wall clock, synchronised); [12] 1 if the last ck_factor had to repeat the factorisation because
 * a workgroup of the cooperative panel step (option "panel_fused" bit 4) timed out waiting for a pivot block (never
 * observed; the bit is then off for the handle); [13] after ck_factor_predict: the span of the two overlapped sweeps -- [1] is then the
 * factorisation's span inside it (it shares the chip with the substitution), [3] what the substitution adds behind the
 * factorisation's end, and [5] .. [8] are 0 (a launch's duration would include the other sweep's share of the chip) -- except
 * in the tall sweep (option "tall_sweep", the default): [5]/[6] = sum of the durations / number of its update launches
 * (k_tall_group_d; launches of the two streams overlap each other, so the sum exceeds the span); [10] counts device work only
 * (counting pass + solve), [14] = host milliseconds the last ck_predict_local / ck_local_reserve spent growing the scratch slab
 * (hipMalloc; 0 when it did not grow); [15] after a tall sweep with "time_gemm": the union of the intervals of its update launches
 * -- the time during which k_tall_group_d is running at all (its launches on the two streams overlap each other).
 * ck_predict_blocks (n up to 23): [16] K2 assembly of the point rows, summed over the chunks; [17] the fold into block rows
 * (k_block_fold), summed; [18] the blocks' prior covariance (k_block_prior_part + _sum: diagonal, and the lower triangle with cov);
 * [19] the forward sweep over the r + 1 block rows; [20] reductions, and with cov V^T V (k_schur_syrk_d) and its download;
 * [21] host wall clock of the call; [22] number of chunks.
 * ck_loglik (n up to 30): [24] the assembly of its Sigma (= [0] of that ck_assemble_joint); [25] its factorisation (0 when it
 * used a resident factor); [26] the sweep of the right-hand sides (the data row, with the gradient also the unit rows of all
 * data sites) with the reductions alpha, |y|^2 and log|Sigma|; [27] G = alpha alpha^T - Sigma^-1 (k_ginv_syrk_d);
 * [28] the contraction (k_loglik_grad); [29] host wall clock of the call.
 * ck_conditional_draws (n up to 40): [30] the point prediction (host wall clock of its ck_predict); [31] the assembly of C_pp;
 * [32] V^T V (k_schur_syrk_d); [33] deflation and jitter (k_draw_deflate, k_draw_zero); [34] the factor of S; [35] noise
 * generation (k_draw_noise), summed over the chunks; [36] the draw product and its epilogue (k_draw_trmm), summed over the
 * chunks; [37] host wall clock of the call; [38] number of deflated sites; [39] number of chunks.
 * ck_predict_universal (n up to 48): [40] K2 assembly of its right-hand sides; [41] the forward sweep; [42] the universal
 * reduction (k_reduce_univ); [43] the host GLS step; [44] the host epilogue; [45] host wall clock of the call.
 * ck_predict_local_universal (n up to 54): [48] the counting pass; [49] assembly and factorisation of both size classes (the
 * LDS class's kernel whole, its reduction included); [50] the tiled class's universal reduction (Gram matrix of the solved
 * rows and the GLS step), summed over the batches; [51] host wall clock of the call; [52] / [53] number of points in the LDS
 * class (empty neighbourhoods included) / in the tiled class.
 * ck_cv_folds (n up to 60): [56] the unit rows and their sweep; [57] alpha = W y and the folds' Gram matrices (k_fold_gram);
 * [58] the fold solves of both size classes; [59] host wall clock of the call.
 * The neighbour cap (ck_set_local_neighbours; n up to 64), after a local call or ck_debug_local_neighbours: [60] the select
 * pass (device; it is the counting pass of a capped call and part of [10]); [61] points with at least one capped process;
 * [62] the largest candidate count of a point (both processes together) before the cap; [63] points where a process had more
 * candidates than the LDS lists hold (option "local_select_cap") and re-scanned its chunks every round.  All 0 after an
 * uncapped local call.
 * ck_loglik_vecchia (n up to 78): [72] the select passes of both processes; [73] the solves of both size classes; [74] the
 * terms and their reduction (k_vecchia_terms, k_vecchia_sum); [75] host wall clock of the call; [76] / [77] number of data in
 * the LDS class (empty sets included) / beyond it.  [10], [14] and [60 ..] then hold the sums over its two passes.
 * ck_loglik_vecchia_grad (n up to 86): [80] the select passes of both processes; [81] solve, back substitution and contraction
 * (k_vecchia_grad, both processes); [82] the reductions (the terms' and the scores'); [83] host wall clock of the call; [84] data
 * solved; [85] pairs contracted (sum over the data of (k + 1)(k + 2) / 2).  [72 ..] and [60 ..] are filled as by ck_loglik_vecchia.
 * ck_loglik_vecchia_fisher (n up to 94): [88] the select passes of both processes; [89] k_vecchia_info, both processes; [90] the
 * reductions; [91] host wall clock of the call; [92] data solved; [93] entries evaluated (sum over the data of (k + 1)^2).
 * ck_loglik_vecchia_trend / _trend_grad (n up to 103): [96] the select passes of both processes; [97] k_vecchia_trend, both
 * processes; [98] the terms with their rows and the Gram matrix (k_vecchia_trend_terms, k_vecchia_sum, k_vecchia_trend_gram and
 * its tree); [99] the gradient call's residual, k_vecchia_grad and score sums (0 after the value call); [100] host wall clock of
 * the call; [101] data solved; [102] trend columns p.  [72 ..] and [60 ..] are filled as by ck_loglik_vecchia.
 * ck_predict_local_blocks (n up to 110): [104] the counting or select pass of the centres; [105] the LDS class (search,
 * assembly with cbar, factorisation, outputs); [106] the tiled class; [107] the sigma_BB pass (k_block_prior_part + _sum); [108]
 * host wall clock of the call; [109] member-neighbour covariance evaluations, sum over the blocks of q_b k_b.  [10], [14] and
 * [60 ..] are filled as by ck_predict_local.
 * ck_simulate_local (n up to 118): [110] the select pass of the sites on the augmented set; [111] the weights (k_local_sim_weights);
 * [112] the level planning on the host; [113] the recursion (one launch per level and chunk, and the scatter); [114] host wall
 * clock of the call; [115] sites solved (a non-empty set); [116] levels; [117] sum over the sites of their site-neighbours.
 * ck_cv_local_folds (n up to 124): [118] the counting or select pass of the predicted data; [119] the solves of every size
 * class; [120] the fold scores (k_cv_fold_scores); [121] host wall clock of the call; [122] data predicted; [123] folds.  [10],
 * [14] and [60 ..] are filled as by ck_predict_local.
 * ck_conditional_draws_pair (n up to 134): [124] the joint point prediction (host wall clock of ck_predict_pair's stages);
 * [125] the assembly of C_pp; [126] V^T V; [127] deflation and jitter; [128] the factor of S; [129] noise generation, summed
 * over the chunks; [130] the draw product, summed; [131] host wall clock of the call; [132] number of deflated sites; [133]
 * number of chunks.
 * ck_predict_pair (n up to 138; also set by ck_conditional_draws_pair): [134] K2 assembly of the stacked right-hand sides;
 * [135] the forward sweep; [136] the reductions (k_reduce_pred per process, k_pair_cov); [137] host wall clock of the call.
 * ck_predict_local_pair (n up to 143): [138] the counting pass (a capped call's select pass); [139] the solve window: assembly,
 * factorisation and outputs of both size classes; [140] host: a growth of the scratch slab; [141] points of the tiled class;
 * [142] the batches the tiled class was factored in under the slab budget.
 * [60 ..] are filled as by ck_predict_local.  Like every block, [138 ..] hold until the next call that describes itself in a
 * lower block: such a call zeroes the slots from its own first one upwards (ck_simulate_local and its pair form from [110]). */
int ck_timings(ck_handle* h, double* out, int n);
/* The assembly kernels evaluate the covariance through a per-block table of C = amp * rho over
 * the squared chord (built on the device from the exact K_nu evaluator and verified against it
 * when the data are laid out; error measure |table - C| / (|amp| max(rho, 1e-6)), gate 2e-13).
 * Per block (0 = 11, 1 = 12, 2 = 22): whether the table passed its check (else the assembly uses
 * the exact evaluator), its size / range, its measured error. */
int ck_table_info(ck_handle* h, int block, int* enabled, int* n_intervals, double* q_lo, double* q_hi,
                  double* max_rel_err);
/* Entries the table path deferred to the exact evaluator (pairs closer than the table's lower end
 * or beyond its upper end) in this handle's assemblies since the last reset. */
int ck_table_fallbacks(ck_handle* h, int reset, int64_t* count);
/* Options: "time_gemm" (0/1/2) brackets every trailing-update launch with HIP events (2: the Sigma updates only, for
 * the step-wise form, where Sigma and right-hand-side updates alternate; read back through ck_timings);
 * "exact_cov" (0/1) makes the assembly kernels evaluate K_nu per entry instead of the tables;
 * "recv_slots" (2..64, default 2; before the first assemble / ck_estimate_bytes): receive buffers for remote panels of a
 * multi-process run -- 2 for the per-panel look-ahead schedule, 2 G for the grouped one (ck_panel_apply_group);
 * "lookahead" (-1/0/1, default -1 = automatic) runs the panel step of column K+1 on a second stream under the trailing
 * update of the columns beyond it (per-panel updates); automatic: ck_factor uses it from 12 to 63 panels (where the update is
 * short against the panel step and the one-launch cooperative panel step, submitted in front of the update, really runs
 * beside it: N = 10 000: 12.8 -> 11.4 ms), grouped updates without it from 64 panels on; 1 also switches the solve sweep's
 * variant on;
 * "panel_group" (1..16; default 0 = automatic: 4 for 40 or more panels (3 in rounds 1-3), else 1) = panels per trailing update of
 * ck_factor / ck_predict;
 * "panel_fused" (0..31, default 18 = 2 | 16; bit 0: factorisation, bit 1: right-hand-side rows): inside a 512-column panel the
 * 64-column sub-blocks are processed left-looking with the update and the row solve fused into one launch; bit 2: the
 * 512 x 512 diagonal block first, then one launch for all rows below it; bit 4 (on by default): the WHOLE panel step of the
 * factorisation -- eight 64 x 64 Cholesky factorisations with their inverses, the row solves, the panel-internal updates --
 * in ONE launch of cooperating workgroups: workgroup b owns the 64-row chunk b of the panel and walks it through the
 * sub-blocks as their pivot chunks are published through flags in device memory (agent-scope release / coherent loads,
 * bounded waits), so that a chunk waits for the one chunk above it in the dependency chain instead of for 24 launch
 * boundaries;
 * "coop_spins" (default 2 000 000, ~2 s): polls a workgroup of that launch spends on one flag before it sets the error word and
 * leaves (ck_factor / ck_factor_predict then repeat the factorisation with one launch per dependency and switch bit 4 off:
 * ck_timings [12]); "coop_inject_panel" (default -1; tests): the cooperative step of that panel drops one flag store, once, so
 * that the bounded wait trips and the recovery runs;
 * "tall_sweep" (0/1, default 1): ck_factor_predict as ONE sweep over the tall matrix [Sigma; c0^T; z^T] -- the right-hand-side
 * rows are further workgroups of the cooperative panel step and further tiles of every update launch (k_tall_group_d), with
 * the look-ahead of "fused_la" -- instead of a factorisation and a substitution sweep that share the chip on two streams
 * (same bits either way);
 * "tall_split" (0 never / 1 every panel / 2 automatic, the default) and "tall_split_rows" (default 12 288): in the tall sweep the panel
 * steps of panels behind the first group with at least that many rows run as the cooperative launch on the 512 x 512 head only plus
 * ONE launch of k_panel_rows_all for every other row of the panel and of the right-hand sides -- no workgroup holds a slot while it
 * waits for the head (same bits; N = 40 000: 0.5 % faster);
 * "solve_la" (-1 automatic = from 40 panels, 0, 1): ck_predict's sweep on a resident factor with the chain of the next panel group (the
 * one-column in-group updates, which fill 55 % of the chip, and the rows' walk through each panel) on the high-priority stream UNDER the
 * bulk update of the current group instead of in front of it (N = 40 000: 210 -> 200 ms; same bits);
 * "tall_b2_stream" (0/1, default 1): the tall sweep's update "group g -> everything beyond the next two groups" on the handle's own stream
 * beside the update of the group after next, instead of behind it on one stream (both only wait for group g's panels; 0.2 %);
 * "tall_thin" (0/1, default 1): a last right-hand-side tile row with at most 16 rows in front of the padding (m + 1 = 8 834: two rows)
 * computes those rows' 16-row block only (same bits, 0.35 % at N = 40 000);
 * "assemble_queue" (-1 automatic, 0 off, else the number of workgroups): the table-path assembly kernels as a resident set of
 * workgroups that take their 64 x 512 strips (or halves / quarters of them) from a work queue -- the 48 KB table is loaded once per
 * workgroup instead of once per strip; automatic: the right-hand-side assembly (K2) with 768 workgroups from 8 strips per workgroup
 * on (N = 40 000: 0.62 -> 0.56 ms), Sigma (K1) never (faster on one box, slower on another);
 * "draw_chunk" (default 0 = automatic: half of the free device memory, 128 .. 8192 draws): draws per product launch of
 * ck_conditional_draws;
 * "sim_free_bytes" (default 0 = automatic: what the device reports; tests): the device memory ck_simulate_local counts as free
 * when it admits its weights and its first chunk of draws, and sizes an automatic draw chunk;
 * "fisher_product_mb" (default 0 = automatic: what is free beside everything else the call holds): MiB the stored products of
 * ck_loglik_fisher may take -- less than all of them and they are formed in groups (the same bits);
 * "block_chunk" (default 0 = automatic: what the arena has left, or half of the free device memory, beside the point rows
 * the handle holds): prediction sites per K2 assembly of ck_predict_blocks;
 * "local_slab_mb" = scratch budget of ck_predict_local in MiB (0, default: a quarter of the free memory, at most
 * 32 GiB; the points are processed in batches that fit; the scratch is kept until ck_destroy and reused);
 * "local_tile_min" (default 64 = the LDS kernel's limit): neighbourhoods with more sites than this are factored by
 * the tiled path of ck_predict_local (batched 64-column steps on the matrix cores) instead of one workgroup per
 * point (in LDS up to 64 sites, on a global slab above); ck_predict_local_universal with a trend set has no slab kernel:
 * there every neighbourhood beyond min(local_tile_min, 64) sites takes the tiled path;
 * "local_select_cap" (1..2048, default 2048 = the compiled capacity): candidates per process the select pass of the neighbour
 * cap keeps in LDS; a point with more re-scans its chunks every round (slower, the same result) -- lowered by tests to reach
 * that path at small sizes;
 * "local_group" (1..8, default 4) = 64-column blocks per group of that path; "local_left" (0/1, default 1): a group's columns receive
 * everything from their left in one pass (K = the group's first column) before the group is factored, instead of a K = 64 x
 * local_group update of everything behind every group (same bits: the accumulation order per element is the same);
 * "group_first" (default -1 = automatic: half a group from 40 panels on; 0 = a whole group) / "group_tail" / "group_tail_panels"
 * (default 0 = off): the single-process sweeps' group boundaries -- a first group of so many panels, groups of group_tail panels for
 * the last group_tail_panels panels (the grouping does not change a bit of the results: an element's updates are accumulated k
 * ascending whatever the split; measured, DESIGN.md section 5: groups of four with a first group of two are 0.6 % ahead of groups of three, the tail
 * variants change nothing);
 * "site_order" (0/1, default 1; changing it after the first assemble lays the sites out again): 1 lays the sites of each process -- and
 * sets of >= 256 prediction points -- out along a Hilbert curve inside the library, so that the rows and
 * columns of an assembly tile are neighbours in space (fewer LDS bank conflicts in the table lookups,
 * less divergence in the exact evaluator).  Predictions, LOOCV results and variograms come back in the
 * caller's order either way and agree to rounding (Sigma is permuted symmetrically).  What depends on
 * the order: L itself (ck_debug_get_lower; ck_sample therefore insists on site_order = 0), and the
 * index of the failing leading minor of a Sigma that is not positive definite -- ck_factor repeats such
 * a factorisation in the caller's order to report numpy's index; ck_panel_* callers get the index in
 * factorisation order and can do the same by setting site_order = 0 and sweeping again
 * (distributed.DistributedJoint does). */
int ck_set_option(ck_handle* h, const char* name, int64_t value);
/* Plain C -= A B^T on device buffers through the MFMA kernel (tests / microbenchmarks).
 * A: M x K (lda), B: N x K (ldb), C: M x N (ldc), all row-major device doubles;
 * M % 256 == 0, N % 64 == 0, K % 16 == 0.  lower != 0 skips tiles strictly above the diagonal. */
int ck_dev_gemm_nt(ck_handle* h, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda, const double* B_dev,
                   int64_t ldb, int64_t M, int64_t N, int64_t K, int lower);

#ifdef __cplusplus
}
#endif
#endif /* COKRIGE_H */
