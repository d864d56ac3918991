// ck_host.h -- the host-only part of libcokrige_hip.so: no HIP call, no device pointer.  Error text, the thread team,
// the Hilbert site order (stable radix sort on a few threads), the reference's own distance arithmetic on libm, and
// the variogram's level planning and tie decisions (every pair the kernels leave to the host).  Compiled into the
// product by hipcc as plain C++ and, for tests/test_host_sanitize.py, by g++ with -fsanitize=address,undefined and
// -fsanitize=thread (CPU only).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

// symbols of this file that are not part of include/cokrige.h stay inside the shared object
#define CK_HIDDEN __attribute__((visibility("hidden")))

#define CK_HOST_METRIC_HAVERSINE 0
#define CK_HOST_METRIC_EUCLID 1
#define CK_HOST_VG_MAXBINS 60   // == CK_VG_MAXBINS (ck_internal.h)

CK_HIDDEN int ck_fail(const std::string& msg);   // sets the thread-local error text, returns -1

// fn(thread, begin, end) over [0, n) on a few host threads when n is large
CK_HIDDEN int ck_host_parallel_threads(int64_t n);
template <class F>
static inline void ck_host_parallel(int64_t n, F fn) {
    const int nt = ck_host_parallel_threads(n);
    if (nt == 1) {
        fn(0, (int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([&, t]() { fn(t, n * t / nt, n * (t + 1) / nt); });
    for (auto& x : th) x.join();
}

// perm <- the indices 0..n-1 ordered along the Hilbert curve of order 16 through the box [lo, hi]^2 of the 2-column
// coordinates (stable: coincident sites keep the caller's order)
CK_HIDDEN void ck_host_hilbert_order(const double* xy, int64_t n, const double lo[2], const double hi[2],
                                     std::vector<int64_t>& perm);
// lo / hi are UPDATED (start them at +-1e300)
CK_HIDDEN void ck_host_bounding_box(const double* xy, int64_t n, double lo[2], double hi[2]);

// The reference's own distance arithmetic, on the host with libm -- bit for bit what src/fields.py:332-342 returns
CK_HIDDEN double ck_host_ref_distance(int metric, const double* a, const double* b);

// ---- variogram: thresholds and tie decisions (ck_api.hip: ck_vario_extent / ck_vario_bin) -------------------
// a pair the kernels leave to the host (indices in the order the device sees the points; lev: the level whose
// band the pair lies in, 0 for the candidates of the extent pass)
struct CkVarioPair {
    int i, j, lev, pad;
};
// distance -> the monotone q the kernels compare (ck_vario.hip): squared chord of the unit vectors | squared distance
CK_HIDDEN double ck_host_vario_q_of_dist(int metric, double d);
// rounding band of q around a threshold
CK_HIDDEN double ck_host_vario_band(int metric, double q);
// largest chord |u_i - u_j| of a pair with q <= qlim, with a safety margin
CK_HIDDEN double ck_host_vario_cmax(double qlim);

// Levels 1 .. E in ascending order: the inner edges below the cap, then the cap min(max_dist, last edge); clusters 1 .. EC
// of levels whose rounding bands overlap (one level for the device).  Index 0 of every array is a zero sentinel.
struct CkVarioLevels {
    int E, EC;
    double dthr[CK_HOST_VG_MAXBINS + 2];                                             // per level: the threshold distance
    int cfirst[CK_HOST_VG_MAXBINS + 2], clast[CK_HOST_VG_MAXBINS + 2];               // per cluster: its levels
    double cxa[CK_HOST_VG_MAXBINS + 2], cxb[CK_HOST_VG_MAXBINS + 2], cthr[CK_HOST_VG_MAXBINS + 2];   // per cluster: band, threshold
    double q_reach;                                                                  // largest q still inside the cap's band
};
// 0, or -1 with the error text set (edges too close to zero / below the resolution of the distances)
CK_HIDDEN int ck_host_vario_levels(int metric, double max_dist, const double* edges, int nb, CkVarioLevels* out);

// Extreme distances among candidate pairs, decided by the reference's arithmetic (src/fields.py:212, 394-395):
// *best_lo / *best_hi are UPDATED (start them at +inf / -1)
CK_HIDDEN void ck_host_vario_decide_extent(int metric, const double* ci, const double* cj, const CkVarioPair* cand,
                                           int64_t nc, double max_dist, double* best_lo, double* best_hi);
// The pairs inside the band of a level (cluster) were binned below it by the device; the reference's formula decides
// where they belong: sm[b] / cnt[b] (nb_total + 1 entries) are corrected in place.
CK_HIDDEN void ck_host_vario_fix(int metric, const double* ci, const double* cj, const double* vi, const double* vj,
                                 const CkVarioPair* fix, int64_t nf, const CkVarioLevels& lv, int covariogram,
                                 double* sm, long long* cnt);

// ---- universal cokriging: the p x p GLS step (ck_api.hip: ck_predict_universal / ck_loglik_reml) -------------------
// A = X^T Sigma^-1 X (p x p row-major; the lower triangle is read), b = X^T Sigma^-1 z.  Cholesky A = R R^T with a relative
// pivot threshold: column j is refused when its pivot is not above tol A_jj (a column that is, to rounding, a combination of
// the columns in front of it).  Returns 0, or 1 + the first refused column.  Outputs (any may be null): R (p x p, lower,
// zeros above), beta = A^-1 b, Ainv = A^-1 (p x p, symmetric), logdet = log|A|, bAb = b^T A^-1 b.
CK_HIDDEN int ck_host_gls(int p, const double* A, const double* b, double tol, double* R, double* beta, double* Ainv,
                          double* logdet, double* bAb);

// ---- Fisher information (ck_api.hip: ck_loglik_fisher) -----------------------------------------------------------------
// Parameter slots: the 11 model parameters in the flat order (one process: the first 4), then the noise scales s_0, s_1.
// Operands (ck_internal.h: CK_FOP_*): 0 .. 3 = R, amp dR/dnu, amp dR/dlen, Z of block (0, 0); 4 .. 7 of block (1, 1); 8 .. 10 =
// R, amp dR/dnu, amp dR/dlen of the cross block with its transpose; 11, 12 = diag(d_a) on process 0 / 1.
#define CK_HOST_FISHER_NPAR 13
#define CK_HOST_FISHER_NOPS 13
// C[par NOPS + op]: dSigma/dtheta_par = sum_op C D_op  (D_sigma1 = 2 sigma1 R00 + rho sigma2 (R01 + R01^T), ...)
CK_HIDDEN void ck_host_fisher_coef(int n_procs, double sig1, double sig2, double rho, double* C);
// I = C T C^T over the live slots (T: NOPS x NOPS, the upper triangle is read), rows / columns of the others 0; symmetric to
// the bit (I_kj is written from I_jk)
CK_HIDDEN void ck_host_fisher_combine(const double* C, const double* T, const unsigned char* live, double* I);
// REML: T_ab = 1/2 tr(P D_a P D_b) from the ML value 1/2 tr(Sigma^-1 D_a Sigma^-1 D_b) already in T (nops x nops, both
// triangles written), P = Sigma^-1 - H A^-1 H^T:  T_ab -= 1/2 (tr(A^-1 K_ab) + tr(A^-1 K_ba)) - 1/2 tr(A^-1 G_a A^-1 G_b) with
// K_ab = Y_a^T Sigma^-1 Y_b = K[(a p + i) ldk + b p + j], G_a = Y_a^T H = Gm[(a p + i) p + j], Y_a = D_a H.  A: p x p (lower
// triangle read).  Returns 0, or 1 + the column at which A failed to factor.
CK_HIDDEN int ck_host_fisher_reml(int p, int nops, const double* A, const double* K, int64_t ldk, const double* Gm, double* T);

// ck_loglik_fisher's plan, pure arithmetic: the geometry of the derivative operands, the doubles of their products B_a =
// -Sigma^-1 D_a, and the products cut into groups that fit.  A unit is one launch's operand: the columns of process r
// (c0 rounded DOWN to 128, wpad columns, the live ones in [nlo, nhi)) times the K-panels of process kp (pK0, npan); an operand
// inside a process has one unit, a cross operand two.  op_live[CK_HOST_FISHER_NOPS]: the diagonal operands (11, 12) have no unit
// and no product.  room: the bytes the call may take beside the unit-row sweep (may be negative); fixed_bytes -- Sigma^-1 in
// full, the operands, the thin REML terms of p trend columns, `ngr` workgroups' partial sums, a margin -- comes off it first,
// cap (bytes, 0: none) bounds what is left for the products.  All products fit: one group, region = their doubles.  Otherwise
// two regions of room / 16 doubles each hold a group apiece: the operands in order, a new group where the next product does not
// fit; region = the largest group.  Returns 0, or 1 when two of the largest product (b_max) do not fit: groups is empty, and
// the caller words the refusal from fixed_bytes, d_total and b_max.
#define CK_HOST_NB 512                    // == CK_NB (ck_internal.h)
#define CK_HOST_PANEL_TAIL (8 * 64 * 64)  // == CK_PANEL_TAIL
#define CK_HOST_FOP_R11 4                 // == CK_FOP_R11, CK_FOP_R01, CK_FOP_DIAG0
#define CK_HOST_FOP_R01 8
#define CK_HOST_FOP_DIAG0 11
#define CK_HOST_FISHER_YROWS 256          // == CK_FISHER_YROWS
struct CkFisherUnit0 {
    int op, r, kp;   // operand, process of its columns, process of its K-panels
    int64_t d_doubles;
};
struct CkFisherPlan {
    int64_t c0[2], wpad[2], nlo[2], nhi[2];
    int pK0[2], npan[2];
    std::vector<CkFisherUnit0> units;
    int64_t b_doubles[CK_HOST_FISHER_NOPS];
    int64_t d_total = 0, b_total = 0, b_max = 0, fixed_bytes = 0, region = 0;
    std::vector<std::vector<int>> groups;
};
CK_HIDDEN int ck_host_fisher_plan(int n_procs, int64_t Npad, int64_t n0p, int nK, const bool* op_live, int64_t room, int p,
                                  int64_t ngr, int64_t cap, CkFisherPlan* out);

// ---- the REML gradient's start vectors (ck_api.hip: ck_loglik_reml) ---------------------------------------------------
// W: the reduced rows of the sweep, q + 1 = p + 2 doubles each (|row|^2, row . y, row . U_0 .. U_p-1); row q + r is the unit
// row of internal position r < Npad, so W[q + r] = (., alpha_r, B_r).  av (q x Npad, row-major) <- row 0: alpha_R = alpha -
// B beta; rows 1 .. p: C = R^-1 B^T by forward substitution (A = R R^T, R lower, p x p row-major).  A padding position's row
// goes through the same arithmetic.
CK_HIDDEN void ck_host_reml_start(int p, int64_t Npad, const double* W, int q, const double* beta, const double* R, double* av);

// ---- device memory admission (ck_api.hip: mem_admit) -------------------------------------------------------------------
// bytes of panel K of a packed lower triangle of order Np: its rows with the diagonal blocks' inverses behind them
static inline int64_t ck_host_panel_payload(int64_t Np, int K) {
    return ((Np - (int64_t)K * CK_HOST_NB) * CK_HOST_NB + CK_HOST_PANEL_TAIL) * 8;
}
// the packed triangle of order Mp (a multiple of CK_NB) | with the 8 Mp doubles of site arrays schur_ensure allocates beside it
static inline int64_t ck_host_tri_bytes(int64_t Mp) {
    int64_t b = 0;
    for (int K = 0; (int64_t)K * CK_HOST_NB < Mp; ++K) b += ck_host_panel_payload(Mp, K);
    return b;
}
static inline int64_t ck_host_schur_bytes(int64_t Mp) { return Mp > 0 ? ck_host_tri_bytes(Mp) + 8 * Mp * 8 : 0; }
// One rule for every call that grows the handle's buffers: free memory plus what the call releases first, against what it must
// take.  A buffer that does not grow (right-hand sides and slab: the ask is not above what is held; Schur buffers: the same
// order, or order 0 = not wanted) adds nothing to either side.  Right-hand sides of an arena handle come out of the arena's
// rest and never count against free memory: arena_short says they do not fit there.  extra_bytes: the call's temporaries.
struct CkMemState {
    int64_t free_bytes;
    bool arena;
    int64_t arena_size, arena_used;
    int64_t rhs_bytes, schur_order, slab_bytes;   // held
};
struct CkMemAsk {
    int64_t rhs_bytes, schur_order, slab_bytes, extra_bytes;
};
struct CkMemAdmit {
    int64_t need, avail;
    bool arena_short;
};
CK_HIDDEN CkMemAdmit ck_host_mem_admit(const CkMemState& st, const CkMemAsk& ask);

// ---- tiled local systems: their geometry (ck_internal.h has the layout) and ck_predict_local's plan -----------------------
struct CkLocalSys {
    long long off;      // doubles into the slab
    int k, kq, ld, p;   // neighbours, padded size, leading dimension, prediction point index
};
#define CK_LT_ROWS(kq) ((kq) + 128)
#define CK_LT_NINV 8   // inverses of the diagonal blocks of one column group kept side by side (option local_group <= 8)
// p: trend rows of the universal form, in [kq - 2 - p, kq - 2) between the identity padding and the c / z rows
static inline long long ck_local_tiled_kq(long long k, int p = 0) { return (k + 2 + p + 63) / 64 * 64; }
static inline long long ck_local_tiled_ld(long long kq) { return kq + 128; }
// the padded matrix and the inverses behind it
static inline long long ck_local_tiled_matrix(long long kq) { return CK_LT_ROWS(kq) * ck_local_tiled_ld(kq) + CK_LT_NINV * 64 * 64; }
static inline long long ck_local_tiled_doubles(long long k, int p = 0) {
    return (ck_local_tiled_matrix(ck_local_tiled_kq(k, p)) + (k + 1) / 2 + 1) & ~1LL;
}

// Pure index work between ck_predict_local's counting pass and its first solve launch, in two steps around the device query
// for the budget.  Step (a), from the neighbour counts cnt[0 .. m): need[p], the doubles of point p's scratch slab where
// lds_limit < k <= k_hi (matrix + index list, kept 16-byte aligned; 0 elsewhere); tiled, the points with k > k_hi (k_hi may
// lie below lds_limit: the universal form) sorted by k descending, ties by index -- the systems still active at a column are
// a prefix; need_max, the largest need of a single point of either class (trend: the p trend rows of every tiled system).
struct CkLocalNeeds {
    std::vector<long long> need;
    std::vector<int64_t> tiled;
    int64_t k_max = 0, n_empty = 0;
    long long need_max = 0;
};
CK_HIDDEN void ck_host_local_needs(const int* cnt, int64_t m, int lds_limit, int k_hi, int trend, CkLocalNeeds* out);
// Step (b): both classes cut in order into batches [begin, end) whose needs sum to at most `budget` doubles (a batch holds at
// least one element, whatever it needs); off[p] / sys[t].off: the prefix sums inside a batch; slab_doubles: the largest batch.
struct CkLocalPlan {
    std::vector<long long> off;
    std::vector<std::pair<int64_t, int64_t>> batches, tbatches;   // points | indices into sys (empty without a tiled point)
    std::vector<CkLocalSys> sys;
    long long slab_doubles = 0;
};
CK_HIDDEN void ck_host_local_plan(const int* cnt, const CkLocalNeeds& nd, long long budget, int trend, CkLocalPlan* out);
// ck_predict_local_pair: the c rows of both processes and z ride along every system, three extra rows.  Step (a) for them: two
// classes only -- k <= lds_limit in LDS ((k + 3) x k doubles), everything larger tiled with kq = roundup(k + 3, 64) rows, whatever
// tile_min says (the pair form has no slab kernel; tile_min below lds_limit lowers the LDS class's bound as in the universal
// form).  Step (b) is ck_host_local_plan with trend = CK_LOCAL_PAIR_ROWS - 2: batches and the slab budget count the third row.
#define CK_LOCAL_PAIR_ROWS 3
CK_HIDDEN void ck_host_local_pair_needs(const int* cnt, int64_t m, int lds_limit, int tile_min, CkLocalNeeds* out);

// ---- the dense predictors' host arithmetic (ck_api.hip: ck_predict_universal, ck_predict_blocks, ck_conditional_draws) --------
// The standard error behind a variance: a negative variance gives NaN and then 0.0 (np.nan_to_num; the device's k_reduce_pred
// has the same rule)
static inline double ck_host_err_of(double var) {
    const double e = sqrt(var);
    return e == e ? e : 0.0;
}

// Members of r blocks by stable counting sort: block[a] in [0, r) labels site a < m.
//   off      r + 1 CSR offsets: the members of block b are the grouped positions off[b] .. off[b + 1]
//   member   m: the caller's index of the member at each grouped position, the caller's order kept inside a block
//   q_max    the largest block
// Returns CK_HOST_BLOCKS_OK; CK_HOST_BLOCKS_LABEL with *at = the first site whose label is outside [0, r) (the outputs are not
// usable); or CK_HOST_BLOCKS_EMPTY with *at = the first block without a member -- the outputs are complete, and a caller that
// groups one chunk of a call's sites takes them as they are.  The caller words the refusal.
#define CK_HOST_BLOCKS_OK 0
#define CK_HOST_BLOCKS_LABEL 1
#define CK_HOST_BLOCKS_EMPTY 2
CK_HIDDEN int ck_host_block_members(const int32_t* block, int64_t m, int32_t r, std::vector<int>& off, std::vector<int64_t>& member,
                                    int64_t* q_max, int64_t* at);

// Piece offsets of the blocks' prior (ck_blocks.hip): poff[e] .. poff[e + 1] = the pieces of CK_HOST_PRIOR_PIECE pairs of element
// e (full == 0: e = b, n_b^2 pairs; full != 0: e = R (R + 1) / 2 + C, n_R n_C pairs), n_b = off[b + 1] - off[b].  Returns the
// number of pieces, poff's last entry.
#define CK_HOST_PRIOR_PIECE 512   // == CK_PRIOR_PIECE (ck_internal.h)
CK_HIDDEN int64_t ck_host_prior_pieces(const int* off, int32_t r, int full, std::vector<long long>& poff);

// ck_predict_blocks' sites per pass through the assembly.  option > 0 (block_chunk): that many.  Otherwise what the handle may
// still take beside the held_bytes of point rows it holds: with an arena (arena_rest >= 0, the bytes it has left; it never takes
// memory back) the larger of the two, without one (arena_rest < 0) half of free_bytes plus what is held (the buffer is freed
// before a larger one is allocated); in rows of Npad doubles, less CK_HOST_AUX_ALIGN rows of padding, at least CK_HOST_AUX_ALIGN.
// Never more than m.
#define CK_HOST_AUX_ALIGN 256   // == CK_AUX_ALIGN (ck_internal.h)
CK_HIDDEN int64_t ck_host_block_chunk(int64_t option, int64_t free_bytes, int64_t arena_rest, int64_t held_bytes, int64_t Npad,
                                      int64_t m);
// ck_conditional_draws' draws per pass.  option > 0 (draw_chunk): that many.  Otherwise the multiple of 128 whose noise (Mp
// doubles a draw), draws and, with the caller's noise, its copy (m doubles each) fit half of free_bytes, within [128, 8192].
// Never more than n_draws.
CK_HIDDEN int64_t ck_host_draw_chunk(int64_t option, int64_t free_bytes, int64_t Mp, int64_t m, bool caller_noise, int64_t n_draws);

// Two sites at the same coordinates have identical rows of the posterior covariance: the exact factorisation stops at the later
// of them.  pcoords: m x 2 in the caller's order; cmap[j]: the caller's index of internal position j < m; mask[j] != 0: position
// j is deflated and cannot stop anything.  Returns the smallest internal position that coincides with an earlier one, or -1.
CK_HIDDEN int64_t ck_host_coincident_site(const double* pcoords, const int* cmap, const unsigned char* mask, int64_t m);

// ---- joint prediction of both processes: the stacked layout (ck_api.hip: ck_predict_pair, ck_conditional_draws_pair) --------
// Pure index work, no device.  The m0 sites of process 0 (pc0: m0 x 2) and the m1 sites of process 1 (pc1: m1 x 2) as ONE set of
// right-hand-side rows laid out like Sigma's own sites: process 0 in the rows [0, m0), zero rows up to m0p = roundup(m0, 64),
// process 1 in [m0p, rows), rows = m0p + m1 (the data row's index).  Inside its range each set lies along its own Hilbert curve
// (ck_hilbert_order of that set) when site_order is on and the set has at least CK_HOST_PAIR_SORT_MIN sites, else in the
// caller's order.  The caller's STACKED index of a site: k for site k of process 0, m0 + k for site k of process 1.
//   cmap     rows ints: the stacked index of the site in internal row j, -1 in the gap
//   row_of   m0 + m1: the internal row of every stacked index
//   xy       rows x 2: the coordinates in the internal order, zeros in the gap
#define CK_HOST_PAIR_SORT_MIN 256
struct CkPairPlan {
    int64_t m0 = 0, m1 = 0, m0p = 0, rows = 0;
    bool sorted[2] = {false, false};
    std::vector<int> cmap;
    std::vector<int64_t> row_of;
    std::vector<double> xy;
};
CK_HIDDEN void ck_host_pair_plan(const double* pc0, int64_t m0, const double* pc1, int64_t m1, bool site_order, CkPairPlan* out);
// ck_host_coincident_site inside each process (two processes at one location are two random variables: no stop).  mask: rows
// bytes, != 0 where the row is deflated (the gap rows among them).  Returns the smallest internal row that coincides with an
// earlier row of its own process, or -1.
CK_HIDDEN int64_t ck_host_pair_coincident(const CkPairPlan& P, const double* pc0, const double* pc1, const unsigned char* mask);

// ck_predict_universal's epilogue over the reduced rows W (internal order, p + 2 doubles each: |V_s|^2, V_s . y, U^T V_s):
//   r_s = x0_s - U^T V_s,  pred_s = V_s . y + r_s^T beta,  pred_err_s^2 = c0 - |V_s|^2 + r_s^T A^-1 r_s
// with x0_s = f0[c pi .. c pi + pi) in the columns offi .. offi + pi of the predicted process and zero elsewhere (pi may be 0);
// c = pperm[s], or s where pperm is null: the results land in the caller's order.  beta: p, Ainv: p x p row-major, p <=
// CK_HOST_TREND_QMAX - 1.
#define CK_HOST_TREND_QMAX 17   // == CK_UNIV_QMAX (ck_internal.h)
CK_HIDDEN void ck_host_universal_finish(const double* W, const double* beta, const double* Ainv, const double* f0,
                                        const int64_t* pperm, double c0, int64_t m, int p, int pi, int offi, double* pred,
                                        double* pred_err);

// ---- block cokriging in the neighbourhood: the member layout (ck_api.hip: ck_predict_local_blocks) --------------------------
// Pure index work, no device.  block[a] in [0, r) labels member site a (pcoords: m x 2, weight: m), centres: r x 2.
//   off     r + 1 CSR offsets: the members of block b are the grouped positions off[b] .. off[b + 1]
//   perm    m: the caller's index of the member at each grouped position -- a stable grouping, the caller's order kept inside
//           a block
//   xy, w   the members' coordinate rows (mpad x 2, as the caller gave them) and weights (mpad) in grouped order, zero beyond
//           m; mpad = m rounded up to `pad`.  The device's site transform (the one that prepares the centres and every other
//           point of a local call) turns xy into the two forms the kernels read, the exact-formula rows and the chord vectors:
//           the same arithmetic as for a point, which is what makes a block of one site the point itself to the bit.
//   q_max   the largest block
// The batch plan of the call is ck_host_local_needs / ck_host_local_plan with the r centres as the points.
struct CkLocalBlockLayout {
    std::vector<int> off;
    std::vector<int64_t> perm;
    std::vector<double> xy, w;
    int64_t mpad = 0, q_max = 0;
};
// 0, or -1 with the error text set, the offender named with its index and value: r < 1, m outside [1, 2^31), a label outside
// [0, r), a block without a member, a weight, centre or member coordinate that is not finite
CK_HIDDEN int ck_host_local_block_layout(const double* centres, int32_t r, const double* pcoords, int64_t m, const int32_t* block,
                                         const double* weight, int pad, CkLocalBlockLayout* out);

// ---- the Vecchia likelihood: the ordering's index work (ck_api.hip: ck_loglik_vecchia, ck_loglik_vecchia_grad) --------------
// Pure index work, no device.  rank: N = n[0] + n[1] distinct integers in the caller's stacked order (process 0, then 1); only
// their order counts.  perm_k as in the fold plan below (ck_handle::perm); internal position of the site at position j of
// process k: j for process 0, n0p + j for process 1.
//   pos    N: every datum's position 0 .. N - 1 in the ordering, stacked order.  Ranks that already are a permutation of
//          0 .. N - 1 (what vecchia.ordering_ranks hands over) cost one pass, any others a sort
//   rs     npad: every site's position in the ordering, internal order; padding (between the processes, behind the last) keeps
//          INT32_MAX and is never earlier than a point
//   gself  N: every datum's own internal position, stacked order
struct CkVecchiaOrder {
    std::vector<int> pos, rs, gself;
    int64_t dup[2] = {0, 0};
};
// 0, or -1 with two data of equal rank in out->dup (stacked order, the earlier first; the caller words the refusal)
CK_HIDDEN int ck_host_vecchia_order(const int64_t* rank, int n_procs, const int64_t n[2], int64_t n0p, int64_t npad,
                                    const int64_t* perm0, const int64_t* perm1, CkVecchiaOrder* out);

// ---- leave-group-out cross-validation: the fold layout (ck_api.hip: ck_cv_folds) ---------------------------------------
// Pure index work, no device.  Fold f withholds every datum of either process labelled f (fold_k[a]: the caller's order of
// process k; -1: never withheld; fold1 may be null).  perm_k[j] = caller's index of the site at internal position j of
// process k (ck_handle::perm); internal position of that site: j for process 0, n0p + j for process 1.
//   members     off (n_folds + 1), pos (internal positions, ascending inside a fold), cidx (caller's index within process
//               i, -1 for a datum of the other process)
//   gather list gpos: the internal positions whose unit rows the Gram kernel reads, 128 per tile.  Folds of up to
//               CK_HOST_FOLD_LDS members ("small") are packed several to a tile, sorted by their first position, none across
//               a tile edge; a larger fold ("big") starts its own run of tiles.  Padding entries repeat a position of the
//               same tile (their products are never read).  gbase[f]: where fold f starts in gpos.
//   tiles       one 128 x 128 product each: rows gpos[a0 ..], columns gpos[b0 ..], written at buffer + c_off with leading
//               dimension ld; pos0 = the smallest position among its rows AND columns' later operand, i.e. every panel in
//               front of pos0 / 512 is structurally zero in the product.  Sorted by pos0 (longest contraction first).
//   buffer      [n_small_tiles x 128 x 128 | the big folds' systems].  A big fold of s members is the symmetric system of
//               order kq = roundup(2 s + 1, 64) that the local predictor's batched Cholesky steps factor (ck_la.hip: k_lt_*):
//               rows [0, s) Q_SS, rows s + q the unit rows (they become row q of R^-T), row 2 s alpha_S (becomes R^-1 alpha),
//               ld = kq + 128, kq + 128 rows, then 8 x 64 x 64 doubles for the diagonal blocks' inverses (ck_local_tiled_matrix).  big:
//               largest first.
#define CK_HOST_FOLD_MAX 4096   // == CK_FOLD_MAX (include/cokrige.h)
#define CK_HOST_FOLD_LDS 64     // folds up to this size are solved in LDS
#define CK_HOST_FOLD_TILE 128
struct CkFoldTile {
    long long c_off;
    int a0, b0, ld, pos0;
};
struct CkFoldBig {
    long long off;
    int s, kq, ld, gbase, fold, pad;
};
struct CkFoldSmall {
    int gbase, s, fold, pad;
};
struct CkFoldPlan {
    int64_t pmin = 0, pmax = -1;
    std::vector<int32_t> off, pos, cidx, gbase, gpos;
    std::vector<CkFoldTile> tiles;
    std::vector<CkFoldSmall> small;
    std::vector<CkFoldBig> big;
    int64_t n_small_tiles = 0, buffer_doubles = 0;
};
// 0, or -1 with the error text set: a label outside [-1, n_folds), a fold without a datum of process i, a fold of more than
// fold_max members (the messages state the amounts and name the fold)
CK_HIDDEN int ck_host_fold_plan(int i, int n_procs, const int64_t n[2], int64_t n0p, const int64_t* perm0, const int64_t* perm1,
                                const int32_t* fold0, const int32_t* fold1, int32_t n_folds, int fold_max, CkFoldPlan* out);

// ---- cross-validation in the moving neighbourhood: who is predicted, under which label (ck_api.hip: ck_cv_local_folds) -----
// Pure index work, no device.  fold_k / perm_k / the internal positions as in the fold plan above; either label array may be
// null.  The predicted data are those of process i with a label >= 0, all n_i of them when fold_i is null (admitted only with
// buffer_i, a buffer around the datum of its own process: no datum may predict itself), in the caller's order.
//   plist    m: the caller's index within process i of every predicted datum, ascending
//   fp       m: their labels (-1 throughout when fold_i is null)
//   off/idx  the groups the scores are summed over: group g owns idx[off[g] .. off[g + 1]), positions in plist, ascending.
//            One group per fold; with fold_i null a single group of everything (n_groups = 1, or 0 when n_i = 0)
//   size     n_folds: the data of BOTH processes that carry the label
//   gself    n[0] + n[1]: every datum's own internal position, stacked order (what scatters the labels on the device)
struct CkLocalCvPlan {
    std::vector<int32_t> plist, fp, idx, gself;
    std::vector<long long> off;
    std::vector<int64_t> size;
    int64_t n_groups = 0;
};
// 0, or -1 with the error text set (name: the entry point the text starts with): n_folds < 0, fold_i null without buffer_i, a
// label outside [-1, n_folds) (the message names the process, the datum and the value), a fold without a datum of process i
CK_HIDDEN int ck_host_local_cv_plan(const char* name, int i, int n_procs, const int64_t n[2], int64_t n0p, const int64_t* perm0,
                                    const int64_t* perm1, const int32_t* fold0, const int32_t* fold1, int32_t n_folds, bool buffer_i,
                                    CkLocalCvPlan* out);

// ---- conditional simulation in the moving neighbourhood: the stacked sites of both processes on the augmented set ----------
// Pure index work, no device (ck_api.hip: ck_simulate_local, ck_simulate_local_pair).  The augmented set holds, per process q,
// its n[q] data and behind them its m[q] sites; the STACKED index of site k of process 0 is k, of site k of process 1 m[0] + k
// (ck_conditional_draws_pair's).  rank: m[0] + m[1] distinct integers in stacked order; the sites are ordered by rank across
// both processes, every datum precedes every site.  perm_q / n0p / npad: the augmented set's layout as in ck_host_vecchia_order
// (perm_q[j] = the augmented caller index, within process q, of the site at internal position j).
//   pos   m[0] + m[1]: every stacked site's position in the ordering
//   ext   npad: internal index -> the caller's stacked index, a datum its stacked datum index < N, a site N + its stacked
//         index; -1 in the padding
//   rs    npad: internal index -> precedence, a datum its stacked index, a site N + its position; INT32_MAX in the padding
//   rp    m[0] + m[1]: N + pos, the points' own precedence
// 0, or -1 with two stacked sites of equal rank in out->dup (the earlier first; the caller words the refusal).
struct CkSimSites {
    std::vector<int> pos, ext, rs, rp;
    int64_t dup[2] = {0, 0};
};
CK_HIDDEN int ck_host_sim_order(const int64_t* rank, const int64_t m[2], CkSimSites* out);
CK_HIDDEN void ck_host_sim_ext(int n_procs, const int64_t n[2], const int64_t m[2], int64_t n0p, int64_t npad, const int64_t* perm0,
                               const int64_t* perm1, CkSimSites* out /* pos set */);

// ---- conditional simulation in the moving neighbourhood: the levels of the recursion (ck_api.hip: ck_simulate_local) --------
// Pure index work, no device.  Site t (the caller's index) sits at position pos[t] of the ordering (a permutation of 0 .. m - 1)
// and conditions on ns[t] earlier sites, whose POSITIONS are nbr[t ld .. t ld + ns[t]).  level[t] = 1 + the largest level among
// them, 1 without any: walking the positions upwards meets every neighbour before the site.  A level's sites depend on lower
// levels only, so one launch per level computes them all.
//   level   m: the caller's order
//   order   m: the caller's indices grouped by level, ascending position inside a level
//   off     the level l (1-based) owns order[off[l - 1] .. off[l]); n_levels + 1 entries
struct CkSimLevels {
    std::vector<int32_t> level, order;
    std::vector<int64_t> off;
};
// the number of levels, or -1 when pos is no permutation or a neighbour is not an earlier position (out->off[0], off[1]: the
// caller's index of the site and the offending entry)
CK_HIDDEN int64_t ck_host_sim_levels(int64_t m, int ld, const int32_t* pos, const int32_t* ns, const int32_t* nbr, CkSimLevels* out);
