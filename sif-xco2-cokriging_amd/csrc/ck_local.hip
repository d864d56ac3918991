// ck_local.hip -- local-neighbourhood cokriging: one workgroup per prediction point.
//
// Replaces the per-row Python of point_prediction.Predictor (src/point_prediction.py:127-249):
//   _local_dist_ix   radius search d <= max_dist per process (cross-validation: process i also d > 0, :141-143)
//   _local_values    gather of the precomputed Sigma blocks -> here the k x k local covariance is assembled on the fly
//                    from the k neighbours (no global Sigma is ever stored)
//   _pred_calc       cho_factor / cho_solve, pred = w.z, std = sqrt(c0 - w.c), nanmax([std, 0]) -> one Cholesky of the
//                    local system carrying c and z as two extra rows (forward substitution only)
// Empty neighbourhood -> (NaN, NaN) (:229-233); local Sigma not positive definite -> (NaN, NaN) (:218-222).
//
// Every kernel is told about the call by one CkLocalProblem (ck_internal.h), passed by value.  The steps, each written once:
//   lp_point      what a workgroup loads for its point: exact and chord coordinates, its reach (LpReach: max_dist / cmax, or
//                 the neighbour cap's own cut distances and culling chord), its rank in the Vecchia ordering, the site rows
//   lp_compact    the neighbour list in site order (process 0 sites ascending, then process 1 -- the reference's order):
//                 chunk culling, the predicate, block-wide ordered compaction; optionally k0 = neighbours of process 0
//   lp_triangle   lower triangle of the local covariance, one entry per thread through the triangular index
//   lp_cz_rows    the c row (covariances with the point, lp_c_entry) and the z row behind the triangle
//   lp_noise      measurement-error variances on the diagonal
//   lp_chol       unblocked Cholesky in LDS, nx extra rows riding along: behind it they hold L^-1 c, L^-1 z, ..
//   lp_dots       v . y and v . v by a 256-wide LDS tree;  lp_write / lp_write_nan: pred, v . v, err = nanmax(sqrt(c0 - v.v), 0)
//   vt_tree / vg_tree   the fixed trees of the Vecchia terms (sum, sum, first bad) and of the 13 score columns
// and the kernels that compose them:
//   k_local_count       lp_point, the predicate, a count                        (uncapped call)
//   k_local_select      lp_point within max_dist, radix select (ck_select.h)    (capped call: counts, cut distances)
//   k_local_solve       k <= LP_KL: lp_point lp_compact lp_triangle lp_cz_rows lp_noise lp_chol(2) lp_dots lp_write
//   k_local_solve_big   k <= "local_tile_min": lp_point lp_compact, its own row-by-row triangle, lp_cz_rows lp_noise, a blocked
//                       Cholesky on a slab in global memory, lp_dots lp_write
//   k_local_search_t    the tiled path (batched 64-column steps on the matrix cores, ck_la.hip): lp_point lp_compact (with k0),
//                       padding, lp_c_entry;  k_local_assemble_t: the triangle from a table in LDS;  k_local_reduce_t:
//                       lp_dots lp_write
//   k_local_solve_u     universal cokriging, k <= LP_KL: lp_point lp_compact (with k0) lp_triangle lp_cz_rows, trend rows,
//                       lp_noise lp_chol(2 + p), Gram matrix, GLS step (ck_local_gls.h);  tiled: k_local_trend_rows_t /
//                       k_local_reduce_ut behind the tiled path
//   k_local_solve_b     block cokriging, k <= LP_KL: k_local_solve_u's calls around the block's centre with lp_cbar_z_rows for
//                       lp_cz_rows (cbar = the members' weighted covariances, lp_cbar_part);  tiled: k_local_search_t<true>
//   k_local_solve_pair  both processes at a point (ck_predict_local_pair), k <= LP_KL: k_local_solve's calls with lp_cz_rows_pair
//                       for lp_cz_rows, lp_chol(3), lp_write_pair (three lp_dots);  tiled: k_local_search_t<false, true> /
//                       k_local_reduce_pair_t
//   k_vecchia_terms / k_vecchia_sum            vt_tree
//   k_vecchia_grad      k_local_solve's calls, then back substitution and the contraction (ck_vecchia_grad.h)
//   k_vecchia_grad_part / k_vecchia_grad_sum   vg_tree
//   k_vecchia_info      k_vecchia_grad's calls up to the back substitution, then the product D b, the forward substitution and
//                       the combination (ck_vecchia_info.h);  k_vecchia_info_part / k_vecchia_info_sum: vg_tree, 7 x 13 columns
//   k_vecchia_trend     k_local_solve's calls with the p trend rows of k_local_solve_u riding along, then mu, v . v and the first
//                       column of the Gram matrix (ck_loglik_vecchia_trend);  k_vecchia_trend_terms: k_vecchia_terms plus a
//                       datum's row (ck_vecchia_trend.h);  k_vecchia_trend_gram: G = R^T R, 256 rows per workgroup, then
//                       k_vecchia_info_sum on 12 x 13 columns;  k_vecchia_residual: z - X beta for k_vecchia_grad
//   k_local_sim_weights k_vecchia_grad's calls up to the back substitution, then the weights kept: all of the set, the earlier
//                       sites' once more as (position, weight) rows, the data's share of the mean (ck_simulate_local);
//                       k_local_sim_level: one level of the draws' recursion;  k_local_sim_gather / _scatter: the caller's noise
//                       into the recursion's layout, the draws back into the caller's order
// The Vecchia likelihood (ck_loglik_vecchia) runs the prediction kernels with the data as the points and one more predicate
// in the search: only sites that come earlier in the caller's ordering (lp_later).
// Cross-validation by folds and buffers (ck_cv_local_folds) runs them with the data as the points and two more: a site that
// carries the point's fold label, or lies within the buffer radius of its process, takes no part (lp_same_fold, lp_in_reach);
//   k_cv_labels         the labels of both processes into the internal site order;  k_cv_fold_scores: a fold's five sums
#include "ck_internal.h"
#include "ck_rng.h"
#include "ck_select.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

#define LP_TPB 256
#define LP_KL 64             // (64 + 2) * 64 doubles = 34 KB of LDS: four workgroups per CU (with 124 and one
                             // workgroup per CU the kernel was 2x slower than the tiled path from k ~ 40 on)

__device__ __forceinline__ double lp_dist(int metric, double a0, double a1, double a2, double b0, double b1,
                                          double b2) {
    return metric == CK_METRIC_HAVERSINE ? ck_haversine_km(a0, a1, a2, b0, b1, b2) : ck_euclid(a0, a1, b0, b1);
}

// ---- the point ----
// What a point's search compares against: the cut distance of either process and the culling chord.
struct LpReach {
    double r0, r1, cmax;
};
struct LpPoint {
    double p0, p1, p2;                 // exact-formula coordinates
    double q0, q1, q2;                 // chord vector
    LpReach Q;
    int rp;                            // position in the ordering (precedence), 0 without one
    int fp;                            // fold label (withholding), -1 without one
    const double *s0, *s1, *s2;        // the sites' coordinate rows
    const double *u0, *u1, *u2;        // and chord-vector rows (table path)
};
// own_reach: the point's cut distances and culling chord from the select pass where the call has a neighbour cap (P.rq);
// false: max_dist and the host's cmax whatever P.rq holds -- the select pass itself, which searches the candidates
__device__ __forceinline__ LpPoint lp_point(const CkLocalProblem& P, long p, bool own_reach = true) {
    LpPoint X;
    X.p0 = P.pc[p], X.p1 = P.pc[P.mpad + p], X.p2 = P.pc[2 * P.mpad + p];
    X.q0 = P.pu[p], X.q1 = P.pu[P.mpad + p], X.q2 = P.pu[2 * P.mpad + p];
    X.Q = (own_reach && P.rq) ? LpReach{P.rq[2 * p], P.rq[2 * p + 1], P.cp[p]} : LpReach{P.max_dist, P.max_dist, P.cmax};
    X.rp = P.rs ? P.rp[p] : 0;
    X.fp = P.fs ? P.fp[p] : -1;
    X.s0 = P.sc, X.s1 = P.sc + P.L.npad, X.s2 = P.sc + 2 * P.L.npad;
    X.u0 = P.su, X.u1 = P.su + P.L.npad, X.u2 = P.su + 2 * P.L.npad;
    return X;
}

// ---- the search ----
// Precedence (ck_loglik_vecchia): a site takes part only if it comes earlier in the ordering than the point.
__device__ __forceinline__ bool lp_later(const CkLocalProblem& P, const LpPoint& X, long g) { return P.rs && !(P.rs[g] < X.rp); }

// Withholding by fold (ck_cv_local_folds): a site that carries the point's own label takes no part.  A label is loaded only
// where the call has labels.
__device__ __forceinline__ bool lp_same_fold(const CkLocalProblem& P, const LpPoint& X, long g) {
    if (!P.fs) return false;
    const int f = P.fs[g];
    return f >= 0 && f == X.fp;
}
// the conditions that read a per-site list, behind one uniform gate: a call without either pays one scalar branch
__device__ __forceinline__ bool lp_listed_out(const CkLocalProblem& P, const LpPoint& X, long g) {
    return P.listed && (lp_later(P, X, g) || lp_same_fold(P, X, g));
}
// The distance conditions: d <= lim, and where the call has a lower cut (P.cv: the reference's cross-validation flag, lo = 0 for
// process i_pred -- the compare is d > 0.0 -- or the buffer radii of ck_cv_local_folds; -1 for a process without one) also d > lo.
__device__ __forceinline__ bool lp_in_reach(const CkLocalProblem& P, int proc, double d, double lim) {
    if (P.cv) return d > (proc ? P.lo[1] : P.lo[0]) && d <= lim;
    return d <= lim;
}

// the radius predicate within max_dist (the candidates of the neighbour cap): *d is the device distance, *proc the site's process
__device__ __forceinline__ bool lp_candidate(const CkLocalProblem& P, const LpPoint& X, long g, double* d, int* proc) {
    const CkLayout& L = P.L;
    if (!(g < L.n0 || (g >= L.n0p && g < L.nend))) return false;
    if (lp_listed_out(P, X, g)) return false;
    *d = lp_dist(P.metric, X.p0, X.p1, X.p2, X.s0[g], X.s1[g], X.s2[g]);
    *proc = g >= L.n0p;
    return lp_in_reach(P, *proc, *d, P.max_dist);
}

// the same within the point's reach
__device__ __forceinline__ bool lp_is_neighbour(const CkLocalProblem& P, const LpPoint& X, long g) {
    const CkLayout& L = P.L;
    if (!(g < L.n0 || (g >= L.n0p && g < L.nend))) return false;
    if (lp_listed_out(P, X, g)) return false;
    const double d = lp_dist(P.metric, X.p0, X.p1, X.p2, X.s0[g], X.s1[g], X.s2[g]);
    const int proc = g >= L.n0p;
    return lp_in_reach(P, proc, d, proc ? X.Q.r1 : X.Q.r0);
}

// Radius search with chunk culling: the sites are laid out along a Hilbert curve (ck_api.hip: site_order), so
// 256 consecutive sites are a compact patch.  Per chunk: the mean c of its chord vectors and rad = max |u - c|
// (P.cb: 4 x nchunk -- centre x, y, z, rad; rad < 0: no valid site in the chunk).
// A site can only be within max_dist of a point with chord vector q if its chord to q is <= cmax (haversine:
// 2 sin(max_dist / 2R), monotone; Euclid: max_dist), and |u - q| >= |c - q| - rad, so a chunk with
// |c - q| - rad > cmax holds no neighbour and is skipped by the whole workgroup.  cmax carries a relative
// margin of 1e-9 (host), far above the rounding of either formula; which sites pass is still decided by the
// reference's distance formula, so the neighbour lists do not change.
__host__ __device__ __forceinline__ long lp_nchunk(const CkLayout& L) { return (long)((L.nend + LP_TPB - 1) / LP_TPB); }

__device__ __forceinline__ bool lp_chunk_far(const CkLocalProblem& P, const LpPoint& X, long chunk) {
    const long nchunk = lp_nchunk(P.L);
    if (chunk >= nchunk) return true;
    const double rad = P.cb[3 * nchunk + chunk];
    if (rad < 0.0) return true;
    const double dx = P.cb[chunk] - X.q0, dy = P.cb[nchunk + chunk] - X.q1, dz = P.cb[2 * nchunk + chunk] - X.q2;
    return sqrt(dx * dx + dy * dy + dz * dz) - rad > X.Q.cmax;
}

// The neighbour list, in site order: block-wide ordered compaction into idx.  K0: *k0 = the neighbours of process 0 (a
// second ballot and counter, paid only here).  CAP > 0: the capacity of idx, entries beyond it are dropped.  Uniform path:
// every thread reaches both barriers of every chunk that is not culled.
template <bool K0, int CAP>
__device__ __forceinline__ void lp_compact(const CkLocalProblem& P, const LpPoint& X, int* idx, int* k0 = nullptr) {
    __shared__ int wsum[K0 ? 2 : 1][LP_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0, n0 = 0;
    for (long g0 = 0; g0 < P.L.nend; g0 += LP_TPB) {
        if (lp_chunk_far(P, X, g0 / LP_TPB)) continue;   // uniform
        const long g = g0 + tid;
        const bool f = g < P.L.nend && lp_is_neighbour(P, X, g);
        const unsigned long long bal = __ballot(f);
        const int below = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) wsum[0][wv] = __popcll(bal);
        if (K0) {
            const unsigned long long bal0 = __ballot(f && g < P.L.n0p);
            if (lane == 0) wsum[K0 ? 1 : 0][wv] = __popcll(bal0);
        }
        __syncthreads();
        int off = base;
        for (int w2 = 0; w2 < wv; ++w2) off += wsum[0][w2];
        if (f && (CAP <= 0 || off + below < CAP)) idx[off + below] = (int)g;
        for (int w2 = 0; w2 < LP_TPB / 64; ++w2) {
            base += wsum[0][w2];
            if (K0) n0 += wsum[K0 ? 1 : 0][w2];
        }
        __syncthreads();
    }
    if (K0) *k0 = n0;
}

// ---- the local system ----
// Covariance of a pair: through the block's table (ck_math.h "Tabulated covariance"; coefficients read from
// global memory / L2 here -- three 48 KB tables do not fit next to the local system in LDS) when the pair's
// squared chord is inside the table, else the exact evaluator (closer than the table's lower end incl.
// h == 0 and the nugget, beyond its upper end, or tables disabled).
// the exact formulas out of line: rare beside the table, and inlined they cost the callers their registers
__device__ __noinline__ double lp_exact_xyz(const CkMatern* m, int metric, int nug, double a0, double a1, double a2,
                                            double b0, double b1, double b2) {
    return ck_cov_entry(*m, lp_dist(metric, a0, a1, a2, b0, b1, b2), nug);
}

__device__ __forceinline__ double lp_cov(const CkLocalProblem& P, int bidx, int nug, double a0, double a1, double a2,
                                         double au0, double au1, double au2, double b0, double b1, double b2, double bu0,
                                         double bu1, double bu2) {
    if (P.use_tab) {
        const double dx = au0 - bu0, dy = au1 - bu1, dz = au2 - bu2;
        const double q = dx * dx + dy * dy + dz * dz;
        int iv;
        const double y = ck_table_y(q, &iv, P.tabs[bidx].base);
        if ((unsigned)iv < (unsigned)P.tabs[bidx].n_int) return ck_table_poly(P.coefs[bidx], iv, y);
    }
    return lp_exact_xyz(&P.blk[bidx], P.metric, nug, a0, a1, a2, b0, b1, b2);
}

// the point's covariance, as process ip, with site ga (point_prediction.py:115-125)
__device__ __forceinline__ double lp_c_entry_of(const CkLocalProblem& P, const LpPoint& X, long ga, int ip) {
    const int pa = ga >= P.L.n0p;
    return lp_cov(P, ip + pa, pa == ip, X.p0, X.p1, X.p2, X.q0, X.q1, X.q2, X.s0[ga], X.s1[ga], X.s2[ga], X.u0[ga], X.u1[ga],
                  X.u2[ga]);
}
// as the call's predicted process
__device__ __forceinline__ double lp_c_entry(const CkLocalProblem& P, const LpPoint& X, long ga) {
    return lp_c_entry_of(P, X, ga, P.i_pred);
}

// Block cokriging: the members [a0, a1) of a block (P.mc / P.mu / P.bw) against site ga, summed in the members' order:
// sum_a w_a C_{i, proc(ga)}(x_a, s_ga), every term lp_c_entry's evaluation with the member in the point's place.  The first
// term starts the sum, so a single member of weight 1 gives lp_c_entry's value itself.
__device__ __forceinline__ double lp_cbar_part(const CkLocalProblem& P, const LpPoint& X, long ga, int a0, int a1) {
    const int pa = ga >= P.L.n0p;
    const double b0 = X.s0[ga], b1 = X.s1[ga], b2 = X.s2[ga], bu0 = X.u0[ga], bu1 = X.u1[ga], bu2 = X.u2[ga];
    const double *m0 = P.mc, *m1 = P.mc + P.bmpad, *m2 = P.mc + 2 * P.bmpad;
    const double *v0 = P.mu, *v1 = P.mu + P.bmpad, *v2 = P.mu + 2 * P.bmpad;
    double acc = 0.0;
    for (int a = a0; a < a1; ++a) {
        const double t = P.bw[a] * lp_cov(P, P.i_pred + pa, pa == P.i_pred, m0[a], m1[a], m2[a], v0[a], v1[a], v2[a], b0, b1, b2,
                                          bu0, bu1, bu2);
        acc = a == a0 ? t : acc + t;
    }
    return acc;
}

// rows k (cbar) and k + 1 (z) of S for block p, k <= LP_KL.  The q k covariance evaluations are spread as (neighbour, member
// slice) pairs: the members are cut into nsl = LP_TPB / k slices of consecutive members, thread s k + g sums slice s against
// neighbour g into part[s k + g], and thread g adds the slices that hold a member in ascending order -- one fixed order for
// given (q, k), so repeated calls give the same bits.  part: LP_TPB doubles of LDS.
__device__ __forceinline__ void lp_cbar_z_rows(const CkLocalProblem& P, const LpPoint& X, long p, const int* idx, double* S, long ld,
                                               int k, double* part) {
    const int tid = threadIdx.x;
    const int a0 = P.bo[p], q = P.bo[p + 1] - a0;
    const int nsl = LP_TPB / k;
    const int qs = (q + nsl - 1) / nsl;   // members per slice
    const int nus = (q + qs - 1) / qs;    // slices that hold a member (<= nsl)
    const int g = tid % k, s = tid / k;
    if (s < nus) part[s * k + g] = lp_cbar_part(P, X, idx[g], a0 + s * qs, a0 + min(q, (s + 1) * qs));
    __syncthreads();
    if (tid < k) {
        double acc = part[tid];
        for (int s2 = 1; s2 < nus; ++s2) acc += part[s2 * k + tid];
        S[(long)k * ld + tid] = acc;
        S[(long)(k + 1) * ld + tid] = P.z[idx[tid]];
    }
}

// lower triangle of the k x k local covariance into S (leading dimension ld), one entry per thread and pass
__device__ __forceinline__ void lp_triangle(const CkLocalProblem& P, const LpPoint& X, const int* idx, double* S, long ld, int k) {
    const long npair = (long)k * (k + 1) / 2;
    for (long e = threadIdx.x; e < npair; e += LP_TPB) {
        // e -> (a, b), a >= b:  a = floor((sqrt(8e + 1) - 1) / 2)
        long a = (long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (a * (a + 1) / 2 > e) --a;
        while ((a + 1) * (a + 2) / 2 <= e) ++a;
        const long b = e - a * (a + 1) / 2;
        const long ga = idx[a], gb = idx[b];
        const int pa = ga >= P.L.n0p, pb = gb >= P.L.n0p;
        S[a * ld + b] = lp_cov(P, pa + pb, pa == pb, X.s0[ga], X.s1[ga], X.s2[ga], X.u0[ga], X.u1[ga], X.u2[ga], X.s0[gb],
                               X.s1[gb], X.s2[gb], X.u0[gb], X.u1[gb], X.u2[gb]);
    }
}

// rows k (c) and k + 1 (z) of S
__device__ __forceinline__ void lp_cz_rows(const CkLocalProblem& P, const LpPoint& X, const int* idx, double* S, long ld, int k) {
    for (int a = threadIdx.x; a < k; a += LP_TPB) {
        const long ga = idx[a];
        S[(long)k * ld + a] = lp_c_entry(P, X, ga);
        S[(long)(k + 1) * ld + a] = P.z[ga];
    }
}

// the pair form (ck_predict_local_pair): rows k (c as process 0), k + 1 (c as process 1) and k + 2 (z) of S
__device__ __forceinline__ void lp_cz_rows_pair(const CkLocalProblem& P, const LpPoint& X, const int* idx, double* S, long ld, int k) {
    for (int a = threadIdx.x; a < k; a += LP_TPB) {
        const long ga = idx[a];
        S[(long)k * ld + a] = lp_c_entry_of(P, X, ga, 0);
        S[(long)(k + 1) * ld + a] = lp_c_entry_of(P, X, ga, 1);
        S[(long)(k + 2) * ld + a] = P.z[ga];
    }
}

// closes the assembly (barrier), then the measurement-error variances (ck_set_noise): the neighbour's s d on the true diagonal
__device__ __forceinline__ void lp_noise(const CkLocalProblem& P, const int* idx, double* S, long ld, int k) {
    __syncthreads();
    if (P.nz) {
        for (int a = threadIdx.x; a < k; a += LP_TPB) S[(long)a * ld + a] += P.nz[idx[a]];
        __syncthreads();
    }
}

// Cholesky of the k x k block of S in LDS; the nx rows below it ride along (forward substitution).  False: a pivot was not
// > 0 (src/point_prediction.py:218-222).  Every thread takes the same path: the pivot is read by all, the break is uniform.
__device__ __forceinline__ bool lp_chol(double* S, long ld, int k, int nx) {
    __shared__ int fail;
    const int tid = threadIdx.x;
    if (tid == 0) fail = 0;
    for (int j = 0; j < k; ++j) {
        const double piv = S[(long)j * ld + j];
        if (!(piv > 0.0)) {
            if (tid == 0) fail = 1;
            break;   // uniform: every thread reads the same pivot
        }
        const double rd = 1.0 / sqrt(piv);
        __syncthreads();
        for (int a = j + 1 + tid; a < k + nx; a += LP_TPB) S[(long)a * ld + j] *= rd;
        if (tid == 0) S[(long)j * ld + j] = sqrt(piv);
        __syncthreads();
        // S[a][b] -= S[a][j] S[b][j] for j < b <= min(a, k - 1), a in (j, k + nx)
        const int nb = k - 1 - j;            // columns b = j + 1 .. k - 1
        const int na = k + nx - 1 - j;       // rows    a = j + 1 .. k + nx - 1
        const long tot = (long)na * nb;
        for (long e = tid; e < tot; e += LP_TPB) {
            const int a = j + 1 + (int)(e / nb), b = j + 1 + (int)(e % nb);
            if (b <= a) S[(long)a * ld + b] -= S[(long)a * ld + j] * S[(long)b * ld + j];
        }
        __syncthreads();
    }
    __syncthreads();
    return fail == 0;
}

// ---- the outputs ----
// v . y and v . v over k entries of the two solved rows: a strided partial sum per thread, then the 256-wide tree in LDS.
// Every thread returns with both sums.
__device__ __forceinline__ void lp_dots(const double* v, const double* y, int k, double* vy, double* vv) {
    __shared__ double red[2][LP_TPB];
    const int tid = threadIdx.x;
    double s1v = 0.0, s2v = 0.0;
    for (int a = tid; a < k; a += LP_TPB) {
        s1v += v[a] * y[a];
        s2v += v[a] * v[a];
    }
    red[0][tid] = s1v;
    red[1][tid] = s2v;
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    *vy = red[0][0];
    *vv = red[1][0];
}

// one thread: pred = v . y, the raw v . v where asked for (ck_loglik_vecchia: the unclamped variance is the caller's),
// err = np.nanmax([sqrt(c0 - v . v), 0.0]) (point_prediction.py:217)
__device__ __forceinline__ void lp_write(long p, double vy, double vv, double c0var, double* pred, double* err, double* vvout) {
    pred[p] = vy;
    if (vvout) vvout[p] = vv;
    const double sd = sqrt(c0var - vv);
    err[p] = (sd == sd) ? fmax(sd, 0.0) : 0.0;
}

// one thread: an empty neighbourhood (src/point_prediction.py:229-233) or a system that is not positive definite (:218-222)
__device__ __forceinline__ void lp_write_nan(long p, double* pred, double* err) {
    pred[p] = NAN;
    err[p] = NAN;
}

// The pair form's outputs (ck_predict_local_pair) from the solved rows v0, v1, y: three calls of lp_dots -- (v0, y), (v1, y),
// (v0, v1) -- on its one tree, a barrier between them (a thread may still be reading the last call's root), so pred_q and
// v_q . v_q are the single calls' bits; then one thread writes lp_write's outputs of both processes and C_01(0) - v0 . v1.
// An empty neighbourhood or a system that is not positive definite: lp_write_pair_nan.
__device__ __forceinline__ void lp_write_pair(const CkLocalPairOut& O, long p, const double* v0, const double* v1, const double* y,
                                              int k) {
    double vy0, vv0, vy1, vv1, v01, unused;
    lp_dots(v0, y, k, &vy0, &vv0);
    __syncthreads();
    lp_dots(v1, y, k, &vy1, &vv1);
    __syncthreads();
    lp_dots(v0, v1, k, &v01, &unused);
    if (threadIdx.x == 0) {
        lp_write(p, vy0, vv0, O.c0var[0], O.pred0, O.err0, nullptr);
        lp_write(p, vy1, vv1, O.c0var[1], O.pred1, O.err1, nullptr);
        O.cov[p] = O.c01 - v01;
    }
}
__device__ __forceinline__ void lp_write_pair_nan(const CkLocalPairOut& O, long p) {
    lp_write_nan(p, O.pred0, O.err0);
    lp_write_nan(p, O.pred1, O.err1);
    O.cov[p] = NAN;
}

__global__ __launch_bounds__(LP_TPB) void k_local_chunk_bounds(const double* __restrict__ su, CkLayout L, long nchunk,
                                                                double* __restrict__ cb) {
    __shared__ double red[4][LP_TPB];
    const int tid = threadIdx.x;
    const long g = (long)blockIdx.x * LP_TPB + tid;
    const bool valid = g < L.n0 || (g >= L.n0p && g < L.nend);
    const double x = valid ? su[g] : 0.0, y = valid ? su[L.npad + g] : 0.0, zc = valid ? su[2 * L.npad + g] : 0.0;
    red[0][tid] = x;
    red[1][tid] = y;
    red[2][tid] = zc;
    red[3][tid] = valid ? 1.0 : 0.0;
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int c = 0; c < 4; ++c) red[c][tid] += red[c][tid + s];
        __syncthreads();
    }
    const double n = red[3][0];
    const double cx = n > 0.0 ? red[0][0] / n : 0.0, cy = n > 0.0 ? red[1][0] / n : 0.0, cz = n > 0.0 ? red[2][0] / n : 0.0;
    __syncthreads();
    const double dx = x - cx, dy = y - cy, dz = zc - cz;
    red[0][tid] = valid ? sqrt(dx * dx + dy * dy + dz * dz) : 0.0;
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) red[0][tid] = fmax(red[0][tid], red[0][tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        cb[blockIdx.x] = cx;
        cb[nchunk + blockIdx.x] = cy;
        cb[2 * nchunk + blockIdx.x] = cz;
        cb[3 * nchunk + blockIdx.x] = n > 0.0 ? red[0][0] * (1.0 + 1e-12) : -1.0;
    }
}

void ck_launch_local_chunk_bounds(hipStream_t s, const double* su, CkLayout L, double* cb) {
    const long nchunk = (L.nend + LP_TPB - 1) / LP_TPB;
    if (nchunk <= 0) return;
    k_local_chunk_bounds<<<dim3((unsigned)nchunk), dim3(LP_TPB), 0, s>>>(su, L, nchunk, cb);
}

// neighbour count per prediction point
__global__ __launch_bounds__(LP_TPB) void k_local_count(CkLocalProblem P, int* __restrict__ counts) {
    __shared__ int red[LP_TPB];
    const long p = blockIdx.x;
    const LpPoint X = lp_point(P, p);
    int c = 0;
    for (long g0 = 0; g0 < P.L.nend; g0 += LP_TPB) {
        if (lp_chunk_far(P, X, g0 / LP_TPB)) continue;
        const long g = g0 + threadIdx.x;
        c += (g < P.L.nend && lp_is_neighbour(P, X, g)) ? 1 : 0;
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[p] = red[0];
}

// ---------------------------------------------------------------------------------------
// The neighbour cap (ck_set_local_neighbours): the counting pass of a capped call
// ---------------------------------------------------------------------------------------
// One workgroup per point.  The candidates of process q -- the sites today's predicate lets through -- are cut at
// r_pq = the nmax_q-th smallest distance when there are more than nmax_q of them, and every candidate with d <= r_pq stays (ties
// at the cut included: the set is a function of the distances alone).  The order statistic comes from the radix select of
// ck_select.h over the distances' bit patterns: per round a 256-bin histogram filled with integer LDS atomics (the same
// histogram whatever the arrival order), then one thread per process narrows.  Up to key_cap candidates per process are kept
// in LDS by the first scan; a process with more re-scans its chunks and recomputes the distances every round (same keys,
// same result).  No floating-point sum anywhere: repeated calls give the same bits.
#define LS_CAP 2048   // keys per process in LDS: 2 x 16 KB

// calls f(process, key) for every candidate this thread meets, chunk by chunk as the counting pass walks them
template <class F>
__device__ __forceinline__ void ls_scan(const CkLocalProblem& P, const LpPoint& X, F f) {
    for (long g0 = 0; g0 < P.L.nend; g0 += LP_TPB) {
        if (lp_chunk_far(P, X, g0 / LP_TPB)) continue;
        const long g = g0 + threadIdx.x;
        double d;
        int proc;
        if (g < P.L.nend && lp_candidate(P, X, g, &d, &proc)) f(proc, ck_sel_key(d));
    }
}

__global__ __launch_bounds__(LP_TPB) void k_local_select(CkLocalProblem P, int nmax0, int nmax1, int key_cap,
                                                          int* __restrict__ counts, int* __restrict__ sel,
                                                          double* __restrict__ rq, double* __restrict__ cp) {
    __shared__ unsigned long long keys[2][LS_CAP];
    __shared__ unsigned hist[2][CK_SEL_BINS];
    __shared__ unsigned ncand[2];
    __shared__ CkSelState st[2];
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const int metric = P.metric;
    const double max_dist = P.max_dist;
    const CkLayout& L = P.L;
    const LpPoint X = lp_point(P, p, /*own_reach=*/false);   // the candidates are searched within max_dist
    if (tid < 2) ncand[tid] = 0;
    __syncthreads();
    ls_scan(P, X, [&](int q, unsigned long long key) {
        const unsigned slot = atomicAdd(&ncand[q], 1u);
        if (slot < (unsigned)key_cap) keys[q][slot] = key;
    });
    __syncthreads();
    // everything below is uniform (scalar branches around the barriers); bit q of a mask speaks of process q (no array is
    // indexed at run time)
    const int nc0 = __builtin_amdgcn_readfirstlane((int)ncand[0]), nc1 = __builtin_amdgcn_readfirstlane((int)ncand[1]);
    const unsigned capped = (nmax0 > 0 && nc0 > nmax0 ? 1u : 0u) | (nmax1 > 0 && nc1 > nmax1 ? 2u : 0u);
    const unsigned rescan = capped & ((nc0 > key_cap ? 1u : 0u) | (nc1 > key_cap ? 2u : 0u));
    if (capped) {
        if (tid < 2 && (capped >> tid & 1u)) ck_sel_begin(&st[tid], tid ? nmax1 : nmax0);
        for (int round = 0; round < CK_SEL_ROUNDS; ++round) {
            for (int e = tid; e < 2 * CK_SEL_BINS; e += LP_TPB) hist[e / CK_SEL_BINS][e % CK_SEL_BINS] = 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (!((capped & ~rescan) >> q & 1u)) continue;
                const int n = q ? nc1 : nc0;
                for (int e = tid; e < n; e += LP_TPB) {
                    const unsigned long long key = keys[q][e];
                    if (ck_sel_match(&st[q], key)) atomicAdd(&hist[q][ck_sel_digit(&st[q], key)], 1u);
                }
            }
            if (rescan)
                ls_scan(P, X, [&](int q, unsigned long long key) {
                    if ((rescan >> q & 1u) && ck_sel_match(&st[q], key)) atomicAdd(&hist[q][ck_sel_digit(&st[q], key)], 1u);
                });
            __syncthreads();
            if ((tid == 0 || tid == 64) && (capped >> (tid >> 6) & 1u)) ck_sel_narrow(&st[tid >> 6], hist[tid >> 6]);   // a wave per process
            __syncthreads();
        }
    }
    if (tid == 0) {
        const double r0 = (capped & 1u) ? ck_sel_dist(st[0].prefix) : max_dist, r1 = (capped & 2u) ? ck_sel_dist(st[1].prefix) : max_dist;
        const int k0 = (capped & 1u) ? (int)(st[0].less + st[0].ties) : nc0, k1 = (capped & 2u) ? (int)(st[1].less + st[1].ties) : nc1;
        rq[2 * p] = r0;
        rq[2 * p + 1] = r1;
        sel[4 * p] = k0;
        sel[4 * p + 1] = k1;
        sel[4 * p + 2] = nc0 + nc1;
        sel[4 * p + 3] = (capped ? CK_LS_CAPPED : 0) | (rescan ? CK_LS_RESCAN : 0);
        counts[p] = k0 + k1;
        // the chord of the point's reach, with the margin of cmax; a process without sites does not widen it
        const double reach = L.nend > L.n0p ? fmax(r0, r1) : r0;
        double c = P.cmax;
        if (reach < max_dist) {
            c = reach;
            if (metric == CK_METRIC_HAVERSINE) {
                const double half = reach / (2.0 * CK_EARTH_RADIUS_KM);
                c = half >= 1.5 ? 4.0 : 2.0 * sin(half);
            }
            c = fmin(c * (1.0 + 1e-9) + 1e-12, P.cmax);
        }
        cp[p] = c;
    }
}

// Systems of k <= LP_KL neighbours, in LDS: a (k + 2) x k matrix (rows k, k + 1 carry c and z) and the neighbour list
__global__ __launch_bounds__(LP_TPB) void k_local_solve(CkLocalProblem P, const int* __restrict__ counts, long p_base, int k_hi,
                                                         double* __restrict__ pred, double* __restrict__ err,
                                                         double* __restrict__ vv) {
    __shared__ double S[(LP_KL + 2) * LP_KL];
    __shared__ int idx[LP_KL];
    const int tid = threadIdx.x;
    const long p = p_base + blockIdx.x;
    const int k = counts[p];
    if (k == 0) {
        if (tid == 0) lp_write_nan(p, pred, err);
        return;
    }
    if (k > LP_KL || k > k_hi) return;   // larger systems: k_local_solve_big / the tiled path
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    lp_compact<false, 0>(P, X, idx);           // 1. neighbour list
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, noise
    lp_cz_rows(P, X, idx, S, ld, k);
    lp_noise(P, idx, S, ld, k);
    if (!lp_chol(S, ld, k, 2)) {               // 3. Cholesky, the two extra rows ride along
        if (tid == 0) lp_write_nan(p, pred, err);
        return;
    }
    double vy, v2;                             // 4. pred = v . y, var = c0 - v . v
    lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &vy, &v2);
    if (tid == 0) lp_write(p, vy, v2, P.c0var, pred, err, vv);
}

// ---------------------------------------------------------------------------------------
// Neighbourhoods beyond the LDS limit: blocked Cholesky of the local system in a global slab
// ---------------------------------------------------------------------------------------
// Same steps as k_local_solve (neighbour list in site order, local covariance with the c and z rows
// riding along, forward substitution only).  The factorisation is blocked: LB_IB columns are
// factored in place (unblocked, rank-1 updates confined to the column panel), then the trailing
// matrix is updated ONCE with all of them -- 64 x 64 tiles, the two LB_IB-wide operand strips of
// a tile staged (transposed) in LDS, a 4 x 4 register tile per thread.  The unblocked form makes
// one pass over the trailing matrix per COLUMN: k / LB_IB times the memory traffic (it measured
// 0.4 TFLOP/s at k = 1 359).
#define LB_IB 32
#define LB_PR 128   // panel rows per pass; LB_IB * (LB_PR + 1) <= 2 * LB_IB * 68 doubles of LDS
__global__ __launch_bounds__(LP_TPB, 3) void k_local_solve_big(CkLocalProblem P, const int* __restrict__ counts,
                                                             const long long* __restrict__ slab_off,
                                                             double* __restrict__ slab, long p_base, int k_hi,
                                                             double* __restrict__ pred, double* __restrict__ err,
                                                             double* __restrict__ vv) {
    __shared__ __attribute__((aligned(16))) double lbuf[2 * LB_IB * (64 + 4)];
    double (*At)[64 + 4] = reinterpret_cast<double (*)[64 + 4]>(lbuf);                 // At[c][r] = strip of the tile's rows
    double (*Bt)[64 + 4] = reinterpret_cast<double (*)[64 + 4]>(lbuf + LB_IB * (64 + 4));   // Bt[c][r] = ... columns
    double (*Pt)[LB_PR + 1] = reinterpret_cast<double (*)[LB_PR + 1]>(lbuf);           // panel rows (3a), same storage
    __shared__ double Ld[LB_IB][LB_IB + 1];   // diagonal block of the column panel
    __shared__ double rdiag[LB_IB], Ldiag[LB_IB];
    __shared__ int fail;
    const int tid = threadIdx.x;
    const long p = p_base + blockIdx.x;
    const int k = counts[p];
    if (k <= LP_KL || k > k_hi) return;   // k_local_solve (also the empty neighbourhoods) / the tiled path
    const LpPoint X = lp_point(P, p);
    double* S = slab + slab_off[p];   // (k + 2) x k, rows k and k + 1 carry c and z
    int* idx = reinterpret_cast<int*>(S + (long)(k + 2) * k);
    const long ld = k;
    if (tid == 0) fail = 0;
    lp_compact<false, 0>(P, X, idx);   // 1. neighbour list
    // ---- 2. local covariance (lower triangle), c row, z row, noise ----
    for (int a = 0; a < k; ++a) {   // row by row: coalesced writes, no sqrt to invert the triangular index
        const long ga = idx[a];
        const int pa = ga >= P.L.n0p;
        const double a0 = X.s0[ga], a1 = X.s1[ga], a2 = X.s2[ga], au0 = X.u0[ga], au1 = X.u1[ga], au2 = X.u2[ga];
        for (int b = tid; b <= a; b += LP_TPB) {
            const long gb = idx[b];
            const int pb = gb >= P.L.n0p;
            S[(long)a * ld + b] = lp_cov(P, pa + pb, pa == pb, a0, a1, a2, au0, au1, au2, X.s0[gb], X.s1[gb], X.s2[gb], X.u0[gb],
                                         X.u1[gb], X.u2[gb]);
        }
    }
    lp_cz_rows(P, X, idx, S, ld, k);
    lp_noise(P, idx, S, ld, k);
    // ---- 3. blocked Cholesky; rows k, k + 1 ride along (forward substitution) ----
    const int ty = tid >> 4, tx = tid & 15;
    bool bad = false;
    for (int jb = 0; jb < k && !bad; jb += LB_IB) {
        const int nbc = (k - jb < LB_IB) ? (k - jb) : LB_IB;
        const int jend = jb + nbc;
        // 3a. the column panel jb .. jend - 1: its diagonal block is factored in LDS (padded to LB_IB with the
        //     identity), then every row below is solved against it -- one thread per row, the row's LB_IB
        //     entries in registers, LB_PR rows per pass staged through LDS so that global memory sees whole
        //     256-byte row segments.  (Column-at-a-time on the slab walked it with a stride of k doubles:
        //     one cache line per entry, k times over -- half of this kernel's time at k = 1 359.)
        for (int e = tid; e < LB_IB * LB_IB; e += LP_TPB) {
            const int r = e / LB_IB, c = e % LB_IB;
            Ld[r][c] = (r < nbc && c <= r) ? S[(long)(jb + r) * ld + jb + c] : (r == c ? 1.0 : 0.0);
        }
        __syncthreads();
        for (int j = 0; j < LB_IB; ++j) {
            const double piv = Ld[j][j];
            if (!(piv > 0.0)) {   // uniform: every thread reads the same pivot
                if (tid == 0) fail = 1;
                bad = true;
                break;
            }
            const double rd = 1.0 / sqrt(piv);
            if (tid > j && tid < LB_IB) Ld[tid][j] *= rd;
            if (tid == 0) {
                rdiag[j] = rd;
                Ldiag[j] = sqrt(piv);
            }
            __syncthreads();
            for (int e = tid; e < LB_IB * LB_IB; e += LP_TPB) {
                const int a = e / LB_IB, b = e % LB_IB;
                if (b > j && a >= b) Ld[a][b] -= Ld[a][j] * Ld[b][j];
            }
            __syncthreads();
        }
        if (bad) break;
        for (int e = tid; e < LB_IB * LB_IB; e += LP_TPB) {
            const int r = e / LB_IB, c = e % LB_IB;
            if (r < nbc && c <= r) S[(long)(jb + r) * ld + jb + c] = (r == c) ? Ldiag[r] : Ld[r][c];
        }
        for (int r0 = jend; r0 < k + 2; r0 += LB_PR) {
            for (int e = tid; e < LB_PR * LB_IB; e += LP_TPB) {
                const int r = e / LB_IB, c = e % LB_IB, a = r0 + r;
                Pt[c][r] = (a < k + 2 && c < nbc) ? S[(long)a * ld + jb + c] : 0.0;
            }
            __syncthreads();
            if (tid < LB_PR) {
                double x[LB_IB];
#pragma unroll
                for (int c = 0; c < LB_IB; ++c) x[c] = Pt[c][tid];
#pragma unroll
                for (int j = 0; j < LB_IB; ++j) {
                    x[j] *= rdiag[j];
#pragma unroll
                    for (int c = j + 1; c < LB_IB; ++c) x[c] -= x[j] * Ld[c][j];
                }
#pragma unroll
                for (int c = 0; c < LB_IB; ++c) Pt[c][tid] = x[c];
            }
            __syncthreads();
            for (int e = tid; e < LB_PR * LB_IB; e += LP_TPB) {
                const int r = e / LB_IB, c = e % LB_IB, a = r0 + r;
                if (a < k + 2 && c < nbc) S[(long)a * ld + jb + c] = Pt[c][r];
            }
            __syncthreads();
        }
        // 3b. trailing update  S[a][b] -= sum_c S[a][jb + c] S[b][jb + c],  a in [jend, k + 2), b in [jend, min(a, k - 1)]
        const int nrow = k + 2 - jend, ncol = k - jend;
        const int tr = (nrow + 63) / 64, tc = (ncol + 63) / 64;
        for (int ta = 0; ta < tr; ++ta) {
            for (int tb = 0; tb < tc && tb <= ta; ++tb) {
                for (int e = tid; e < 64 * LB_IB; e += LP_TPB) {
                    const int r = e / LB_IB, c = e % LB_IB;            // consecutive threads: consecutive columns of one row
                    const int a = jend + ta * 64 + r, b = jend + tb * 64 + r;
                    At[c][r] = (a < k + 2 && c < nbc) ? S[(long)a * ld + jb + c] : 0.0;
                    Bt[c][r] = (b < k && c < nbc) ? S[(long)b * ld + jb + c] : 0.0;
                }
                __syncthreads();
                double acc[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j2 = 0; j2 < 4; ++j2) acc[i][j2] = 0.0;
#pragma unroll 8
                for (int c = 0; c < LB_IB; ++c) {
                    const d2_t a01 = *reinterpret_cast<const d2_t*>(&At[c][4 * ty]), a23 = *reinterpret_cast<const d2_t*>(&At[c][4 * ty + 2]);
                    const d2_t b01 = *reinterpret_cast<const d2_t*>(&Bt[c][4 * tx]), b23 = *reinterpret_cast<const d2_t*>(&Bt[c][4 * tx + 2]);
                    const double av[4] = {a01[0], a01[1], a23[0], a23[1]}, bv[4] = {b01[0], b01[1], b23[0], b23[1]};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j2 = 0; j2 < 4; ++j2) acc[i][j2] = fma(av[i], bv[j2], acc[i][j2]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int a = jend + ta * 64 + 4 * ty + i;
#pragma unroll
                    for (int j2 = 0; j2 < 4; ++j2) {
                        const int b = jend + tb * 64 + 4 * tx + j2;
                        if (a < k + 2 && b < k && b <= a) S[(long)a * ld + b] -= acc[i][j2];
                    }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (fail) {
        if (tid == 0) lp_write_nan(p, pred, err);
        return;
    }
    double vy, v2;   // ---- 4. pred = v . y, var = c0 - v . v ----
    lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &vy, &v2);
    if (tid == 0) lp_write(p, vy, v2, P.c0var, pred, err, vv);
}

void ck_launch_local_count(hipStream_t s, const CkLocalProblem& P, int64_t m, int* counts) {
    if (m <= 0) return;
    k_local_count<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts);
}

int ck_local_select_capacity() { return LS_CAP; }

void ck_launch_local_select(hipStream_t s, const CkLocalProblem& P, int64_t m, int nmax0, int nmax1, int key_cap, int* counts,
                            int* sel, double* rq, double* cp) {
    if (m <= 0) return;
    key_cap = key_cap < 1 ? 1 : (key_cap > LS_CAP ? LS_CAP : key_cap);   // never beyond the LDS lists
    k_local_select<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, nmax0, nmax1, key_cap, counts, sel, rq, cp);
}

void ck_launch_local_solve(hipStream_t s, const CkLocalProblem& P, int64_t p_base, int64_t m, const int* counts,
                           const long long* slab_off, double* slab, int k_hi, double* pred, double* err, double* vv) {
    if (m <= 0) return;
    k_local_solve<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts, p_base, k_hi, pred, err, vv);
    if (slab && k_hi > LP_KL)   // some neighbourhood is larger than the LDS limit
        k_local_solve_big<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts, slab_off, slab, p_base, k_hi, pred, err, vv);
}

// Both processes at a point from one local system (ck_predict_local_pair), k <= LP_KL: k_local_solve's steps with the c rows of
// both processes riding along -- a (k + 3) x k matrix, 34 304 B of LDS, still four workgroups per CU.  With cv = 0 nothing in
// the search, the triangle or the noise looks at the predicted process, so one list, one Sigma_loc and one Cholesky serve both.
__global__ __launch_bounds__(LP_TPB) void k_local_solve_pair(CkLocalProblem P, const int* __restrict__ counts, int k_hi,
                                                              CkLocalPairOut O) {
    __shared__ double S[(LP_KL + 3) * LP_KL];
    __shared__ int idx[LP_KL];
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k == 0) {
        if (tid == 0) lp_write_pair_nan(O, p);
        return;
    }
    if (k > LP_KL || k > k_hi) return;   // the tiled path
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    lp_compact<false, 0>(P, X, idx);           // 1. neighbour list
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, both c rows, z row, noise
    lp_cz_rows_pair(P, X, idx, S, ld, k);
    lp_noise(P, idx, S, ld, k);
    if (!lp_chol(S, ld, k, 3)) {               // 3. Cholesky, the three extra rows ride along
        if (tid == 0) lp_write_pair_nan(O, p);
        return;
    }
    lp_write_pair(O, p, S + (long)k * ld, S + (long)(k + 1) * ld, S + (long)(k + 2) * ld, k);   // 4. the five outputs
}

void ck_launch_local_solve_pair(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, int k_hi,
                                const CkLocalPairOut& O) {
    if (m <= 0) return;
    k_local_solve_pair<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts, k_hi, O);
}

// ---------------------------------------------------------------------------------------
// tiled path (ck_internal.h: CkLocalSys; the factorisation steps are in ck_la.hip)
// ---------------------------------------------------------------------------------------
// the exact formulas as an out-of-line call: rare in the table kernel below, and out of line it does not inflate
// its registers
__device__ __noinline__ double lp_exact_pair(const CkMatern* m, int metric, int nug, const double* s0, const double* s1,
                                             const double* s2, long ga, long gb) {
    return ck_cov_entry(*m, lp_dist(metric, s0[ga], s1[ga], s2[ga], s0[gb], s1[gb], s2[gb]), nug);
}

// Neighbour lists and padded local systems of a batch.
// k_local_search_t (one workgroup per system): the neighbour list, the number k0 of process-0 neighbours, the
// identity padding, the zeros the 64 x 64 factorisation expects above the diagonal, the c and z rows.
// k_local_assemble_t (one launch per Matern block): the neighbours come out sorted by process (process 0 first),
// so the lower triangle splits into three regions with ONE block each -- (0,0), (1,0) and (1,1).  A launch keeps
// its block's table in LDS, like the joint assembly (ck_cov.hip), and its workgroups walk over the systems
// (loading 48 KB of table per system cost more than the entries of a 100-site neighbourhood): chord vectors of
// LT_BC columns and LT_AC rows staged in LDS, a thread takes one column of four rows at a time (four
// independent Horner chains), writes run along rows.  Entries outside the table (coincident sites, pairs beyond
// its range) and everything when the tables are off go through the exact evaluator in a second, rolled loop.
#define LT_BC 512
#define LT_WL 1024   // deferred exact pairs per system and block (LDS list; beyond that they are evaluated in place)
#define LT_AC 256
#define LT_TPB 512   // 8 waves: with two workgroups per CU (LDS) four waves per SIMD hide the table-read latency
// BLK (block cokriging): the point is the block's centre and the c row holds cbar, every entry the sum over all the block's
// members in their order (lp_cbar_part)
// PAIR (ck_predict_local_pair): three rows behind the identity padding -- kq - 3 (c as process 0), kq - 2 (c as process 1) and
// kq - 1 (z), their corner diag(BIG, BIG, BIG); kq = roundup(k + 3, 64)
template <bool BLK, bool PAIR>
__global__ __launch_bounds__(LP_TPB) void k_local_search_t(CkLocalProblem P, const CkLocalSys* __restrict__ sys,
                                                            double* __restrict__ slab, int* __restrict__ k0out) {
    constexpr int NX = PAIR ? 3 : 2;
    const int tid = threadIdx.x;
    const CkLocalSys q = sys[blockIdx.x];
    const int k = q.k, kq = q.kq;
    const long ld = q.ld;
    const LpPoint X = lp_point(P, q.p);
    double* S = slab + q.off;
    int* idx = reinterpret_cast<int*>(S + (long)CK_LT_ROWS(kq) * ld + CK_LT_NINV * 64 * 64);
    int k0;   // neighbours of process 0
    lp_compact<true, 0>(P, X, idx, &k0);
    if (tid == 0) k0out[blockIdx.x] = k0;
    // zeros up to the end of each row's 4-column diagonal block (the 64 x 64 factorisation loads whole 4 x 4
    // register blocks); rows [k, kq - NX): identity padding
    for (int a = tid; a < k; a += LP_TPB)
        for (int b = a + 1; b <= (a | 3); ++b) S[(long)a * ld + b] = 0.0;
    for (int a = k; a < kq - NX; ++a)
        for (int b = tid; b <= (a | 3); b += LP_TPB) S[(long)a * ld + b] = (b == a) ? 1.0 : 0.0;
    // rows kq - 2 (c) and kq - 1 (z): two more rows of the matrix, their own 2 x 2 corner diag(BIG, BIG); PAIR: kq - 3 (c as
    // process 0), kq - 2 (c as process 1), kq - 1 (z), a 3 x 3 corner
    for (int a = tid; a < kq; a += LP_TPB) {
        double cv0 = 0.0, cv1 = 0.0, zv = 0.0;
        if (a < k) {
            const long ga = idx[a];
            if (PAIR) {
                cv0 = lp_c_entry_of(P, X, ga, 0);
                cv1 = lp_c_entry_of(P, X, ga, 1);
            } else {
                cv0 = BLK ? lp_cbar_part(P, X, ga, P.bo[q.p], P.bo[q.p + 1]) : lp_c_entry(P, X, ga);
            }
            zv = P.z[ga];
        }
        if (PAIR) {
            S[(long)(kq - 3) * ld + a] = a == kq - 3 ? CK_LT_BIG : cv0;
            S[(long)(kq - 2) * ld + a] = a == kq - 2 ? CK_LT_BIG : cv1;
        } else {
            S[(long)(kq - 2) * ld + a] = a == kq - 2 ? CK_LT_BIG : cv0;
        }
        S[(long)(kq - 1) * ld + a] = a == kq - 1 ? CK_LT_BIG : zv;
    }
}

struct LpTab {   // the tables as k_local_assemble_t takes them (its other arguments: the descriptor's members one by one)
    const CkTable* tabs;             // [3]
    const double* const* coefs;      // [3]
    int use;
};

__global__ __launch_bounds__(LT_TPB, 4) void k_local_assemble_t(const CkMatern* __restrict__ blk, int metric, int reg,
                                                                 const double* __restrict__ sc, CkLayout L,
                                                                 const CkLocalSys* __restrict__ sys, int n_sys,
                                                                 double* __restrict__ slab, LpTab T,
                                                                 const double* __restrict__ su,
                                                                 const int* __restrict__ k0in,
                                                                 const double* __restrict__ nz) {
    __shared__ double tab[(CK_TAB_DEG + 1) * CK_TAB_STRIDE];
    __shared__ double bu[3][LT_BC];
    __shared__ double au[3][LT_AC];
    __shared__ int2 wl[LT_WL];   // (row, column) of entries the table does not cover: evaluated one pair per LANE after
    __shared__ int wl_n;         // the system's region is done, instead of one pair per WAVE where they are found
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *s0 = sc, *s1 = sc + L.npad, *s2 = sc + 2 * L.npad;
    const double *u0 = su, *u1 = su + L.npad, *u2 = su + 2 * L.npad;
    const int nug = reg != 1;
    const double cdiag = blk[reg].amp + blk[reg].nugget;   // an entry's own site: h = 0 (ck_cov_entry)
    int tbase = 0, tn = 0;                                  // tn = 0: every entry takes the exact evaluator
    if (T.use) {
        tbase = T.tabs[reg].base;
        tn = T.tabs[reg].n_int;
        const double* cf = T.coefs[reg];
        for (int e = tid; e < (CK_TAB_DEG + 1) * tn; e += LT_TPB) {
            const int kk = e / tn, iv = e - kk * tn;
            tab[kk * CK_TAB_STRIDE + iv] = cf[kk * CK_TAB_STRIDE + iv];
        }
    }
    for (int sidx = blockIdx.x; sidx < n_sys; sidx += gridDim.x) {
        const CkLocalSys q = sys[sidx];
        const int k = q.k, k0 = k0in[sidx];
        const long ld = q.ld;
        double* S = slab + q.off;
        const int* idx = reinterpret_cast<const int*>(S + (long)CK_LT_ROWS(q.kq) * ld + CK_LT_NINV * 64 * 64);
        const int alo = reg == 0 ? 0 : k0, ahi = reg == 0 ? k0 : k;
        const int blo = reg == 2 ? k0 : 0, bhi = reg == 2 ? k : k0;
        if (alo >= ahi || blo >= bhi) continue;   // uniform
        if (tid == 0) wl_n = 0;   // (ordered against the appends by the barrier at the top of the chunk loop)
        for (int bc = blo; bc < bhi; bc += LT_BC) {
            const int nbc = min(LT_BC, bhi - bc);
            __syncthreads();
            for (int e = tid; e < nbc; e += LT_TPB) {
                const long g = idx[bc + e];
                bu[0][e] = u0[g];
                bu[1][e] = u1[g];
                bu[2][e] = u2[g];
            }
            for (int ac = max(alo, bc); ac < ahi; ac += LT_AC) {
                const int nac = min(LT_AC, ahi - ac);
                __syncthreads();
                if (tid < nac) {
                    const long g = idx[ac + tid];
                    au[0][tid] = u0[g];
                    au[1][tid] = u1[g];
                    au[2][tid] = u2[g];
                }
                __syncthreads();
                // a wave takes four rows, its lanes the columns: short rows (small neighbourhoods, the top of a
                // triangle) still fill most of a wave, and a wave's stores are 512 contiguous bytes per row
                for (int r0 = 4 * wv; r0 < nac; r0 += 4 * (LT_TPB / 64)) {
                    const int nr = min(4, nac - r0), amax = ac + r0 + nr - 1;
                    for (int bl = lane; bl < nbc && bc + bl <= amax; bl += 64) {
                        const int b = bc + bl;
                        const double b0 = bu[0][bl], b1 = bu[1][bl], b2 = bu[2][bl];
                        // four rows of this column at once: chords / interval indices, then all 32 coefficient
                        // reads, then four interleaved Horner chains (the barriers keep hipcc from sinking every
                        // read next to its FMA -- one exposed LDS latency per Horner step otherwise)
                        unsigned need = 0, fast = 0;
                        double y[4], cf[CK_TAB_DEG + 1][4];
                        const double* lp[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rr = min(r0 + r, nac - 1);
                            const int a = ac + r0 + r;
                            const double dx = au[0][rr] - b0, dy = au[1][rr] - b1, dz = au[2][rr] - b2;
                            int iv;
                            y[r] = ck_table_y(dx * dx + dy * dy + dz * dz, &iv, tbase);
                            const bool in = r < nr && b <= a, hit = (unsigned)iv < (unsigned)tn;
                            fast |= (in && hit) ? 1u << r : 0u;
                            need |= (in && !hit) ? 1u << r : 0u;
                            lp[r] = tab + min(max(iv, 0), max(tn - 1, 0));   // keep the lookup inside the table
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kk = CK_TAB_DEG; kk >= 0; --kk)
#pragma unroll
                            for (int r = 0; r < 4; ++r) cf[kk][r] = lp[r][kk * CK_TAB_STRIDE];
                        __builtin_amdgcn_sched_barrier(0);
                        double pv[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) pv[r] = cf[CK_TAB_DEG][r];
#pragma unroll
                        for (int kk = CK_TAB_DEG - 1; kk >= 0; --kk)
#pragma unroll
                            for (int r = 0; r < 4; ++r) pv[r] = fma(pv[r], y[r], cf[kk][r]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int a = ac + r0 + r;
                            if (fast >> r & 1u)
                                S[(long)a * ld + b] = pv[r];
                            else if ((need >> r & 1u) && b == a) {   // one per row: kept out of the slow loop below
                                S[(long)a * ld + b] = cdiag;
                                need &= ~(1u << r);
                            }
                        }
                        if (need) {
#pragma unroll 1
                            for (int r = 0; r < 4; ++r)
                                if (need >> r & 1u) {
                                    const int a = ac + r0 + r;
                                    const int slot = atomicAdd(&wl_n, 1);
                                    if (slot < LT_WL) {
                                        wl[slot] = make_int2(a, b);
                                    } else {   // list full: in place
                                        S[(long)a * ld + b] = lp_exact_pair(&blk[reg], metric, nug, s0, s1, s2, idx[a], idx[b]);
                                    }
                                }
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int nw = min(wl_n, LT_WL);
        for (int e = tid; e < nw; e += LT_TPB) {
            const int a = wl[e].x, b = wl[e].y;
            S[(long)a * ld + b] = lp_exact_pair(&blk[reg], metric, nug, s0, s1, s2, idx[a], idx[b]);
        }
        if (nz && reg != 1) {   // measurement-error variances (ck_set_noise) on the diagonal of this launch's region
            __syncthreads();
            for (int a = alo + tid; a < ahi; a += LT_TPB) S[(long)a * ld + a] += nz[idx[a]];
        }
    }
}

// pred = v . y, var = c0 - v . v from the two solved rows
__global__ __launch_bounds__(LP_TPB) void k_local_reduce_t(const CkLocalSys* __restrict__ sys, const double* __restrict__ slab,
                                                            const long long* __restrict__ info, double c0var,
                                                            double* __restrict__ pred, double* __restrict__ err,
                                                            double* __restrict__ vv, const double* __restrict__ sbb) {
    const int tid = threadIdx.x;
    const CkLocalSys q = sys[blockIdx.x];
    if (info[blockIdx.x] != 0) {
        if (tid == 0) lp_write_nan(q.p, pred, err);
        return;
    }
    const double* v = slab + q.off + (long)(q.kq - 2) * q.ld;
    double vy, v2;
    lp_dots(v, v + q.ld, q.k, &vy, &v2);
    if (tid == 0) lp_write(q.p, vy, v2, sbb ? sbb[q.p] : c0var, pred, err, vv);
}

// the pair form: the five outputs from the three solved rows kq - 3 (v0), kq - 2 (v1), kq - 1 (y)
__global__ __launch_bounds__(LP_TPB) void k_local_reduce_pair_t(const CkLocalSys* __restrict__ sys, const double* __restrict__ slab,
                                                                 const long long* __restrict__ info, CkLocalPairOut O) {
    const CkLocalSys q = sys[blockIdx.x];
    if (info[blockIdx.x] != 0) {
        if (threadIdx.x == 0) lp_write_pair_nan(O, q.p);
        return;
    }
    const double* v0 = slab + q.off + (long)(q.kq - 3) * q.ld;
    lp_write_pair(O, q.p, v0, v0 + q.ld, v0 + 2 * (long)q.ld, q.k);
}

void ck_launch_local_assemble_t(hipStream_t s, const CkLocalProblem& P, const CkLocalSys* sys, int n_sys, double* slab,
                                int* k0buf, bool pair) {
    if (n_sys <= 0) return;
    if (pair)
        k_local_search_t<false, true><<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(P, sys, slab, k0buf);
    else if (P.bo)
        k_local_search_t<true, false><<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(P, sys, slab, k0buf);
    else
        k_local_search_t<false, false><<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(P, sys, slab, k0buf);
    const LpTab T{P.tabs, P.coefs, P.use_tab};
    const int nreg = P.L.nend > P.L.n0p ? 3 : 1;           // a second process?
    const int grid = n_sys < 512 ? n_sys : 512;            // two workgroups per CU; they walk over the systems
    for (int reg = 0; reg < nreg; ++reg)
        k_local_assemble_t<<<dim3((unsigned)grid), dim3(LT_TPB), 0, s>>>(P.blk, P.metric, reg, P.sc, P.L, sys, n_sys, slab, T, P.su,
                                                                         k0buf, P.nz);
}

void ck_launch_local_reduce_t(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab,
                              const long long* info, double c0var, double* pred, double* err, double* vv, const double* sbb) {
    if (n_sys <= 0) return;
    k_local_reduce_t<<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(sys, slab, info, c0var, pred, err, vv, sbb);
}

void ck_launch_local_reduce_pair_t(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab, const long long* info,
                                   const CkLocalPairOut& O) {
    if (n_sys <= 0) return;
    k_local_reduce_pair_t<<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(sys, slab, info, O);
}

int ck_local_lds_limit() { return LP_KL; }

// ---------------------------------------------------------------------------------------
// universal cokriging in the neighbourhood (ck_predict_local_universal; include/cokrige.h has the rules)
// ---------------------------------------------------------------------------------------
// The p trend rows X_loc^T ride along the factorisation as c and z do: behind it they hold U^T = (L^-1 X_loc)^T.  Every
// kernel then forms the Gram matrix G of the nx = 2 + p solved rows [v; y; U_0 .. U_{p-1}] -- one thread per entry, each a
// sequential sum over the neighbours: a fixed order, no atomics -- and one thread runs the GLS step (ck_local_gls.h) on it:
//   G[0][0] = v.v, G[1][0] = v.y, G[2 + j][0] = (U^T v)_j, G[2 + j][1] = b_j, G[2 + j][2 + l] = A_jl.
// Work area E (LDS): G nx nx | W p p + 2 p | bb p | rr p | bl p doubles.
#include "ck_local_gls.h"

#define LU_EXTRA(p) (((p) + 2) * ((p) + 2) + (p) * (p) + 5 * (p))
#define LU_NPAIR(nx) ((nx) * ((nx) + 1) / 2)

__device__ __forceinline__ void lu_fill_nan(long p, int np, double* __restrict__ pred, double* __restrict__ err,
                                            double* __restrict__ beta, int* __restrict__ status, int code) {
    pred[p] = NAN;
    err[p] = NAN;
    status[p] = code;
    if (beta)
        for (int j = 0; j < np; ++j) beta[p * np + j] = NAN;
}

// entry e of the lower triangle -> (r, c), r >= c (e < 171: exact in the few steps below)
__device__ __forceinline__ void lu_pair(int e, int* r, int* c) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    *r = a;
    *c = e - a * (a + 1) / 2;
}

// one thread: r = x0 - U^T v, the GLS step, the outputs of point p
__device__ __forceinline__ void lu_finish(double* E, CkLocalTrend Tr, int i_pred, int k0, int k1, long p, double c0var,
                                          double* __restrict__ pred, double* __restrict__ err, double* __restrict__ beta,
                                          int* __restrict__ status) {
    const int np = Tr.p0 + Tr.p1, nx = np + 2;
    double *G = E, *W = G + nx * nx, *bb = W + np * np + 2 * np, *rr = bb + np, *bl = rr + np;
    const int pi = i_pred == 0 ? Tr.p0 : Tr.p1, offi = i_pred == 0 ? 0 : Tr.p0;
    for (int j = 0; j < np; ++j) {
        bb[j] = G[(2 + j) * nx + 1];
        const double x0 = (j >= offi && j < offi + pi) ? Tr.f0[p * pi + (j - offi)] : 0.0;
        rr[j] = x0 - G[(2 + j) * nx];
    }
    double rb, rar;
    if (ck_local_gls(Tr.p0, Tr.p1, k0, k1, i_pred, G + 2 * nx + 2, nx, bb, rr, Tr.tol, W, bl, &rb, &rar) != CK_LG_OK) {
        lu_fill_nan(p, np, pred, err, beta, status, CK_LU_RANK_DEF);
        return;
    }
    pred[p] = G[nx] + rb;
    const double sd = sqrt(c0var - G[0] + rar);
    err[p] = (sd == sd) ? fmax(sd, 0.0) : 0.0;
    status[p] = CK_LU_OK;
    if (beta)
        for (int j = 0; j < np; ++j) beta[p * np + j] = bl[j];
}

// the Gram matrix G of the nx solved rows behind a k x k factor in LDS (rows k .. k + nx - 1 of S) into E: one thread per entry of
// the lower triangle, each a sequential sum over the neighbours; ends with a barrier
__device__ __forceinline__ void lu_gram(const double* S, long ld, int k, int nx, double* E) {
    const int tid = threadIdx.x;
    if (tid < LU_NPAIR(nx)) {
        int r, c;
        lu_pair(tid, &r, &c);
        const double *xr = S + (long)(k + r) * ld, *xc = S + (long)(k + c) * ld;
        double acc = 0.0;
        for (int a = 0; a < k; ++a) acc += xr[a] * xc[a];
        E[r * nx + c] = acc;
    }
    __syncthreads();
}

// LDS class: k_local_solve with k + 2 + p rows (c, z, then the trend rows); dynamic LDS sized by p
__global__ __launch_bounds__(LP_TPB) void k_local_solve_u(CkLocalProblem P, const int* __restrict__ counts, int k_hi,
                                                           CkLocalTrend Tr, double* __restrict__ pred, double* __restrict__ err,
                                                           double* __restrict__ beta, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lu_lds[];   // (LP_KL + nx) x LP_KL matrix | LU_EXTRA(p)
    __shared__ int idx[LP_KL];
    const int tid = threadIdx.x;
    const int np = Tr.p0 + Tr.p1, nx = np + 2;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k == 0) {
        if (tid == 0) lu_fill_nan(p, np, pred, err, beta, status, CK_LU_EMPTY);
        return;
    }
    if (k > LP_KL || k > k_hi) return;   // the tiled path
    double* S = lu_lds;
    double* E = lu_lds + (LP_KL + nx) * LP_KL;
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    int k0;                                    // 1. neighbour list; k0 = neighbours of process 0
    lp_compact<true, 0>(P, X, idx, &k0);
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, trend rows, noise
    lp_cz_rows(P, X, idx, S, ld, k);
    for (int e = tid; e < np * k; e += LP_TPB) {
        const int j = e / k, a = e - j * k;
        S[(long)(k + 2 + j) * ld + a] = Tr.X[(long)j * P.L.npad + idx[a]];
    }
    lp_noise(P, idx, S, ld, k);
    if (!lp_chol(S, ld, k, nx)) {              // 3. Cholesky, the nx extra rows ride along
        if (tid == 0) lu_fill_nan(p, np, pred, err, beta, status, CK_LU_NOT_PD);
        return;
    }
    lu_gram(S, ld, k, nx, E);                  // 4. Gram matrix of the solved rows, then the GLS step
    if (tid == 0) lu_finish(E, Tr, P.i_pred, k0, k - k0, p, P.c0var, pred, err, beta, status);
}

void ck_launch_local_solve_u(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, int k_hi, CkLocalTrend Tr,
                             double* pred, double* err, double* beta, int* status) {
    if (m <= 0) return;
    const int np = Tr.p0 + Tr.p1;
    const size_t lds = (size_t)((LP_KL + 2 + np) * LP_KL + LU_EXTRA(np)) * sizeof(double);   // 34.9 KB (p = 2) .. 47.2 KB (p = 16)
    k_local_solve_u<<<dim3((unsigned)m), dim3(LP_TPB), lds, s>>>(P, counts, k_hi, Tr, pred, err, beta, status);
}

// Block cokriging, LDS class (ck_predict_local_blocks): k_local_solve_u's steps for block p -- the neighbourhood of its centre,
// then the same local system -- with row k holding cbar (lp_cbar_z_rows) and P.sbb[p] in place of c0var.  No trend (np == 0):
// k_local_solve's step 4, its tree and its outputs (status may be null).
__global__ __launch_bounds__(LP_TPB) void k_local_solve_b(CkLocalProblem P, const int* __restrict__ counts, int k_hi,
                                                           CkLocalTrend Tr, double* __restrict__ pred, double* __restrict__ err,
                                                           double* __restrict__ beta, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lu_lds[];   // (LP_KL + nx) x LP_KL matrix | LU_EXTRA(p)
    __shared__ int idx[LP_KL];
    __shared__ double part[LP_TPB];
    const int tid = threadIdx.x;
    const int np = Tr.p0 + Tr.p1, nx = np + 2;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k == 0) {
        if (tid == 0) {
            if (np) lu_fill_nan(p, np, pred, err, beta, status, CK_LU_EMPTY);
            else lp_write_nan(p, pred, err);
        }
        return;
    }
    if (k > LP_KL || k > k_hi) return;   // the tiled path
    double* S = lu_lds;
    double* E = lu_lds + (LP_KL + nx) * LP_KL;
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);          // the block's centre
    int k0;                                    // 1. neighbour list; k0 = neighbours of process 0
    lp_compact<true, 0>(P, X, idx, &k0);
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, cbar row, z row, trend rows, noise
    lp_cbar_z_rows(P, X, p, idx, S, ld, k, part);
    for (int e = tid; e < np * k; e += LP_TPB) {
        const int j = e / k, a = e - j * k;
        S[(long)(k + 2 + j) * ld + a] = Tr.X[(long)j * P.L.npad + idx[a]];
    }
    lp_noise(P, idx, S, ld, k);
    if (!lp_chol(S, ld, k, nx)) {              // 3. Cholesky, the nx extra rows ride along
        if (tid == 0) {
            if (np) lu_fill_nan(p, np, pred, err, beta, status, CK_LU_NOT_PD);
            else lp_write_nan(p, pred, err);
        }
        return;
    }
    if (np == 0) {                             // 4. simple cokriging: pred = v . y, var = sigma_BB - v . v
        double vy, v2;
        lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &vy, &v2);
        if (tid == 0) lp_write(p, vy, v2, P.sbb[p], pred, err, nullptr);
        return;
    }
    lu_gram(S, ld, k, nx, E);                  // 4. Gram matrix of the solved rows, then the GLS step
    if (tid == 0) lu_finish(E, Tr, P.i_pred, k0, k - k0, p, P.sbb[p], pred, err, beta, status);
}

void ck_launch_local_solve_b(hipStream_t s, const CkLocalProblem& P, int64_t r, const int* counts, int k_hi, CkLocalTrend Tr,
                             double* pred, double* err, double* beta, int* status) {
    if (r <= 0) return;
    const int np = Tr.p0 + Tr.p1;
    const size_t lds = (size_t)((LP_KL + 2 + np) * LP_KL + LU_EXTRA(np)) * sizeof(double);   // k_local_solve_u's, + 2 KB of partials
    k_local_solve_b<<<dim3((unsigned)r), dim3(LP_TPB), lds, s>>>(P, counts, k_hi, Tr, pred, err, beta, status);
}

// Tiled class: behind k_local_search_t (which has written identity rows up to kq - 2) the p rows [kq - 2 - p, kq - 2)
// become the trend rows -- X_loc^T in the columns [0, k), CK_LT_BIG on the diagonal, the zeros in between stay
__global__ __launch_bounds__(LP_TPB) void k_local_trend_rows_t(const CkLocalSys* __restrict__ sys, double* __restrict__ slab,
                                                                CkLayout L, CkLocalTrend Tr) {
    const CkLocalSys q = sys[blockIdx.x];
    const int np = Tr.p0 + Tr.p1, t0 = q.kq - 2 - np;
    double* S = slab + q.off;
    const int* idx = reinterpret_cast<const int*>(S + (long)CK_LT_ROWS(q.kq) * q.ld + CK_LT_NINV * 64 * 64);
    for (int j = 0; j < np; ++j) {
        double* row = S + (long)(t0 + j) * q.ld;
        for (int a = threadIdx.x; a < q.k; a += LP_TPB) row[a] = Tr.X[(long)j * L.npad + idx[a]];
        if (threadIdx.x == 0) row[t0 + j] = CK_LT_BIG;
    }
}

// the solved rows dotted with [y; U] (64 columns at a time through LDS), then the GLS step
__global__ __launch_bounds__(LP_TPB) void k_local_reduce_ut(const CkLocalSys* __restrict__ sys, const double* __restrict__ slab,
                                                             const long long* __restrict__ info, const int* __restrict__ k0in,
                                                             int i_pred, double c0var, double* __restrict__ pred,
                                                             double* __restrict__ err, CkLocalTrend Tr, double* __restrict__ beta,
                                                             int* __restrict__ status, const double* __restrict__ sbb) {
    __shared__ double tile[2 + CK_LU_PMAX][65];
    __shared__ double E[LU_EXTRA(CK_LU_PMAX)];
    const int tid = threadIdx.x;
    const int np = Tr.p0 + Tr.p1, nx = np + 2;
    const CkLocalSys q = sys[blockIdx.x];
    if (info[blockIdx.x] != 0) {
        if (tid == 0) lu_fill_nan(q.p, np, pred, err, beta, status, CK_LU_NOT_PD);
        return;
    }
    const double* S = slab + q.off;
    int r = 0, c = 0;
    if (tid < LU_NPAIR(nx)) lu_pair(tid, &r, &c);
    double acc = 0.0;
    for (int a0 = 0; a0 < q.k; a0 += 64) {
        const int na = min(64, q.k - a0);
        __syncthreads();
        for (int e = tid; e < nx * 64; e += LP_TPB) {
            const int rr = e >> 6, a = e & 63;
            // row 0: v (kq - 2), row 1: y (kq - 1), rows 2 ..: the trend rows
            const int row = rr < 2 ? q.kq - 2 + rr : q.kq - 2 - np + (rr - 2);
            tile[rr][a] = a < na ? S[(long)row * q.ld + a0 + a] : 0.0;
        }
        __syncthreads();
        if (tid < LU_NPAIR(nx))
            for (int a = 0; a < na; ++a) acc += tile[r][a] * tile[c][a];
    }
    if (tid < LU_NPAIR(nx)) E[r * nx + c] = acc;
    __syncthreads();
    if (tid == 0) {
        const int k0 = k0in[blockIdx.x];
        lu_finish(E, Tr, i_pred, k0, q.k - k0, q.p, sbb ? sbb[q.p] : c0var, pred, err, beta, status);
    }
}

void ck_launch_local_trend_rows_t(hipStream_t s, const CkLocalSys* sys, int n_sys, double* slab, CkLayout L, CkLocalTrend Tr) {
    if (n_sys <= 0) return;
    k_local_trend_rows_t<<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(sys, slab, L, Tr);
}

void ck_launch_local_reduce_ut(hipStream_t s, const CkLocalSys* sys, int n_sys, const double* slab, const long long* info,
                               const int* k0buf, int i_pred, double c0var, double* pred, double* err, CkLocalTrend Tr, double* beta,
                               int* status, const double* sbb) {
    if (n_sys <= 0) return;
    k_local_reduce_ut<<<dim3((unsigned)n_sys), dim3(LP_TPB), 0, s>>>(sys, slab, info, k0buf, i_pred, c0var, pred, err, Tr, beta,
                                                                     status, sbb);
}

// ---------------------------------------------------------------------------------------
// the Vecchia likelihood's terms (ck_loglik_vecchia; include/cokrige.h has the definition, ck_vecchia.h a term's arithmetic)
// ---------------------------------------------------------------------------------------
// k_vecchia_terms: one thread per datum, in the caller's stacked order; a workgroup's LP_TPB terms are summed by a fixed tree
// in LDS into part[2 b], part[2 b + 1], and bad[b] = 1 + the smallest index of a datum without a term (0: none).
// k_vecchia_sum (one workgroup): thread t adds the partial sums t, t + LP_TPB, .. in that order, the same tree finishes.
// No atomics, no dependence on the launch: repeated calls give the same bits.
#include "ck_vecchia.h"

// the tree of both kernels: (lv, qd) summed, b = the smallest non-zero; thread 0 writes out2[0], out2[1], *outb
__device__ __forceinline__ void vt_tree(double lv, double qd, long long b, double* out2, long long* outb) {
    __shared__ double red[2][LP_TPB];
    __shared__ long long first[LP_TPB];
    const int tid = threadIdx.x;
    red[0][tid] = lv;
    red[1][tid] = qd;
    first[tid] = b;
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            const long long o = first[tid + s];
            if (o != 0 && (first[tid] == 0 || o < first[tid])) first[tid] = o;
        }
        __syncthreads();
    }
    if (tid == 0) {
        out2[0] = red[0][0];
        out2[1] = red[1][0];
        *outb = first[0];
    }
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_terms(long n, const double* __restrict__ z, const double* __restrict__ mu,
                                                           const double* __restrict__ vv, const double* __restrict__ prior,
                                                           const double* __restrict__ noise, const int* __restrict__ cnt2,
                                                           double* __restrict__ mean, double* __restrict__ var,
                                                           double* __restrict__ part, long long* __restrict__ bad) {
    const long t = (long)blockIdx.x * LP_TPB + threadIdx.x;
    double lv = 0.0, qd = 0.0;
    long long b = 0;
    if (t < n) {
        double m, s2;
        if (ck_vecchia_term(z[t], mu[t], vv[t], prior[t], noise ? noise[t] : 0.0, cnt2[2 * t] + cnt2[2 * t + 1], &m, &s2, &lv, &qd))
            b = t + 1;
        mean[t] = m;
        var[t] = s2;
    }
    vt_tree(lv, qd, b, part + 2 * blockIdx.x, bad + blockIdx.x);
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_sum(long nblk, const double* __restrict__ part, const long long* __restrict__ bad,
                                                         double* __restrict__ out2, long long* __restrict__ info) {
    double lv = 0.0, qd = 0.0;
    long long b = 0;
    for (long e = threadIdx.x; e < nblk; e += LP_TPB) {
        lv += part[2 * e];
        qd += part[2 * e + 1];
        if (b == 0) b = bad[e];   // the blocks come in ascending order of their data
    }
    vt_tree(lv, qd, b, out2, info);
}

void ck_launch_vecchia_terms(hipStream_t s, int64_t n, const double* z, const double* mu, const double* vv, const double* prior,
                             const double* noise, const int* cnt2, double* mean, double* var, double* part, long long* bad,
                             double* out2, long long* info) {
    if (n <= 0) return;
    const long nblk = (long)((n + LP_TPB - 1) / LP_TPB);
    k_vecchia_terms<<<dim3((unsigned)nblk), dim3(LP_TPB), 0, s>>>((long)n, z, mu, vv, prior, noise, cnt2, mean, var, part, bad);
    k_vecchia_sum<<<dim3(1), dim3(LP_TPB), 0, s>>>(nblk, part, bad, out2, info);
}

// ---------------------------------------------------------------------------------------
// the gradient of the Vecchia likelihood (ck_loglik_vecchia_grad; ck_vecchia_grad.h has the formula and the pair rule)
// ---------------------------------------------------------------------------------------
// k_vecchia_grad: one workgroup per datum, sets of at most LP_KL data.  Steps 1 - 4 are k_local_solve's: the same
// calls of the same device functions with the same arguments, so mu and v . v come out with the same bits (the one difference:
// the neighbour list is written under the capacity guard of lp_compact, which never drops an entry here); then
//   5. back substitution in place on rows k and k + 1: v -> w = L^-T v, y -> alpha = L^-T y (vg_back_substitute, shared with
//      k_vecchia_info).  ONE wave, lane a holding x_a of
//      both rows: step j broadcasts x_j / L_jj from lane j and every lane a < j subtracts L[j][a] x_j -- row j of L is
//      contiguous in LDS, and with k <= 64 the whole vector lives in one wave, so the k dependent steps need no barrier
//      (a barrier per step across four waves would cost more than the three waves add: a step has at most 64 updates);
//   6. the contraction over the lower triangle of the set plus the datum, (k + 1)(k + 2) / 2 pairs over the 256 threads,
//      ck_vecchia_pair per pair with the exact evaluator's derivatives; 13 sums per thread, reduced by wave shuffles and a
//      fixed four-wave order (k_loglik_grad's), one 13-vector per datum.
// An empty set is the one-entry system (b = 1, a = 0): it runs step 6 alone.  A system that is not positive definite or a
// variance that is not > 0: NaN in the live slots.  k_vecchia_grad_part / _sum: the column sums of the scores by vg_tree,
// the 13-column form of the terms' tree and partial-sum order.  No atomics: repeated calls give the same bits.

// step 5 of both kernels: rows k, k + 1 of S become b = -L^-T v and alpha = L^-T y; ends with a barrier
__device__ __forceinline__ void vg_back_substitute(double* S, long ld, int k) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (wv == 0 && k > 0) {
        double xv = lane < k ? S[(long)k * ld + lane] : 0.0, xy = lane < k ? S[(long)(k + 1) * ld + lane] : 0.0;
        for (int j = k - 1; j >= 0; --j) {
            const double dj = S[(long)j * ld + j];
            const double lj = lane < j ? S[(long)j * ld + lane] : 0.0;
            const double vj = __shfl(xv, j) / dj, yj = __shfl(xy, j) / dj;
            if (lane == j) {
                xv = vj;
                xy = yj;
            } else if (lane < j) {
                xv -= lj * vj;
                xy -= lj * yj;
            }
        }
        if (lane < k) {
            S[(long)k * ld + lane] = -xv;
            S[(long)(k + 1) * ld + lane] = xy;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_grad(CkLocalProblem P, const int* __restrict__ counts,
                                                          double* __restrict__ pred, double* __restrict__ err,
                                                          double* __restrict__ vv, CkVecchiaGradArgs A) {
    __shared__ double S[(LP_KL + 2) * LP_KL];
    __shared__ int idx[LP_KL];
    __shared__ double sred[LP_TPB / 64][CK_VG_NPAR];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k > LP_KL) return;   // refused by the host before any launch
    const CkVecchiaModel& V = A.V;
    double* score = A.score + p * CK_VG_NPAR;
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    bool ok = true;
    if (k > 0) {
        lp_compact<false, LP_KL>(P, X, idx);       // 1. neighbour list (the count is the select pass's: never beyond k)
        lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, noise
        lp_cz_rows(P, X, idx, S, ld, k);
        lp_noise(P, idx, S, ld, k);
        ok = lp_chol(S, ld, k, 2);                 // 3. Cholesky, the two extra rows ride along
    }
    double mu = 0.0, vvs = 0.0;
    if (!ok || k == 0) {   // no solve: k_local_solve's outputs for these points
        if (tid == 0) lp_write_nan(p, pred, err);
        if (!ok) {
            if (tid < CK_VG_NPAR) score[tid] = ck_vecchia_slot_out(V, tid, 0.0, 1);
            return;
        }
    } else {
        lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &mu, &vvs);   // 4. pred = v . y, var = c0 - v . v
        if (tid == 0) lp_write(p, mu, vvs, P.c0var, pred, err, vv);
    }
    // ---- the two weights of M ----
    const long gs = A.gself[p];
    double w_bb, w_ab;
    const int bad = ck_vecchia_weights(P.z[gs], mu, vvs, P.c0var, P.nz ? P.nz[gs] : 0.0, k, &w_bb, &w_ab);
    if (bad) {   // uniform
        if (tid < CK_VG_NPAR) score[tid] = ck_vecchia_slot_out(V, tid, 0.0, 1);
        return;
    }
    vg_back_substitute(S, ld, k);                  // 5. rows k, k + 1 become b = -w and a = alpha
    // ---- 6. the contraction over the lower triangle of the set plus the datum ----
    double acc[CK_VG_NPAR];
#pragma unroll
    for (int c = 0; c < CK_VG_NPAR; ++c) acc[c] = 0.0;
    const long npair1 = (long)(k + 1) * (k + 2) / 2;
    for (long e = tid; e < npair1; e += LP_TPB) {
        int a, b;
        ck_vg_pair_of(e, &a, &b);
        const long ga = a < k ? idx[a] : gs, gb = b < k ? idx[b] : gs;
        const int pa = a < k ? (V.n_procs == 2 && ga >= P.L.n0p ? 1 : 0) : P.i_pred;
        const int pb = b < k ? (V.n_procs == 2 && gb >= P.L.n0p ? 1 : 0) : P.i_pred;
        const double a0 = a < k ? X.s0[ga] : X.p0, a1 = a < k ? X.s1[ga] : X.p1, a2 = a < k ? X.s2[ga] : X.p2;
        const double b0 = b < k ? X.s0[gb] : X.p0, b1 = b < k ? X.s1[gb] : X.p1, b2 = b < k ? X.s2[gb] : X.p2;
        const double ba = a < k ? S[(long)k * ld + a] : 1.0, aa = a < k ? S[(long)(k + 1) * ld + a] : 0.0;
        const double bb = b < k ? S[(long)k * ld + b] : 1.0, ab = b < k ? S[(long)(k + 1) * ld + b] : 0.0;
        const double h = a == b ? 0.0 : lp_dist(P.metric, a0, a1, a2, b0, b1, b2);
        const double d_p = (a == b && A.dvar) ? A.dvar[ga] : 0.0;
        ck_vecchia_pair(acc, V, pa, pb, a == b, h, ck_vecchia_m(w_bb, w_ab, ba, aa, bb, ab), d_p);
    }
#pragma unroll
    for (int c = 0; c < CK_VG_NPAR; ++c) {
        double v = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        acc[c] = v;
    }
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < CK_VG_NPAR; ++c) sred[wv][c] = acc[c];
    __syncthreads();
    if (tid < CK_VG_NPAR) score[tid] = ck_vecchia_slot_out(V, tid, ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid], 0);
}

// the tree of both kernels: column(c) is this thread's entry of column c; threads 0 .. 12 write the column sums to out
template <class F>
__device__ __forceinline__ void vg_tree(F column, double* out) {
    __shared__ double red[CK_VG_NPAR][LP_TPB];
    const int tid = threadIdx.x;
    for (int c = 0; c < CK_VG_NPAR; ++c) red[c][tid] = column(c);
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int c = 0; c < CK_VG_NPAR; ++c) red[c][tid] += red[c][tid + s];
        __syncthreads();
    }
    if (tid < CK_VG_NPAR) out[tid] = red[tid][0];
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_grad_part(long n, const double* __restrict__ score, double* __restrict__ part) {
    const long t = (long)blockIdx.x * LP_TPB + threadIdx.x;
    vg_tree([&](int c) { return t < n ? score[t * CK_VG_NPAR + c] : 0.0; }, part + (long)blockIdx.x * CK_VG_NPAR);
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_grad_sum(long nblk, const double* __restrict__ part, double* __restrict__ out13) {
    vg_tree(
        [&](int c) {
            double v = 0.0;
            for (long e = threadIdx.x; e < nblk; e += LP_TPB) v += part[e * CK_VG_NPAR + c];
            return v;
        },
        out13);
}

void ck_launch_vecchia_grad(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, double* pred, double* err,
                            double* vv, CkVecchiaGradArgs A) {
    if (m <= 0) return;
    k_vecchia_grad<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts, pred, err, vv, A);
}

void ck_launch_vecchia_grad_sum(hipStream_t s, int64_t n, const double* score, double* part, double* out13) {
    if (n <= 0) return;
    const long nblk = (long)((n + LP_TPB - 1) / LP_TPB);
    k_vecchia_grad_part<<<dim3((unsigned)nblk), dim3(LP_TPB), 0, s>>>((long)n, score, part);
    k_vecchia_grad_sum<<<dim3(1), dim3(LP_TPB), 0, s>>>(nblk, part, out13);
}

// ---------------------------------------------------------------------------------------
// the expected information of the Vecchia likelihood (ck_loglik_vecchia_fisher; ck_vecchia_info.h has the formula and the rules)
// ---------------------------------------------------------------------------------------
// k_vecchia_info: a workgroup takes VI_RUN consecutive data of a process, one after the other, sets of at most LP_KL data.  Per
// datum, steps 1 - 5 are k_vecchia_grad's: the same calls of the same device functions with the same arguments (the z row rides
// along unused), so L, v . v and b = -w are that kernel's.  Then
//   5'. L is mirrored into the unused upper triangle of S, S[j][a] = L[a][j] for a > j, along diagonals (lane l moves entry
//       (l + d, l): reads and writes both walk the banks), so that COLUMN j of L is the contiguous tail of row j;
//   6'. the product U = D b over the full square of the set plus the datum: row a belongs to VI_T = 16 consecutive lanes, lane
//       `sub` of them takes the entries q = sub, sub + 16, .. through ck_vecchia_info_entry (ck_vecchia_pair itself) into 13
//       sums, xor-shuffles over the 16 lanes add them in a fixed order and lane 0 writes U[slot][a]: no two threads add to one
//       element, 16 rows per pass;
//   7'. q_slot = b . U[slot] (a wave reduction) and the forward substitution Y = L^-1 U[., 0 : k], wave w taking the slots w,
//       w + 4, w + 8, w + 12: lane a holds entry a of its (up to four) right-hand sides, step j broadcasts x_j / L_jj from
//       lane j and every lane a > j subtracts L[a][j] x_j, read from the mirrored copy -- the column form of step 5, no barrier
//       and no reduction inside the k dependent steps, no bank conflict (a column walk on L itself puts all lanes on one bank);
//   8'. thread e < 91 adds ck_vecchia_info_combine(y_j . y_k, q_j, q_k, s2) of its pair (j, k) to its running sum.
// The workgroup writes its 91 sums to one row of `part` and 1 + the first of its data without a term (0: none) to `bad`: N / VI_RUN
// rows, whatever the device.  k_vecchia_info_part / _sum: the column sums of the rows by vg_tree, 13 columns per workgroup
// (blockIdx.y / blockIdx.x = the group of columns), in the partial-sum order of the scores.  No atomics: repeated calls give the
// same bits.
#define VI_RUN 8   // consecutive data per workgroup: a constant of the reduction's layout
#define VI_T 16    // lanes per row of the product
static_assert(CK_VI_NTRI % CK_VG_NPAR == 0 && CK_VI_NTRI <= LP_TPB, "91 = 7 groups of vg_tree's 13 columns, one thread per sum");
static_assert(LP_KL <= 64, "the set's vector lives in one wave");

__global__ __launch_bounds__(LP_TPB) void k_vecchia_info(CkLocalProblem P, const int* __restrict__ counts, long m,
                                                          CkVecchiaInfoArgs A) {
    __shared__ double S[(LP_KL + 2) * LP_KL];
    __shared__ int idx[LP_KL];
    __shared__ double U[CK_VI_NPAR][LP_KL + 2];
    __shared__ double qv[CK_VI_NPAR];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CkVecchiaModel& V = A.V;
    const long ld = LP_KL;
    int je = 0, ke = 0;   // this thread's pair of slots (tid < 91)
    if (tid < CK_VI_NTRI) ck_vg_pair_of(tid, &je, &ke);
    double sum = 0.0;
    long long first_bad = 0;
    for (int r = 0; r < VI_RUN; ++r) {
        const long p = (long)blockIdx.x * VI_RUN + r;
        if (p >= m) break;     // uniform
        __syncthreads();       // the previous datum's reads of S, U and qv are done
        const int k = counts[p];
        if (k > LP_KL) continue;   // refused by the host before any launch
        const LpPoint X = lp_point(P, p);
        bool ok = true;
        if (k > 0) {
            lp_compact<false, LP_KL>(P, X, idx);       // 1. neighbour list (the count is the select pass's: never beyond k)
            lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, noise
            lp_cz_rows(P, X, idx, S, ld, k);
            lp_noise(P, idx, S, ld, k);
            ok = lp_chol(S, ld, k, 2);                 // 3. Cholesky, the two extra rows ride along
        }
        double mu = 0.0, vvs = 0.0, s2 = 0.0;
        if (ok && k > 0) lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &mu, &vvs);   // 4. v . v
        const long gs = A.gself[p];
        if (!ok || ck_vecchia_info_var(P.z[gs], mu, vvs, P.c0var, P.nz ? P.nz[gs] : 0.0, k, &s2)) {   // uniform
            if (first_bad == 0) first_bad = A.stacked0 + p + 1;
            continue;
        }
        vg_back_substitute(S, ld, k);                  // 5. row k becomes b = -w
        // ---- 5'. the mirror of L ----
        for (int d = 1 + wv; d < k; d += LP_TPB / 64) {
            const int a = lane + d;
            if (a < k) S[(long)lane * ld + a] = S[(long)a * ld + lane];
        }
        // ---- 6'. U = D b ----
        const int n1 = k + 1;
        for (int a0 = 0; a0 < n1; a0 += LP_TPB / VI_T) {
            const int a = a0 + tid / VI_T, sub = tid % VI_T;
            double row[CK_VI_NPAR];
#pragma unroll
            for (int c = 0; c < CK_VI_NPAR; ++c) row[c] = 0.0;
            if (a < n1) {
                const long ga = a < k ? idx[a] : gs;
                const int pa = a < k ? (V.n_procs == 2 && ga >= P.L.n0p ? 1 : 0) : P.i_pred;
                const double a0c = a < k ? X.s0[ga] : X.p0, a1c = a < k ? X.s1[ga] : X.p1, a2c = a < k ? X.s2[ga] : X.p2;
                const double d_a = A.dvar ? A.dvar[ga] : 0.0;
                for (int q = sub; q < n1; q += VI_T) {
                    const long gq = q < k ? idx[q] : gs;
                    const int pq = q < k ? (V.n_procs == 2 && gq >= P.L.n0p ? 1 : 0) : P.i_pred;
                    const double q0 = q < k ? X.s0[gq] : X.p0, q1 = q < k ? X.s1[gq] : X.p1, q2 = q < k ? X.s2[gq] : X.p2;
                    const double bq = q < k ? S[(long)k * ld + q] : 1.0;
                    const double h = a == q ? 0.0 : lp_dist(P.metric, a0c, a1c, a2c, q0, q1, q2);
                    ck_vecchia_info_entry(row, V, pa, pq, a == q, h, bq, a == q ? d_a : 0.0);
                }
            }
#pragma unroll
            for (int c = 0; c < CK_VI_NPAR; ++c) {
                double v = row[c];
#pragma unroll
                for (int off = VI_T / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (a < n1 && sub == 0) U[c][a] = v;
            }
        }
        __syncthreads();
        // ---- 7'. q = b . U and Y = L^-1 U[., 0 : k], in place ----
        {
            const double bl = lane < k ? S[(long)k * ld + lane] : 0.0;
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int s = wv + 4 * i;
                x[i] = (s < CK_VI_NPAR && lane < k) ? U[s < CK_VI_NPAR ? s : 0][lane] : 0.0;
                double v = x[i] * bl;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (s < CK_VI_NPAR && lane == 0) qv[s] = v + U[s][k];
            }
            for (int j = 0; j < k; ++j) {
                const double dj = S[(long)j * ld + j];
                const double lj = (lane > j && lane < k) ? S[(long)j * ld + lane] : 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double xj = __shfl(x[i], j) / dj;
                    if (lane == j)
                        x[i] = xj;
                    else if (lane > j)
                        x[i] -= lj * xj;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int s = wv + 4 * i;
                if (s < CK_VI_NPAR && lane < k) U[s][lane] = x[i];
            }
        }
        __syncthreads();
        // ---- 8'. the combination ----
        if (tid < CK_VI_NTRI) {
            double yy = 0.0;
            for (int a = 0; a < k; ++a) yy += U[je][a] * U[ke][a];
            sum += ck_vecchia_info_combine(V, je, ke, yy, qv[je], qv[ke], s2);
        }
    }
    const long long row = A.row0 + blockIdx.x;
    if (tid < CK_VI_NTRI) A.part[row * CK_VI_NTRI + tid] = sum;
    if (tid == 0) A.bad[row] = first_bad;
}

// column sums of n rows of 91: workgroup (x, y) sums the rows 256 x .. of the columns 13 y ..
__global__ __launch_bounds__(LP_TPB) void k_vecchia_info_part(long n, const double* __restrict__ rows, double* __restrict__ part) {
    const long t = (long)blockIdx.x * LP_TPB + threadIdx.x;
    const int c0 = CK_VG_NPAR * blockIdx.y;
    vg_tree([&](int c) { return t < n ? rows[t * CK_VI_NTRI + c0 + c] : 0.0; }, part + (long)blockIdx.x * CK_VI_NTRI + c0);
}

// (ld: the doubles of a row of part -- 91 here, the padded triangle of k_vecchia_trend_gram there)
__global__ __launch_bounds__(LP_TPB) void k_vecchia_info_sum(long nblk, int ld, const double* __restrict__ part,
                                                              double* __restrict__ out91) {
    const int c0 = CK_VG_NPAR * blockIdx.x;
    vg_tree(
        [&](int c) {
            double v = 0.0;
            for (long e = threadIdx.x; e < nblk; e += LP_TPB) v += part[e * ld + c0 + c];
            return v;
        },
        out91 + c0);
}

int ck_vecchia_info_run() { return VI_RUN; }

void ck_launch_vecchia_info(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkVecchiaInfoArgs A) {
    if (m <= 0) return;
    k_vecchia_info<<<dim3((unsigned)((m + VI_RUN - 1) / VI_RUN)), dim3(LP_TPB), 0, s>>>(P, counts, (long)m, A);
}

void ck_launch_vecchia_info_sum(hipStream_t s, int64_t n_rows, const double* rows, double* part, double* out91) {
    if (n_rows <= 0) return;
    const long nblk = (long)((n_rows + LP_TPB - 1) / LP_TPB);
    k_vecchia_info_part<<<dim3((unsigned)nblk, CK_VI_NTRI / CK_VG_NPAR), dim3(LP_TPB), 0, s>>>((long)n_rows, rows, part);
    k_vecchia_info_sum<<<dim3(CK_VI_NTRI / CK_VG_NPAR), dim3(LP_TPB), 0, s>>>(nblk, CK_VI_NTRI, part, out91);
}

// ---------------------------------------------------------------------------------------
// the Vecchia likelihood with a GLS trend (ck_loglik_vecchia_trend; include/cokrige.h has the definition, ck_vecchia_trend.h a
// datum's arithmetic)
// ---------------------------------------------------------------------------------------
// k_vecchia_trend: one workgroup per datum, sets of at most LP_KL data, the system and its 2 + p riding rows in dynamic LDS as
// in k_local_solve_u.  Steps 1 - 4 are k_local_solve's: the same calls of the same device functions with the same arguments
// (the neighbour list under lp_compact's capacity guard, as in k_vecchia_grad), and the p trend rows behind c and z change no
// operation on the rows in front of them -- so mu and v . v come out with ck_loglik_vecchia's bits.  Of the Gram matrix of the
// solved rows only the first column is formed: thread j adds g_j = v . U_j over the set in its order.  An empty set returns
// at once (the outputs are cleared by the caller); a system that is not positive definite writes NaN.
// k_vecchia_trend_terms: k_vecchia_terms with the row r_t = (e_t, f_t) / s_t behind it (ck_vecchia_trend_row), one thread per
// datum in the caller's stacked order; the sums of log s^2 go through vt_tree, so they have ck_loglik_vecchia's bits.
// k_vecchia_trend_gram: G = R^T R.  A workgroup stages the rows of LP_TPB consecutive data in LDS and thread e < (p + 1)(p + 2) / 2
// adds its entry over them in order; the workgroups' triangles (padded to CK_VT_NTRI = 12 x 13) are added by
// k_vecchia_info_sum: vg_tree in the partial-sum order of the scores.  No atomics: repeated calls give the same bits.
// k_vecchia_residual: r_s = z_s - sum_j beta_j X[j][s] over the internal site order -- the values k_vecchia_grad then reads.
#include "ck_vecchia_trend.h"

static_assert(CK_VT_PMAX == CK_LU_PMAX && CK_VT_NTRI % CK_VG_NPAR == 0 && CK_VT_NTRI <= LP_TPB &&
                  CK_VT_NTRI >= CK_VT_ROW * (CK_VT_ROW + 1) / 2,
              "the triangle of G: one thread per entry, whole groups of vg_tree's 13 columns");

__global__ __launch_bounds__(LP_TPB) void k_vecchia_trend(CkLocalProblem P, const int* __restrict__ counts, CkLocalTrend Tr,
                                                           double* __restrict__ mu, double* __restrict__ vv,
                                                           double* __restrict__ g) {
    extern __shared__ __attribute__((aligned(16))) double vt_lds[];   // (LP_KL + nx) x LP_KL matrix
    __shared__ int idx[LP_KL];
    const int tid = threadIdx.x;
    const int np = Tr.p0 + Tr.p1, nx = np + 2;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k == 0 || k > LP_KL) return;   // empty: nothing to solve; larger: refused by the host before any launch
    double* S = vt_lds;
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    lp_compact<false, LP_KL>(P, X, idx);       // 1. neighbour list (the count is the select pass's: never beyond k)
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, trend rows, noise
    lp_cz_rows(P, X, idx, S, ld, k);
    for (int e = tid; e < np * k; e += LP_TPB) {
        const int j = e / k, a = e - j * k;
        S[(long)(k + 2 + j) * ld + a] = Tr.X[(long)j * P.L.npad + idx[a]];
    }
    lp_noise(P, idx, S, ld, k);
    if (!lp_chol(S, ld, k, nx)) {              // 3. Cholesky, the nx extra rows ride along
        if (tid == 0) mu[p] = vv[p] = NAN;
        if (tid < np) g[p * np + tid] = NAN;
        return;
    }
    double vy, v2;                             // 4. mu = v . y, v . v, and the first column of the Gram matrix
    lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &vy, &v2);
    if (tid == 0) {
        mu[p] = vy;
        vv[p] = v2;
    }
    if (tid < np) {
        const double *v = S + (long)k * ld, *u = S + (long)(k + 2 + tid) * ld;
        double acc = 0.0;
        for (int a = 0; a < k; ++a) acc += v[a] * u[a];
        g[p * np + tid] = acc;
    }
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_trend_terms(long n, const double* __restrict__ z, const double* __restrict__ mu,
                                                                 const double* __restrict__ vv, const double* __restrict__ prior,
                                                                 const double* __restrict__ noise, const int* __restrict__ cnt2,
                                                                 CkVecchiaTrendRows T, double* __restrict__ mean,
                                                                 double* __restrict__ var, double* __restrict__ part,
                                                                 long long* __restrict__ bad) {
    const long t = (long)blockIdx.x * LP_TPB + threadIdx.x;
    double lv = 0.0, qd = 0.0;
    long long b = 0;
    if (t < n) {
        double m, s2;   // (the row goes straight to global memory: a local array indexed by j would live in scratch)
        if (ck_vecchia_trend_row(z[t], mu[t], vv[t], prior[t], noise ? noise[t] : 0.0, cnt2[2 * t] + cnt2[2 * t + 1], T.p,
                                 T.X + T.gself[t], (long)T.npad, T.g + t * T.p, &m, &s2, &lv, &qd, T.rows + t * (T.p + 1)))
            b = t + 1;
        mean[t] = m;
        var[t] = s2;
    }
    vt_tree(lv, qd, b, part + 2 * blockIdx.x, bad + blockIdx.x);
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_trend_gram(long n, int p, const double* __restrict__ rows,
                                                                double* __restrict__ part) {
    __shared__ double R[LP_TPB * CK_VT_ROW];
    const int tid = threadIdx.x, w = p + 1;
    const long e0 = (long)blockIdx.x * LP_TPB * w, e1 = n * w;   // the workgroup's rows are contiguous in `rows`
    for (int e = tid; e < LP_TPB * w; e += LP_TPB) R[e] = e0 + e < e1 ? rows[e0 + e] : 0.0;
    __syncthreads();
    if (tid < CK_VT_NTRI) {
        double acc = 0.0;
        if (tid < w * (w + 1) / 2) {
            int r, c;
            ck_vecchia_trend_pair(tid, &r, &c);
            for (int t = 0; t < LP_TPB; ++t) acc += R[t * w + r] * R[t * w + c];
        }
        part[(long)blockIdx.x * CK_VT_NTRI + tid] = acc;
    }
}

__global__ __launch_bounds__(LP_TPB) void k_vecchia_residual(long npad, int p, const double* __restrict__ z,
                                                              const double* __restrict__ X, CkVecchiaTrendBeta B,
                                                              double* __restrict__ out) {
    const long s = (long)blockIdx.x * LP_TPB + threadIdx.x;
    if (s >= npad) return;
    double acc = 0.0;
    for (int j = 0; j < p; ++j) acc += B.b[j] * X[(long)j * npad + s];
    out[s] = z[s] - acc;
}

void ck_launch_vecchia_trend(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkLocalTrend Tr, double* mu,
                             double* vv, double* g) {
    if (m <= 0) return;
    const size_t lds = (size_t)((LP_KL + 2 + Tr.p0 + Tr.p1) * LP_KL) * sizeof(double);   // 34 KB (p = 2) .. 41 KB (p = 16)
    k_vecchia_trend<<<dim3((unsigned)m), dim3(LP_TPB), lds, s>>>(P, counts, Tr, mu, vv, g);
}

void ck_launch_vecchia_trend_terms(hipStream_t s, int64_t n, const double* z, const double* mu, const double* vv, const double* prior,
                                   const double* noise, const int* cnt2, CkVecchiaTrendRows T, double* mean, double* var,
                                   double* part, long long* bad, double* out2, long long* info) {
    if (n <= 0) return;
    const long nblk = (long)((n + LP_TPB - 1) / LP_TPB);
    k_vecchia_trend_terms<<<dim3((unsigned)nblk), dim3(LP_TPB), 0, s>>>((long)n, z, mu, vv, prior, noise, cnt2, T, mean, var, part,
                                                                        bad);
    k_vecchia_sum<<<dim3(1), dim3(LP_TPB), 0, s>>>(nblk, part, bad, out2, info);
}

void ck_launch_vecchia_trend_gram(hipStream_t s, int64_t n, int p, const double* rows, double* part, double* out_tri) {
    if (n <= 0) return;
    const long nblk = (long)((n + LP_TPB - 1) / LP_TPB);
    k_vecchia_trend_gram<<<dim3((unsigned)nblk), dim3(LP_TPB), 0, s>>>((long)n, p, rows, part);
    k_vecchia_info_sum<<<dim3(CK_VT_NTRI / CK_VG_NPAR), dim3(LP_TPB), 0, s>>>(nblk, CK_VT_NTRI, part, out_tri);
}

void ck_launch_vecchia_residual(hipStream_t s, int64_t npad, int p, const double* z, const double* X, CkVecchiaTrendBeta B,
                                double* out) {
    if (npad <= 0) return;
    k_vecchia_residual<<<dim3((unsigned)((npad + LP_TPB - 1) / LP_TPB)), dim3(LP_TPB), 0, s>>>((long)npad, p, z, X, B, out);
}

// ---------------------------------------------------------------------------------------
// conditional simulation in the moving neighbourhood (ck_simulate_local; ck_internal.h: CkLocalSimOut, CkLocalSimLevel)
// ---------------------------------------------------------------------------------------
// k_local_sim_weights: one workgroup per site.  Steps 1 - 5 are k_vecchia_grad's, the same calls of the same device functions;
// then ONE wave (the set has at most 64 members, lane a holds member a) splits the set by P.rs[g] >= n_data into data and earlier
// sites: the weights of all members go out in list order, those of the sites once more compacted by a ballot, and the data's
// share of the mean is summed in list order by broadcasting the lanes one after the other -- every lane runs the same 64 steps,
// so the sum has one order.  Plain vector stores, no atomics: repeated calls give the same bits.
__global__ __launch_bounds__(LP_TPB) void k_local_sim_weights(CkLocalProblem P, const int* __restrict__ counts, CkLocalSimOut O) {
    __shared__ double S[(LP_KL + 2) * LP_KL];
    __shared__ int idx[LP_KL];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long p = blockIdx.x;
    const int k = counts[p];
    if (k > LP_KL) return;   // refused by the host before any launch
    int *gi = O.gidx + p * LP_KL, *sp = O.spos + p * LP_KL;
    double *wr = O.w + p * LP_KL, *sw = O.sw + p * LP_KL;
    if (k == 0) {   // an empty set: the prior
        if (tid < LP_KL) {
            gi[tid] = sp[tid] = -1;
            wr[tid] = sw[tid] = 0.0;
        }
        if (tid == 0) {
            O.mu[p] = 0.0;
            O.s2[p] = P.c0var;
            O.ns[p] = 0;
        }
        return;
    }
    const long ld = LP_KL;
    const LpPoint X = lp_point(P, p);
    lp_compact<false, LP_KL>(P, X, idx);       // 1. neighbour list (the count is the select pass's: never beyond k)
    lp_triangle(P, X, idx, S, ld, k);          // 2. local covariance, c row, z row, noise
    lp_cz_rows(P, X, idx, S, ld, k);
    lp_noise(P, idx, S, ld, k);
    const bool ok = lp_chol(S, ld, k, 2);      // 3. Cholesky, the two extra rows ride along
    double vy, vvs;                            // 4. c . w = v . v (uniform: the sums of a failed factor are not used)
    lp_dots(S + (long)k * ld, S + (long)(k + 1) * ld, k, &vy, &vvs);
    if (ok) vg_back_substitute(S, ld, k);      // 5. row k becomes -w
    if (wv != 0) return;
    const bool in = lane < k;
    const int g = in ? idx[lane] : -1;
    const int r = in ? P.rs[g] : 0;
    const bool site = in && r >= O.n_data;
    const double wa = in ? (ok ? -S[(long)k * ld + lane] : NAN) : 0.0;
    const double za = in && !site ? P.z[g] : 0.0;
    const unsigned long long bal = __ballot(site);
    const int below = __popcll(bal & ((1ULL << lane) - 1ULL)), nsite = __popcll(bal);
    double mu = 0.0;
    for (int a = 0; a < k; ++a) {              // the data's share of the mean, list order
        const double t = __shfl(wa, a) * __shfl(za, a);
        if (!(bal >> a & 1ULL)) mu += t;
    }
    gi[lane] = g;
    wr[lane] = wa;
    if (lane >= nsite) {
        sp[lane] = -1;
        sw[lane] = 0.0;
    }
    if (site) {
        sp[below] = r - O.n_data;
        sw[below] = wa;
    }
    if (lane == 0) {
        O.mu[p] = ok ? mu : NAN;
        O.s2[p] = ok ? P.c0var - vvs : NAN;
        O.ns[p] = nsite;
    }
}

void ck_launch_local_sim_weights(hipStream_t s, const CkLocalProblem& P, int64_t m, const int* counts, CkLocalSimOut O) {
    if (m <= 0) return;
    k_local_sim_weights<<<dim3((unsigned)m), dim3(LP_TPB), 0, s>>>(P, counts, O);
}

// k_local_sim_level: workgroup (site of the level, tile of draw pairs).  The site's row of at most 64 (position, weight) entries
// is staged in LDS; a thread owns the draw pair (d, d + 1) and reads the neighbours' rows of Y as 16-byte words, consecutive
// threads consecutive words.  The sum starts from mu, adds the neighbours in list order and then s eps: its bits do not depend
// on n_draws or on the chunk.
__global__ __launch_bounds__(LP_TPB) void k_local_sim_level(CkLocalSimLevel A, const int* __restrict__ order) {
    __shared__ int su[LP_KL];
    __shared__ double sw[LP_KL];
    const int tid = threadIdx.x;
    const long t = order[blockIdx.x];
    const int n = A.ns[t];
    if (tid < n) {
        su[tid] = A.spos[t * LP_KL + tid];
        sw[tid] = A.sw[t * LP_KL + tid];
    }
    __syncthreads();
    const long d = 2 * ((long)blockIdx.y * blockDim.x + tid);
    if (d >= A.ldy) return;
    double a0 = A.mu[t], a1 = a0;
    for (int j = 0; j < n; ++j) {
        const d2_t y = *reinterpret_cast<const d2_t*>(A.Y + (long)su[j] * A.ldy + d);
        a0 += sw[j] * y[0];
        a1 += sw[j] * y[1];
    }
    double* own = A.Y + (long)A.pos[t] * A.ldy + d;
    double e[2];
    if (A.eps_in_y) {   // the caller's noise, put there by k_local_sim_gather
        const d2_t ev = *reinterpret_cast<const d2_t*>(own);
        e[0] = ev[0];
        e[1] = ev[1];
    } else {
        ck_rng_normal2((uint64_t)A.seed, (uint32_t)t, (uint32_t)((A.d0 + d) >> 1), e);
    }
    const double v = A.s2[t];
    const double sd = v > 0.0 ? sqrt(v) : NAN;
    d2_t out;
    out[0] = a0 + sd * e[0];
    out[1] = a1 + sd * e[1];
    *reinterpret_cast<d2_t*>(own) = out;
}

void ck_launch_local_sim_level(hipStream_t s, const CkLocalSimLevel& A, const int* order, int64_t n) {
    if (n <= 0 || A.ldy <= 0) return;
    const long pairs = A.ldy / 2;
    const int tpb = pairs <= 64 ? 64 : pairs <= 128 ? 128 : LP_TPB;
    k_local_sim_level<<<dim3((unsigned)n, (unsigned)((pairs + tpb - 1) / tpb)), dim3(tpb), 0, s>>>(A, order);
}

// X[d][t] = Y[pos[t]][d]: 32 x 32 tiles through LDS, reads along the draws, writes along the sites
__global__ __launch_bounds__(LP_TPB) void k_local_sim_scatter(const double* __restrict__ Y, long ldy, const int* __restrict__ pos,
                                                               long m, long nd, double* __restrict__ X) {
    __shared__ double T[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long t0 = (long)blockIdx.x * 32, d0 = (long)blockIdx.y * 32;
    for (int r = ty; r < 32; r += LP_TPB / 32) {
        const long t = t0 + r, d = d0 + tx;
        if (t < m && d < nd) T[r][tx] = Y[(long)pos[t] * ldy + d];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += LP_TPB / 32) {
        const long d = d0 + r, t = t0 + tx;
        if (t < m && d < nd) X[d * m + t] = T[tx][r];
    }
}

// Y[pos[t]][d] = E[d][t] for d < nd, 0 in the scratch draws up to ldy: the caller's noise (nd x m, the caller's order) laid out
// as the recursion reads it, the scatter in reverse
__global__ __launch_bounds__(LP_TPB) void k_local_sim_gather(const double* __restrict__ E, long m, long nd, const int* __restrict__ pos,
                                                              double* __restrict__ Y, long ldy) {
    __shared__ double T[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long t0 = (long)blockIdx.x * 32, d0 = (long)blockIdx.y * 32;
    for (int r = ty; r < 32; r += LP_TPB / 32) {
        const long d = d0 + r, t = t0 + tx;
        T[r][tx] = (t < m && d < nd) ? E[d * m + t] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += LP_TPB / 32) {
        const long t = t0 + r, d = d0 + tx;
        if (t < m && d < ldy) Y[(long)pos[t] * ldy + d] = T[tx][r];
    }
}

void ck_launch_local_sim_gather(hipStream_t s, const double* E, int64_t m, int64_t nd, const int* pos, double* Y, int64_t ldy) {
    if (m <= 0 || ldy <= 0) return;
    k_local_sim_gather<<<dim3((unsigned)((m + 31) / 32), (unsigned)((ldy + 31) / 32)), dim3(LP_TPB), 0, s>>>(E, (long)m, (long)nd, pos, Y,
                                                                                                         (long)ldy);
}

void ck_launch_local_sim_scatter(hipStream_t s, const double* Y, int64_t ldy, const int* pos, int64_t m, int64_t nd, double* X) {
    if (m <= 0 || nd <= 0) return;
    k_local_sim_scatter<<<dim3((unsigned)((m + 31) / 32), (unsigned)((nd + 31) / 32)), dim3(LP_TPB), 0, s>>>(Y, (long)ldy, pos, (long)m,
                                                                                                          (long)nd, X);
}

// ---------------------------------------------------------------------------------------
// leave-group-out cross-validation in the moving neighbourhood (ck_cv_local_folds; include/cokrige.h has the rules)
// ---------------------------------------------------------------------------------------
// The search is lp_candidate / lp_is_neighbour's with the withholding conditions (lp_same_fold, lp_in_reach); the solves are the
// prediction kernels'.  Two kernels of its own.  k_cv_labels: the labels of both processes from the caller's stacked order into
// the internal site order (fs starts as -1 everywhere; gself: every datum's own internal position, ck_host_local_cv_plan).
// k_cv_fold_scores: one workgroup per fold over the fold's predicted data (idx[off[f] .. off[f + 1]): positions in the call's
// point list, ascending): thread t sums entries t, t + 256, .. in order, then the 256-wide tree of lp_dots over the five columns
// n, sum e, sum e^2, sum e^2 / v, sum log v with e = z - pred, v = err^2 + own (the datum's own s d, null: none).  A datum whose
// pred is not finite or whose v is not > 0 is skipped and not counted.  No atomics: repeated calls give the same bits.
__global__ __launch_bounds__(LP_TPB) void k_cv_labels(long n0, long n1, const int* __restrict__ fold0, const int* __restrict__ fold1,
                                                       const int* __restrict__ gself, int* __restrict__ fs) {
    const long t = (long)blockIdx.x * LP_TPB + threadIdx.x;
    if (t < n0) {
        if (fold0) fs[gself[t]] = fold0[t];
    } else if (t < n0 + n1) {
        if (fold1) fs[gself[t]] = fold1[t - n0];
    }
}

__global__ __launch_bounds__(LP_TPB) void k_cv_fold_scores(CkCvScoreArgs A) {
    __shared__ double red[CK_CV_NSCORE][LP_TPB];
    const int tid = threadIdx.x;
    const long long b = A.off[blockIdx.x], e = A.off[blockIdx.x + 1];
    double acc[CK_CV_NSCORE] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long q = b + tid; q < e; q += LP_TPB) {
        const int t = A.idx[q];
        const double p = A.pred[t], sd = A.err[t];
        const double v = sd * sd + (A.own ? A.own[t] : 0.0);
        if (!isfinite(p) || !(v > 0.0)) continue;
        const double r = A.z[t] - p;
        acc[0] += 1.0;
        acc[1] += r;
        acc[2] += r * r;
        acc[3] += r * r / v;
        acc[4] += log(v);
    }
#pragma unroll
    for (int c = 0; c < CK_CV_NSCORE; ++c) red[c][tid] = acc[c];
    __syncthreads();
    for (int s = LP_TPB / 2; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int c = 0; c < CK_CV_NSCORE; ++c) red[c][tid] += red[c][tid + s];
        __syncthreads();
    }
    if (tid < CK_CV_NSCORE) A.out[(long)blockIdx.x * CK_CV_NSCORE + tid] = red[tid][0];
}

void ck_launch_cv_labels(hipStream_t s, int64_t n0, int64_t n1, const int* fold0, const int* fold1, const int* gself, int* fs) {
    if (n0 + n1 <= 0 || (!fold0 && !fold1)) return;
    k_cv_labels<<<dim3((unsigned)((n0 + n1 + LP_TPB - 1) / LP_TPB)), dim3(LP_TPB), 0, s>>>((long)n0, (long)n1, fold0, fold1, gself, fs);
}

void ck_launch_cv_fold_scores(hipStream_t s, int64_t n_groups, CkCvScoreArgs A) {
    if (n_groups <= 0) return;
    k_cv_fold_scores<<<dim3((unsigned)n_groups), dim3(LP_TPB), 0, s>>>(A);
}
