// ck_draws.hip -- conditional simulation: the deflation of the posterior covariance S and the noise of the draws
// (ck_api.hip: ck_conditional_draws; the draw product X = E L_S^T is ck_la.hip: k_draw_trmm).
//
// S = C_pp - V^T V sits in ck_verify_model's Schur buffers: packed block columns of width NB, panel J holding rows
// [J NB, Mp) x columns [J NB, (J + 1) NB), ld = NB.  Only the lower triangle is meaningful; these kernels never read
// above the diagonal.
//
// Deflation.  A prediction site on a datum of the predicted process has zero posterior variance (the nugget is in c0 at
// h == 0 as in C_pp), and for a positive semi-definite S a zero diagonal entry means a zero row and column
// (Cauchy-Schwarz).  Such a site is removed from the factorisation exactly: its row and column become e_k, so that
// column k of L_S is e_k, its noise is zeroed and its draw is pred.  The other sites' joint distribution is unchanged.
#include "ck_internal.h"
#include "ck_rng.h"

// one thread per site k < m: the verdict S_kk <= thr, then the diagonal 1 (deflated) or S_kk + jit
// PAIR (ck_conditional_draws_pair): the sites of process 0 in [0, m0), those of process 1 in [m0p, m), each judged by its own
// process's threshold and jitter (thr / jit: process 0, thr1 / jit1: process 1).  The gap rows [m0, m0p) are identity rows of S
// already: they count as deflated for good (mask 2, diagonal left at 1), so that every later kernel skips them like a site on a datum.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_draw_deflate(double* const* __restrict__ sch, long m, double thr, double jit,
                                                      unsigned char* __restrict__ mask, long m0 = 0, long m0p = 0,
                                                      double thr1 = 0.0, double jit1 = 0.0) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    if (PAIR && k >= m0 && k < m0p) {
        mask[k] = 2;
        return;
    }
    const long J = k / CK_NB, loc = k - J * CK_NB;
    double* d = sch[J] + loc * CK_NB + loc;
    const double s = *d;
    const bool defl = s <= ((PAIR && k >= m0p) ? thr1 : thr);
    mask[k] = defl ? 1 : 0;
    *d = defl ? 1.0 : s + ((PAIR && k >= m0p) ? jit1 : jit);
}

// the strictly lower entries (r, c), r < m, of rows or columns of deflated sites -> 0.  Workgroup (r, J): row r of panel J.
__global__ __launch_bounds__(256) void k_draw_zero(double* const* __restrict__ sch, long m,
                                                   const unsigned char* __restrict__ mask) {
    const long r = blockIdx.x;
    const long J = blockIdx.y;
    const long c0 = J * CK_NB;
    if (r < c0) return;
    const bool row_defl = mask[r] != 0;
    double* row = sch[J] + (r - c0) * CK_NB;
    for (int t = threadIdx.x; t < CK_NB; t += 256) {
        const long c = c0 + t;
        if (c >= r || c >= m) break;
        if (row_defl || mask[c]) row[t] = 0.0;
    }
}

// above the diagonal of every 512 x 512 diagonal block -> 0 (the draw product reads whole panel rows)
__global__ __launch_bounds__(256) void k_draw_upper(double* const* __restrict__ sch) {
    const int r = blockIdx.x;
    double* row = sch[blockIdx.y] + (long)r * CK_NB;
    for (int t = r + 1 + threadIdx.x; t < CK_NB; t += 256) row[t] = 0.0;
}

// E (the A operand of k_draw_trmm, negated): block column p of the chunk at E + p ldp NB, row d, ld NB.
// Element (d, j), j the internal site index: 0 beyond the chunk's nd rows, beyond m and at deflated sites; else
// -eps(d0 + d, caller's site cmap[j]) -- from noise (nd x ldn, the caller's order) or the Philox stream of ck_rng.h.
// ldn: the caller's number of sites -- m, or fewer where deflated rows that map to no caller column lie among the m (the gap of
// ck_conditional_draws_pair's stacked layout).
__global__ __launch_bounds__(256) void k_draw_noise(double* __restrict__ E, long ldp, long n_el, long nd, long m, long d0,
                                                    const int* __restrict__ cmap, const unsigned char* __restrict__ mask,
                                                    const double* __restrict__ noise, unsigned long long seed, long ldn) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_el) return;
    const long p = e / (ldp * CK_NB);
    const long rem = e - p * ldp * CK_NB;
    const long d = rem / CK_NB;
    const long j = p * CK_NB + (rem - d * CK_NB);
    double v = 0.0;
    if (d < nd && j < m && !mask[j]) {
        const int k = cmap[j];
        if (noise) {
            v = noise[d * ldn + k];
        } else {
            double z[2];
            const long dg = d0 + d;
            ck_rng_normal2((uint64_t)seed, (uint32_t)k, (uint32_t)(dg >> 1), z);
            v = z[dg & 1];
        }
    }
    E[e] = -v;
}

void ck_launch_draw_deflate(hipStream_t s, double* const* sch, int nJ, int64_t m, double thr, double jit, unsigned char* mask) {
    if (m <= 0) return;
    k_draw_deflate<false><<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s>>>(sch, (long)m, thr, jit, mask);
    (void)nJ;
}

void ck_launch_draw_deflate_pair(hipStream_t s, double* const* sch, int64_t m0, int64_t m0p, int64_t m, const double thr[2],
                                 const double jit[2], unsigned char* mask) {
    if (m <= 0) return;
    k_draw_deflate<true><<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s>>>(sch, (long)m, thr[0], jit[0], mask, (long)m0,
                                                                                (long)m0p, thr[1], jit[1]);
}

void ck_launch_draw_zero(hipStream_t s, double* const* sch, int nJ, int64_t m, const unsigned char* mask) {
    if (m <= 0 || nJ <= 0) return;
    k_draw_zero<<<dim3((unsigned)m, (unsigned)nJ), dim3(256), 0, s>>>(sch, (long)m, mask);
}

void ck_launch_draw_upper(hipStream_t s, double* const* sch, int nJ) {
    if (nJ <= 0) return;
    k_draw_upper<<<dim3((unsigned)CK_NB, (unsigned)nJ), dim3(256), 0, s>>>(sch);
}

void ck_launch_draw_noise(hipStream_t s, double* E, int64_t ldp, int64_t Mp, int64_t nd, int64_t m, int64_t d0, const int* cmap,
                          const unsigned char* mask, const double* noise, uint64_t seed, int64_t ldn) {
    const int64_t n_el = ldp * Mp;
    if (n_el <= 0) return;
    k_draw_noise<<<dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s>>>(E, (long)ldp, (long)n_el, (long)nd, (long)m, (long)d0,
                                                                          cmap, mask, noise, (unsigned long long)seed,
                                                                          (long)(ldn > 0 ? ldn : m));
}
