// ck_lik.hip -- the Gaussian log-likelihood of the joint model and its gradient (ck_loglik, ck_api.hip).
//
//   l(theta)      = -1/2 (N log 2 pi + log|Sigma| + z^T Sigma^-1 z),  log|Sigma| = 2 sum log L_qq
//   dl/dtheta_k   = 1/2 sum_pq G_pq (dSigma/dtheta_k)_pq,               G = alpha alpha^T - Sigma^-1, alpha = Sigma^-1 z
//
//   k_lik_logdet     sum of log L_qq per panel (the host adds the panels' partial sums in panel order).
//   k_loglik_grad    one pass over the lower triangle of G (ck_la.hip: k_ginv_syrk_d built it): every entry evaluates the
//                    derivatives of its Matern block with the exact evaluator (ck_math.h: ck_matern_grad) and adds them,
//                    weighted, into per-thread sums; every workgroup writes one partial vector (fixed-order reduction), the
//                    host sums them in workgroup order.  No atomics: two calls give the same bits.
// The distance and the test h == 0 are those of the assembly's exact path (ck_cov.hip: pair_dist, k_assemble_fix), which
// evaluates every pair the tables leave out -- among them all pairs at h == 0, where the nugget enters.
#include "ck_internal.h"

__device__ __forceinline__ bool lik_valid(const CkLayout& L, long g) { return g < L.n0 || (g >= L.n0p && g < L.nend); }

__global__ __launch_bounds__(256) void k_lik_logdet(double* const* __restrict__ sigptr, CkLayout L, double* __restrict__ part) {
    __shared__ double red[4];
    const int K = blockIdx.x;
    const double* P = sigptr[K];
    double s = 0.0;
    for (int j = threadIdx.x; j < CK_NB; j += 256) {
        const long g = (long)K * CK_NB + j;
        if (lik_valid(L, g)) s += log(P[(long)j * CK_NB + j]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[K] = ((red[0] + red[1]) + red[2]) + red[3];
}

void ck_launch_lik_logdet(hipStream_t s, double* const* sigptr_dev, int nK, CkLayout L, double* part) {
    if (nK <= 0) return;
    k_lik_logdet<<<dim3((unsigned)nK), dim3(256), 0, s>>>(sigptr_dev, L, part);
}

// One workgroup per 64-row strip of a block column of G (strip t of block column J: rows J NB + 64 t ..), 256 threads;
// entry e = tid + 256 k of the strip's 64 x 512 is row e / 512, column e % 512: a wave covers 64 consecutive columns of one
// row -- one Matern block (process boundaries lie on multiples of 64), so the block's branch is wave-uniform.
#define CK_LIK_STRIPS(npad) ((npad) / 64)

__global__ __launch_bounds__(256) void k_loglik_grad(double* const* __restrict__ G, CkLayout L, int n_procs, int metric,
                                                      const double* __restrict__ c, const CkMatern* __restrict__ blk5,
                                                      double dnu0, double dnu1, double dnu2, double sig1, double sig2,
                                                      double rho, double* __restrict__ part) {
    __shared__ double red[4][CK_LIK_NPAR];
    const long strips = CK_LIK_STRIPS(L.npad);
    const int J = (int)(blockIdx.x / strips);
    const long t = (long)blockIdx.x - (long)J * strips;
    const long rs = (long)t * 64;                    // strip's first row inside block column J
    const long p0 = (long)J * CK_NB + rs;            // its global row
    double acc[CK_LIK_NPAR];
#pragma unroll
    for (int k = 0; k < CK_LIK_NPAR; ++k) acc[k] = 0.0;
    if (p0 < L.nend) {   // strips below the last site (and beyond the block column's rows) contribute nothing
        const double* Gj = G[J];
        const double* c0 = c;
        const double* c1 = c + L.npad;
        const double* c2 = c + 2 * L.npad;
        for (int k = 0; k < 128; ++k) {
            const int e = threadIdx.x + 256 * k;
            const long p = p0 + (e >> 9);
            const long q = (long)J * CK_NB + (e & 511);
            if (q > p || !lik_valid(L, p) || !lik_valid(L, q)) continue;
            const int pp = p >= L.n0p && n_procs == 2 ? 1 : 0, pq = q >= L.n0p && n_procs == 2 ? 1 : 0;
            const int b = pp + pq;
            const double w = (p == q ? 0.5 : 1.0) * Gj[(rs + (e >> 9)) * CK_NB + (e & 511)];
            const double h = metric == CK_METRIC_HAVERSINE ? ck_haversine_km(c0[p], c1[p], c2[p], c0[q], c1[q], c2[q])
                                                           : ck_euclid(c0[p], c1[p], c0[q], c1[q]);
            const CkMatern& m = blk5[5 * b];
            const double dnu = b == 0 ? dnu0 : b == 1 ? dnu1 : dnu2;
            const CkMaternGrad gr = ck_matern_grad(m, blk5 + 5 * b + 1, dnu, h);
            const double z0 = h == 0.0 ? w : 0.0;
            if (n_procs == 1) {   // sigma nu len nugget
                acc[0] += w * (2.0 * sig1 * gr.M);
                acc[1] += w * (m.amp * gr.dnu);
                acc[2] += w * (m.amp * gr.dlen);
                acc[3] += z0;
            } else if (b == 0) {  // sigma_11 sigma_22 nu_11 nu_12 nu_22 len_11 len_12 len_22 nugget_11 nugget_22 rho_12
                acc[0] += w * (2.0 * sig1 * gr.M);
                acc[2] += w * (m.amp * gr.dnu);
                acc[5] += w * (m.amp * gr.dlen);
                acc[8] += z0;
            } else if (b == 2) {
                acc[1] += w * (2.0 * sig2 * gr.M);
                acc[4] += w * (m.amp * gr.dnu);
                acc[7] += w * (m.amp * gr.dlen);
                acc[9] += z0;
            } else {
                acc[0] += w * (rho * sig2 * gr.M);
                acc[1] += w * (rho * sig1 * gr.M);
                acc[10] += w * (sig1 * sig2 * gr.M);
                acc[3] += w * (m.amp * gr.dnu);
                acc[6] += w * (m.amp * gr.dlen);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CK_LIK_NPAR; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        acc[k] = v;
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < CK_LIK_NPAR; ++k) red[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < CK_LIK_NPAR) {
        const int k = threadIdx.x;
        part[(long)blockIdx.x * CK_LIK_NPAR + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// Derivative in the noise scales (ck_loglik_noise_grad): dl/ds_k = 1/2 sum_{a in k} G_aa d_a over the diagonal of the packed
// G tiles.  One workgroup per block column; part[2 K], part[2 K + 1] = that column's sums of G_aa d_a for process 0 / 1 (the
// host adds the columns in order and halves).  d: npad variances in the internal site order.  Fixed order, no atomics.
__global__ __launch_bounds__(256) void k_lik_noise_grad(double* const* __restrict__ G, CkLayout L, const double* __restrict__ d,
                                                         double* __restrict__ part) {
    __shared__ double red[4][2];
    const int K = blockIdx.x;
    const double* Gk = G[K];
    double s0 = 0.0, s1 = 0.0;
    for (int j = threadIdx.x; j < CK_NB; j += 256) {
        const long g = (long)K * CK_NB + j;
        if (!lik_valid(L, g)) continue;
        const double v = Gk[(long)j * CK_NB + j] * d[g];
        if (g >= L.n0p)
            s1 += v;
        else
            s0 += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = s0;
        red[threadIdx.x >> 6][1] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part[2 * K + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

void ck_launch_lik_noise_grad(hipStream_t s, double* const* G_dev, int nK, CkLayout L, const double* d, double* part) {
    if (nK <= 0) return;
    k_lik_noise_grad<<<dim3((unsigned)nK), dim3(256), 0, s>>>(G_dev, L, d, part);
}

int64_t ck_lik_grad_groups(CkLayout L) { return (L.npad / CK_NB) * CK_LIK_STRIPS(L.npad); }

// ck_debug_matern_grad: one thread per lag, ck_matern_grad on the stencil of one block exactly as k_loglik_grad calls it
__global__ void k_debug_matern_grad(const CkMatern* __restrict__ blk5, double dnu, const double* __restrict__ lags, long n,
                                    double* __restrict__ out3) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CkMaternGrad gr = ck_matern_grad(blk5[0], blk5 + 1, dnu, fabs(lags[i]));
    out3[3 * i] = gr.M;
    out3[3 * i + 1] = gr.dnu;
    out3[3 * i + 2] = gr.dlen;
}

void ck_launch_debug_matern_grad(hipStream_t s, const CkMatern* blk5, double dnu, const double* lags, int64_t n, double* out3) {
    if (n <= 0) return;
    k_debug_matern_grad<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(blk5, dnu, lags, n, out3);
}

void ck_launch_loglik_grad(hipStream_t s, double* const* G_dev, CkLayout L, int n_procs, int metric, const double* c,
                           const CkMatern* blk5, const double* dnu3, double sig1, double sig2, double rho, double* part) {
    const int64_t n = ck_lik_grad_groups(L);
    if (n <= 0) return;
    k_loglik_grad<<<dim3((unsigned)n), dim3(256), 0, s>>>(G_dev, L, n_procs, metric, c, blk5, dnu3[0], dnu3[1], dnu3[2], sig1,
                                                         sig2, rho, part);
}
