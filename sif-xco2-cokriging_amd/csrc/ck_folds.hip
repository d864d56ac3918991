// ck_folds.hip -- leave-group-out cross-validation (ck_cv_folds): what follows the folds' Gram matrices (ck_la.hip: k_fold_gram).
//
// Per fold S with Q_SS = W_S W_S^T and alpha_S = W_S y (W the solved unit right-hand-side rows, y the solved data row):
//     Q_SS = R R^T,  t = R^-1 alpha_S,  x = R^-T t = Q_SS^-1 alpha_S,  d_q = (Q_SS^-1)_qq = |column q of R^-1|^2,
//     log|Q_SS| = 2 sum log R_jj,  alpha_S^T Q_SS^-1 alpha_S = |t|^2.
//   k_fold_small      folds of up to CK_HOST_FOLD_LDS (64) members: one wave per fold, everything in LDS.
//   k_fold_big_fill   larger folds: the fold becomes the symmetric system [[Q_SS, .], [I, BIG], [alpha^T, ., BIG]] whose blocked
//                     Cholesky (the local predictor's batched steps, ck_la.hip: k_lt_*, driven left-looking by ck_api.hip and
//                     stopped behind column s) leaves row q of R^-T in row s + q and t in row 2 s -- the unit rows and alpha
//                     ride along as the c and z rows of a neighbourhood do.
//   k_fold_big_reduce x, d, log|Q_SS| and |t|^2 from those rows.
// Every sum has a fixed order and there are no atomics: repeated calls give the same bits.  A fold whose factorisation meets a
// non-positive pivot gets fail[fold] = 1 and NaN outputs; no other fold is touched.
// Outputs are indexed like the gather list (ck_host.h: CkFoldPlan::gpos): member q of a fold at gbase + q.
#include "ck_internal.h"

#define FS_P 65   // LDS pitch of the 64 x 64 arrays

__global__ __launch_bounds__(64) void k_fold_small(const CkFoldSmall* __restrict__ folds, const double* __restrict__ buf,
                                                    const int* __restrict__ grow, const double* __restrict__ dots,
                                                    double* __restrict__ x_out, double* __restrict__ d_out,
                                                    double* __restrict__ stat2, int* __restrict__ fail) {
    __shared__ double A[64 * FS_P];   // Q, then R (lower)
    __shared__ double W[64 * FS_P];   // R^-1 (lower)
    __shared__ double al[64], tt[64];
    __shared__ int bad;
    const CkFoldSmall f = folds[blockIdx.x];
    const int s = f.s, j = threadIdx.x;
    const int tile = f.gbase / CK_HOST_FOLD_TILE, o = f.gbase % CK_HOST_FOLD_TILE;
    const double* Q = buf + (long)tile * CK_HOST_FOLD_TILE * CK_HOST_FOLD_TILE + (long)o * CK_HOST_FOLD_TILE + o;
    if (j == 0) bad = 0;
    for (int r = 0; r < s; ++r)
        if (j <= r) A[r * FS_P + j] = Q[(long)r * CK_HOST_FOLD_TILE + j];
    if (j < s) al[j] = dots[grow[f.gbase + j]];
    __syncthreads();
    // right-looking Cholesky, thread j owns row j
    for (int k = 0; k < s; ++k) {
        const double d = A[k * FS_P + k];
        if (!(d > 0.0) || d != d) {   // (uniform: every thread reads the same pivot)
            if (j == 0) bad = 1;
            break;
        }
        const double rk = sqrt(d);
        __syncthreads();
        if (j == k) A[k * FS_P + k] = rk;
        if (j > k && j < s) A[j * FS_P + k] /= rk;
        __syncthreads();
        if (j > k && j < s) {
            const double ljk = A[j * FS_P + k];
            for (int c = k + 1; c <= j; ++c) A[j * FS_P + c] -= ljk * A[c * FS_P + k];
        }
        __syncthreads();
    }
    __syncthreads();
    if (bad) {
        if (j < s) {
            x_out[f.gbase + j] = NAN;
            d_out[f.gbase + j] = NAN;
        }
        if (j == 0) {
            stat2[2 * f.fold] = NAN;
            stat2[2 * f.fold + 1] = NAN;
            fail[f.fold] = 1;
        }
        return;
    }
    // column j of R^-1: R w = e_j by forward substitution
    if (j < s) {
        for (int r = 0; r < j; ++r) W[r * FS_P + j] = 0.0;
        W[j * FS_P + j] = 1.0 / A[j * FS_P + j];
        for (int r = j + 1; r < s; ++r) {
            double acc = 0.0;
            for (int c = j; c < r; ++c) acc += A[r * FS_P + c] * W[c * FS_P + j];
            W[r * FS_P + j] = -acc / A[r * FS_P + r];
        }
    }
    __syncthreads();
    if (j < s) {   // t_j = (R^-1 alpha)_j
        double acc = 0.0;
        for (int c = 0; c <= j; ++c) acc += W[j * FS_P + c] * al[c];
        tt[j] = acc;
    }
    __syncthreads();
    if (j < s) {
        double x = 0.0, d = 0.0;
        for (int r = j; r < s; ++r) {
            const double w = W[r * FS_P + j];
            x += w * tt[r];
            d += w * w;
        }
        x_out[f.gbase + j] = x;
        d_out[f.gbase + j] = d;
    }
    if (j == 0) {
        double ld = 0.0, q = 0.0;
        for (int c = 0; c < s; ++c) {
            ld += log(A[c * FS_P + c]);
            q += tt[c] * tt[c];
        }
        stat2[2 * f.fold] = 2.0 * ld;
        stat2[2 * f.fold + 1] = q;
        fail[f.fold] = 0;
    }
}

void ck_launch_fold_small(hipStream_t s, const CkFoldSmall* folds, int64_t n, const double* buf, const int* grow,
                          const double* dots, double* x_out, double* d_out, double* stat2, int* fail) {
    if (n <= 0) return;
    k_fold_small<<<dim3((unsigned)n), dim3(64), 0, s>>>(folds, buf, grow, dots, x_out, d_out, stat2, fail);
}

// everything of a big fold's system outside Q_SS (rows and columns [0, s), written by k_fold_gram before this launch): row r of
// the (kq + 128) x ld storage per workgroup
__global__ __launch_bounds__(256) void k_fold_big_fill(const CkFoldBig* __restrict__ sys, double* __restrict__ buf,
                                                        const int* __restrict__ grow, const double* __restrict__ dots) {
    const CkFoldBig q = sys[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= q.kq + 128) return;
    double* row = buf + q.off + (long)r * q.ld;
    const int s = q.s;
    for (int c = threadIdx.x; c < q.ld; c += 256) {
        if (r < s && c < s) continue;
        double v = 0.0;
        if (r < q.kq) {
            if (r >= s && r < 2 * s) v = c == r - s ? 1.0 : (c == r ? CK_LT_BIG : 0.0);
            else if (r == 2 * s) v = c < s ? dots[grow[q.gbase + c]] : (c == r ? CK_LT_BIG : 0.0);
            else if (r > 2 * s) v = c == r ? 1.0 : 0.0;
        }
        row[c] = v;
    }
}

// one wave per unit row s + q of a factored system
__global__ __launch_bounds__(256) void k_fold_big_reduce(const CkFoldBig* __restrict__ sys, const double* __restrict__ buf,
                                                          const long long* __restrict__ info, double* __restrict__ x_out,
                                                          double* __restrict__ d_out, double* __restrict__ stat2,
                                                          int* __restrict__ fail) {
    const CkFoldBig q = sys[blockIdx.y];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wv;
    const int s = q.s;
    if (m >= s) return;
    const bool bad = info[blockIdx.y] != 0;
    const double* S = buf + q.off;
    const double* t = S + (long)(2 * s) * q.ld;
    const double* w = S + (long)(s + m) * q.ld;
    double x = 0.0, d = 0.0;
    for (int c = lane; c < s; c += 64) {
        const double v = w[c];
        x += v * t[c];
        d += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x += __shfl_xor(x, off);
        d += __shfl_xor(d, off);
    }
    if (lane == 0) {
        x_out[q.gbase + m] = bad ? NAN : x;
        d_out[q.gbase + m] = bad ? NAN : d;
    }
    if (m == 0) {
        double ld = 0.0, qq = 0.0;
        for (int c = lane; c < s; c += 64) {
            ld += log(S[(long)c * q.ld + c]);
            qq += t[c] * t[c];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            ld += __shfl_xor(ld, off);
            qq += __shfl_xor(qq, off);
        }
        if (lane == 0) {
            stat2[2 * q.fold] = bad ? NAN : 2.0 * ld;
            stat2[2 * q.fold + 1] = bad ? NAN : qq;
            fail[q.fold] = bad ? 1 : 0;
        }
    }
}

void ck_launch_fold_big_fill(hipStream_t s, const CkFoldBig* sys, int n_sys, int kq_max, double* buf, const int* grow,
                             const double* dots) {
    if (n_sys <= 0) return;
    k_fold_big_fill<<<dim3((unsigned)(kq_max + 128), (unsigned)n_sys), dim3(256), 0, s>>>(sys, buf, grow, dots);
}

void ck_launch_fold_big_reduce(hipStream_t s, const CkFoldBig* sys, int n_sys, int s_max, const double* buf, const long long* info,
                               double* x_out, double* d_out, double* stat2, int* fail) {
    if (n_sys <= 0) return;
    k_fold_big_reduce<<<dim3((unsigned)((s_max + 3) / 4), (unsigned)n_sys), dim3(256), 0, s>>>(sys, buf, info, x_out, d_out, stat2,
                                                                                             fail);
}
