// ck_blocks.hip -- block (areal) cokriging: the right-hand-side rows and the prior covariance of weighted site sums
// (ck_api.hip: ck_predict_blocks).
//
// A block b is a weighted sum of prediction sites, A[b, a] = w_a.  Its right-hand side is the weighted sum of the point
// rows, c0_b = sum_a w_a c0(s_a) (the point rows come from K2, k_assemble + k_assemble_fix, unchanged), and its prior
// covariance with block c is  Cbar[b, c] = sum_{a in b} sum_{a' in c} w_a w_a' C_ii(h(s_a, s_a'))  with the nugget where
// h == 0 (src/joint_prediction.py:94-102, the point path's C_pp).  Everything else -- the forward substitution, the
// reductions, the Schur product V^T V -- runs through the point path's kernels on the block rows.
//
// Every kernel gives every output element ONE writer and accumulate in a fixed order (no atomics), so that repeated
// calls give the same bits.
#include "ck_internal.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

// ---- block rows -------------------------------------------------------------------------------------------------
// One workgroup per (block row b, panel K); thread t owns the doubles 2t, 2t + 1 of the 512-wide panel row and walks
// the block's members rows[off[b] .. off[b + 1]) in list order (the caller's site order):
//   acc = first ? 0 : out[b];  acc = fma(w_k, aux[rows_k], acc) ...;  out[b] = acc
// so that a block's sum is carried from one chunk of sites to the next in the same order as in one pass.
// b == r: the data row (row zrow of the point rows) is copied; b > r (first chunk only): padding rows are zeroed.
__global__ __launch_bounds__(256) void k_block_fold(const double* __restrict__ aux, long mpad, double* __restrict__ out,
                                                    long mpad_r, const int* __restrict__ off, const int* __restrict__ rows,
                                                    const double* __restrict__ w, long r, long zrow, int first) {
    const long b = blockIdx.x;
    const long K = blockIdx.y;
    const int t = threadIdx.x;
    const double* src = aux + K * mpad * CK_NB + 2 * t;
    d2_t* dst = reinterpret_cast<d2_t*>(out + K * mpad_r * CK_NB + b * CK_NB + 2 * t);
    if (b >= r) {
        if (b == r) *dst = *reinterpret_cast<const d2_t*>(src + zrow * CK_NB);
        else if (first) *dst = d2_t{0.0, 0.0};
        return;
    }
    const int k0 = off[b], k1 = off[b + 1];
    if (!first && k0 == k1) return;   // no member in this chunk: the row stays as the previous chunks left it
    d2_t acc = first ? d2_t{0.0, 0.0} : *dst;
    int k = k0;
    for (; k + 4 <= k1; k += 4) {   // four rows in flight, added in list order
        d2_t x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const d2_t*>(src + (long)rows[k + q] * CK_NB);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double wq = w[k + q];
            acc[0] = fma(wq, x[q][0], acc[0]);
            acc[1] = fma(wq, x[q][1], acc[1]);
        }
    }
    for (; k < k1; ++k) {
        const d2_t x = *reinterpret_cast<const d2_t*>(src + (long)rows[k] * CK_NB);
        acc[0] = fma(w[k], x[0], acc[0]);
        acc[1] = fma(w[k], x[1], acc[1]);
    }
    *dst = acc;
}

void ck_launch_block_fold(hipStream_t s, const double* aux, int64_t mpad, int n_panels, double* out, int64_t mpad_r,
                          const int* off, const int* rows, const double* w, int64_t r, int64_t zrow, int first) {
    if (n_panels <= 0 || r <= 0) return;
    const dim3 grid((unsigned)(first ? mpad_r : r + 1), (unsigned)n_panels);
    k_block_fold<<<grid, dim3(256), 0, s>>>(aux, (long)mpad, out, (long)mpad_r, off, rows, w, (long)r, (long)zrow, first);
}

// ---- block prior covariance ---------------------------------------------------------------------------------------
// Element (R, C) of Cbar is a sum over the n_R x n_C member pairs (p = ia n_C + ic).  The pairs of every element are cut
// into pieces of CK_PRIOR_PIECE consecutive pairs (the host lays out piece offsets poff[e] .. poff[e + 1] per element), so
// that a large block -- a 30-degree band, a whole-domain mean -- is spread over many waves instead of one:
//   k_block_prior_part  one wave per piece: lane l takes the pairs l, l + 64, ... of the piece, evaluates w_a w_c C_ii(h)
//                       with the exact Matern / K_nu of ck_math.h; the 64 partial sums are combined by a fixed butterfly;
//   k_block_prior_sum   one wave per element: lane l takes the pieces l, l + 64, ... in order, fixed butterfly again.
// The partition depends on the block sizes only, so repeated calls give the same bits.  Members are stored block by block
// (off[b] .. off[b + 1]) in exact-formula form.
// full == 0: the diagonal only, element e = (e, e), out to diag[e];
// full != 0: the lower triangle R >= C, element e = R (R + 1) / 2 + C, into the packed panels of the Schur buffers
//            (panel J = C / NB holds rows J NB .., ld = NB) -- the operand layout of k_schur_syrk_d.
__device__ __forceinline__ void prior_element(long e, int full, long& R, long& C) {
    R = C = e;
    if (full) {
        R = (long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (R * (R + 1) / 2 > e) --R;
        while ((R + 1) * (R + 2) / 2 <= e) ++R;
        C = e - R * (R + 1) / 2;
    }
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__global__ __launch_bounds__(256) void k_block_prior_part(const CkMatern* __restrict__ blk, int metric,
                                                          const double* __restrict__ c0, const double* __restrict__ c1,
                                                          const double* __restrict__ c2, const double* __restrict__ w,
                                                          const int* __restrict__ off, const long long* __restrict__ poff,
                                                          long n_elem, int full, long n_pieces, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long piece = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (piece >= n_pieces) return;   // a whole wave leaves together
    long lo = 0, hi = n_elem;        // the element of this piece: poff[lo] <= piece < poff[lo + 1] (every element has a piece)
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (poff[mid] <= piece) lo = mid;
        else hi = mid;
    }
    long R, C;
    prior_element(lo, full, R, C);
    const int a0 = off[R], na = off[R + 1] - a0;
    const int b0 = off[C], nb = off[C + 1] - b0;
    const long p0 = (piece - poff[lo]) * CK_PRIOR_PIECE;
    const long p1 = min(p0 + (long)CK_PRIOR_PIECE, (long)na * nb);
    const CkMatern& m = *blk;   // read in place: a private copy of its coefficient arrays would live in scratch
    double s = 0.0;
    for (long p = p0 + lane; p < p1; p += 64) {
        const int a = a0 + (int)(p / nb);
        const int c = b0 + (int)(p % nb);
        const double h = metric == CK_METRIC_HAVERSINE ? ck_haversine_km(c0[a], c1[a], c2[a], c0[c], c1[c], c2[c])
                                                       : ck_euclid(c0[a], c1[a], c0[c], c1[c]);
        s += (w[a] * w[c]) * ck_cov_entry(m, h, 1);
    }
    s = wave_sum(s);
    if (lane == 0) part[piece] = s;
}

__global__ __launch_bounds__(256) void k_block_prior_sum(const long long* __restrict__ poff, const double* __restrict__ part,
                                                         long n_elem, int full, double* __restrict__ diag,
                                                         double* const* __restrict__ panels) {
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_elem) return;
    double s = 0.0;
    for (long q = poff[e] + lane; q < poff[e + 1]; q += 64) s += part[q];
    s = wave_sum(s);
    if (lane != 0) return;
    if (!full) {
        diag[e] = s;
    } else {
        long R, C;
        prior_element(e, full, R, C);
        const long J = C / CK_NB;
        panels[J][(R - J * CK_NB) * CK_NB + (C - J * CK_NB)] = s;
    }
}

void ck_launch_block_prior(hipStream_t s, const CkMatern* blk, int metric, const double* c0, const double* c1,
                           const double* c2, const double* w, const int* off, int64_t r, int full, const long long* poff,
                           int64_t n_pieces, double* part, double* diag, double* const* panels) {
    const int64_t n_elem = full ? r * (r + 1) / 2 : r;
    if (n_elem <= 0 || n_pieces <= 0) return;
    k_block_prior_part<<<dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, s>>>(blk, metric, c0, c1, c2, w, off, poff,
                                                                                (long)n_elem, full, (long)n_pieces, part);
    k_block_prior_sum<<<dim3((unsigned)((n_elem + 3) / 4)), dim3(256), 0, s>>>(poff, part, (long)n_elem, full, diag, panels);
}
