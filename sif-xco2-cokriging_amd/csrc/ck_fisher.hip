// ck_fisher.hip -- the expected (Fisher) information of the likelihood fit (ck_loglik_fisher, ck_api.hip).
//
//   I_jk = 1/2 tr(Sigma^-1 D_j Sigma^-1 D_k),   D_k = dSigma / dtheta_k
//
// Every D_k is a fixed linear combination of thirteen OPERANDS (ck_internal.h: CK_FOP_*): per Matern block the correlation,
// its derivatives in nu and in the length scale (times the block's amplitude) and -- inside a process -- the 0 / 1 pattern of
// h == 0 (the nugget), and per process diag(d_a) (the noise scale).  The information of the operands, T_ab = 1/2 tr(Sigma^-1
// D_a Sigma^-1 D_b), is computed here; the host combines it (ck_host.cpp: ck_host_fisher_combine).  Plain form:
//   B_a = Sigma^-1 D_a  on the FP64 MFMA tile (ck_la.hip: k_fisher_prod), restricted to the columns D_a lives in;
//   T_ab = 1/2 sum_pq B_a[p,q] B_b[q,p]  (k_fisher_contract: fixed order, one partial vector per workgroup, no atomics).
// The two diagonal operands need no product: B[p,q] = Sigma^-1[p,q] d_q is formed where it is read.
//
//   k_fisher_expand    the lower packed block columns of -Sigma^-1 (k_ginv_syrk_d with a zero start) -> the full symmetric
//                      Sigma^-1 as K-panels (panel P: Npad rows of the 512 columns P NB ..; zero in rows / columns of padding)
//   k_fisher_assemble  one pass over the site pairs of the lower triangle, one ck_matern_grad call per pair with k_loglik_grad's
//                      distance, h == 0 test and nu +- dnu neighbours: entry for entry the matrices whose contraction with G
//                      is ck_loglik's gradient.  Written as the product kernel's second operand (CkFisherUnit).
//   k_fisher_dh, k_fisher_dh_diag, k_fisher_ytv   the thin REML terms: Y_a = D_a H and Y^T V, Y^T H over the sites.
#include "ck_internal.h"

__device__ __forceinline__ bool fi_valid(const CkLayout& L, long g) { return g < L.n0 || (g >= L.n0p && g < L.nend); }

// ---- Sigma^-1 as full K-panels ------------------------------------------------------------------------------------
// grid (Npad / 8, nK), 256 threads: 8 rows of one panel.  Entry (r, c): from the lower triangle at (max, min).
__global__ __launch_bounds__(256) void k_fisher_expand(double* const* __restrict__ G, CkLayout L, double* __restrict__ Sp) {
    const long pc = blockIdx.y;
    for (int i = 0; i < 8; ++i) {
        const long r = (long)blockIdx.x * 8 + i;
        const bool vr = fi_valid(L, r);
        for (int k = threadIdx.x; k < CK_NB; k += 256) {
            const long c = pc * CK_NB + k;
            double v = 0.0;
            if (vr && fi_valid(L, c)) {
                const long a = r >= c ? r : c, b = r >= c ? c : r;
                const long J = b / CK_NB;
                v = -G[J][(a - J * CK_NB) * CK_NB + (b - J * CK_NB)];
            }
            Sp[(pc * L.npad + r) * CK_NB + k] = v;
        }
    }
}

void ck_launch_fisher_expand(hipStream_t s, double* const* G_dev, CkLayout L, double* Sp) {
    const int nK = (int)(L.npad / CK_NB);
    if (nK <= 0) return;
    k_fisher_expand<<<dim3((unsigned)(L.npad / 8), (unsigned)nK), dim3(256), 0, s>>>(G_dev, L, Sp);
}

// ---- derivative assembly ----------------------------------------------------------------------------------------------
// k_loglik_grad's launch shape: one workgroup per 64-row strip of a block column, a wave on 64 consecutive columns of one row
// (one Matern block).  Entry (n, k) of a unit: D[((k / NB - pK0) wpad + (n - c0)) NB + k % NB].
// r: the process of the column n (the unit), kp: the process of the row k (its K-panels)
__device__ __forceinline__ void fi_put(const CkFisherAsm& A, int op, int r, int kp, long n, long k, double v) {
    double* D = A.D[op][r];
    if (D) D[((k / CK_NB - A.pK0[kp]) * A.wpad[r] + (n - A.c0[r])) * CK_NB + (k % CK_NB)] = v;
}

__global__ __launch_bounds__(256) void k_fisher_assemble(CkFisherAsm A, CkLayout L, int n_procs, int metric,
                                                          const double* __restrict__ c, const CkMatern* __restrict__ blk5,
                                                          double dnu0, double dnu1, double dnu2) {
    const long strips = L.npad / 64;
    const int J = (int)(blockIdx.x / strips);
    const long t = (long)blockIdx.x - (long)J * strips;
    const long p0 = (long)J * CK_NB + t * 64;
    if (p0 >= L.nend) return;
    const double* c0 = c;
    const double* c1 = c + L.npad;
    const double* c2 = c + 2 * L.npad;
    for (int k = 0; k < 128; ++k) {
        const int e = threadIdx.x + 256 * k;
        const long p = p0 + (e >> 9);
        const long q = (long)J * CK_NB + (e & 511);
        if (q > p || !fi_valid(L, p) || !fi_valid(L, q)) continue;
        const int pp = p >= L.n0p && n_procs == 2 ? 1 : 0, pq = q >= L.n0p && n_procs == 2 ? 1 : 0;
        const int b = pp + pq;
        const int op0 = b == 0 ? CK_FOP_R00 : b == 2 ? CK_FOP_R11 : CK_FOP_R01;
        if (b == 1) {   // (wave-uniform) nothing of this block is wanted
            if (!A.D[op0][0] && !A.D[op0 + 1][0] && !A.D[op0 + 2][0]) continue;
        } else if (!A.D[op0][pp] && !A.D[op0 + 1][pp] && !A.D[op0 + 2][pp] && !A.D[op0 + 3][pp]) {
            continue;
        }
        const double h = metric == CK_METRIC_HAVERSINE ? ck_haversine_km(c0[p], c1[p], c2[p], c0[q], c1[q], c2[q])
                                                       : ck_euclid(c0[p], c1[p], c0[q], c1[q]);
        const CkMatern& m = blk5[5 * b];
        const double dnu = b == 0 ? dnu0 : b == 1 ? dnu1 : dnu2;
        const CkMaternGrad gr = ck_matern_grad(m, blk5 + 5 * b + 1, dnu, h);
        const double v[4] = {gr.M, m.amp * gr.dnu, m.amp * gr.dlen, h == 0.0 ? 1.0 : 0.0};
        if (b == 1) {   // p in process 1, q in process 0: unit 0 has its columns n in process 0, unit 1 in process 1
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                fi_put(A, op0 + o, 0, 1, q, p, v[o]);
                fi_put(A, op0 + o, 1, 0, p, q, v[o]);
            }
        } else {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                fi_put(A, op0 + o, pp, pp, p, q, v[o]);
                if (p != q) fi_put(A, op0 + o, pp, pp, q, p, v[o]);
            }
        }
    }
}

void ck_launch_fisher_assemble(hipStream_t s, const CkFisherAsm& A, CkLayout L, int n_procs, int metric, const double* c,
                               const CkMatern* blk5, const double* dnu3) {
    const int64_t n = (L.npad / CK_NB) * (L.npad / 64);
    if (n <= 0) return;
    k_fisher_assemble<<<dim3((unsigned)n), dim3(256), 0, s>>>(A, L, n_procs, metric, c, blk5, dnu3[0], dnu3[1], dnu3[2]);
}

// ---- contraction ------------------------------------------------------------------------------------------------------
// One workgroup per 32-row strip P of the matrices; it walks the 32 x 32 tiles (P, Q) of the strip.  Thread (tx, ty) holds
// B_a[p, q] of its four entries p = P + ty + 8 e, q = Q + tx for every operand a; the mirrored tile B_b[Q .., P ..] of one
// operand at a time goes through LDS (read coalesced, used transposed).  part[wg][a (a + 1) / 2 .. ]: sums of
// B_a[p, q] B_b[q, p] for the pairs a <= b whose bit is set in mask[a]; the host adds the workgroups in order and halves.
__device__ __forceinline__ double fi_entry(const CkFisherOp& o, const CkFisherCtx& X, long r, long c) {
    if (o.kind == CK_FOPK_DENSE) return c >= o.c0 && c < o.c0 + o.w ? o.B[r * o.ld + (c - o.c0)] : 0.0;
    // diagonal operand of process kind - 2: -Sigma^-1[r, c] d_c (the sign of the stored products)
    const int proc = X.n_procs == 2 && c >= X.n0p ? 1 : 0;
    if (proc != o.kind - CK_FOPK_DIAG0) return 0.0;
    return -X.Sp[((c / CK_NB) * X.npad + r) * CK_NB + (c % CK_NB)] * X.d[c];
}

__global__ __launch_bounds__(256) void k_fisher_contract(CkFisherOps O, CkFisherCtx X, double* __restrict__ part) {
    __shared__ double tile[32][33];
    __shared__ double red[4][CK_FISHER_NPAIR];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long P = (long)blockIdx.x * 32;
    double acc[CK_FISHER_NPAIR];
#pragma unroll
    for (int k = 0; k < CK_FISHER_NPAIR; ++k) acc[k] = 0.0;
    unsigned anyb = 0;   // operands that are the second of some pair
#pragma unroll
    for (int a = 0; a < CK_FISHER_NOPS; ++a) anyb |= O.mask[a];
    for (long Q = 0; Q < X.npad; Q += 32) {
        double dir[CK_FISHER_NOPS][4];
#pragma unroll
        for (int a = 0; a < CK_FISHER_NOPS; ++a) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dir[a][e] = 0.0;
            if (O.mask[a] != 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dir[a][e] = fi_entry(O.op[a], X, P + ty + 8 * e, Q + tx);
            }
        }
#pragma unroll
        for (int b = 0; b < CK_FISHER_NOPS; ++b) {
            if (!((anyb >> b) & 1u)) continue;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[ty + 8 * e][tx] = fi_entry(O.op[b], X, Q + ty + 8 * e, P + tx);
            __syncthreads();
            double tr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) tr[e] = tile[tx][ty + 8 * e];   // B_b[Q + tx, P + ty + 8 e]
#pragma unroll
            for (int a = 0; a <= b; ++a) {
                if (!((O.mask[a] >> b) & 1u)) continue;
                double s = dir[a][0] * tr[0];
                s += dir[a][1] * tr[1];
                s += dir[a][2] * tr[2];
                s += dir[a][3] * tr[3];
                acc[b * (b + 1) / 2 + a] += s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CK_FISHER_NPAIR; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        acc[k] = v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < CK_FISHER_NPAIR; ++k) red[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < CK_FISHER_NPAIR) {
        const int k = threadIdx.x;
        part[(long)blockIdx.x * CK_FISHER_NPAIR + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

int64_t ck_fisher_contract_groups(int64_t npad) { return npad / 32; }

void ck_launch_fisher_contract(hipStream_t s, const CkFisherOps& O, const CkFisherCtx& X, double* part) {
    const int64_t n = ck_fisher_contract_groups(X.npad);
    if (n <= 0) return;
    k_fisher_contract<<<dim3((unsigned)n), dim3(256), 0, s>>>(O, X, part);
}

// ---- the thin REML terms ---------------------------------------------------------------------------------------------
// Y_a = D_a H (H = Sigma^-1 X, Npad x p row-major) for one unit of a dense operand, one wave per column n of the unit (D_a is
// symmetric: the unit's row n is row c0 + n of D_a).  Written as K-panels of CK_FISHER_YROWS rows: Yp[(g / NB) YROWS + row0 + j]
// [g % NB] = Y_a[g, j], the product kernel's second operand for V = Sigma^-1 Y.
__global__ __launch_bounds__(256) void k_fisher_dh(CkFisherUnit U, const double* __restrict__ H, int p, int row0,
                                                    double* __restrict__ Yp) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long g = U.c0 + n;
    if (n >= U.wpad || g < U.nlo || g >= U.nhi) return;   // (wave-uniform)
    double acc[CK_LU_PMAX];
#pragma unroll
    for (int j = 0; j < CK_LU_PMAX; ++j) acc[j] = 0.0;
    for (int pp = 0; pp < U.npan; ++pp) {
        const double* row = U.D + ((long)pp * U.wpad + n) * CK_NB;
        const long k0 = (long)(U.pK0 + pp) * CK_NB;
        for (int i = 0; i < CK_NB / 64; ++i) {
            const int k = lane + 64 * i;
            const double dv = row[k];
            const double* hr = H + (k0 + k) * p;
#pragma unroll
            for (int j = 0; j < CK_LU_PMAX; ++j)
                if (j < p) acc[j] += dv * hr[j];
        }
    }
#pragma unroll
    for (int j = 0; j < CK_LU_PMAX; ++j) {
        double v = acc[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0 && j < p) Yp[((g / CK_NB) * CK_FISHER_YROWS + row0 + j) * CK_NB + (g % CK_NB)] = v;
    }
}

void ck_launch_fisher_dh(hipStream_t s, const CkFisherUnit& U, const double* H, int p, int row0, double* Yp) {
    if (U.wpad <= 0 || p <= 0) return;
    k_fisher_dh<<<dim3((unsigned)((U.wpad + 3) / 4)), dim3(256), 0, s>>>(U, H, p, row0, Yp);
}

// the diagonal operand of process `proc`: Y[g, j] = d_g H[g, j]
__global__ __launch_bounds__(256) void k_fisher_dh_diag(CkLayout L, int n_procs, int proc, const double* __restrict__ d,
                                                         const double* __restrict__ H, int p, int row0, double* __restrict__ Yp) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.npad || !fi_valid(L, g)) return;
    if ((n_procs == 2 && g >= L.n0p ? 1 : 0) != proc) return;
    for (int j = 0; j < p; ++j) Yp[((g / CK_NB) * CK_FISHER_YROWS + row0 + j) * CK_NB + (g % CK_NB)] = d[g] * H[g * p + j];
}

void ck_launch_fisher_dh_diag(hipStream_t s, CkLayout L, int n_procs, int proc, const double* d, const double* H, int p, int row0,
                              double* Yp) {
    if (p <= 0) return;
    k_fisher_dh_diag<<<dim3((unsigned)((L.npad + 255) / 256)), dim3(256), 0, s>>>(L, n_procs, proc, d, H, p, row0, Yp);
}

// out[a ldo + c] = sum_g Y[g, a] R[g ldr + c] over the sites g in ascending order, a < CK_FISHER_YROWS (one workgroup each),
// c < ncols <= 256
__global__ __launch_bounds__(256) void k_fisher_ytv(const double* __restrict__ Yp, long npad, const double* __restrict__ R,
                                                     long ldr, int ncols, double* __restrict__ out, long ldo) {
    const int a = blockIdx.x, c = threadIdx.x;
    if (c >= ncols) return;
    double s = 0.0;
    for (long P = 0; P < npad / CK_NB; ++P) {
        const double* y = Yp + (P * CK_FISHER_YROWS + a) * CK_NB;
        const double* r = R + P * CK_NB * ldr + c;
        for (int k = 0; k < CK_NB; ++k) s += y[k] * r[(long)k * ldr];
    }
    out[(long)a * ldo + c] = s;
}

void ck_launch_fisher_ytv(hipStream_t s, const double* Yp, int64_t npad, const double* R, int64_t ldr, int ncols, double* out,
                          int64_t ldo) {
    if (ncols <= 0) return;
    k_fisher_ytv<<<dim3(CK_FISHER_YROWS), dim3(256), 0, s>>>(Yp, (long)npad, R, (long)ldr, ncols, out, (long)ldo);
}
