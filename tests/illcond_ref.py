"""Ill-conditioned data sets and their extended-precision references for tests/test_illcond_host.py and
tests/test_gpu_illcond.py ("Stability of the inverse-based row solves").  Host only: numpy, the oracle's
covariances; no GPU and no library call.

The blocked factorisations of csrc/ck_la.hip and csrc/ck_local.hip solve their rows X L_jj^T = A as X = A W^T with W an
explicit inverse of the 64 x 64 diagonal block.  With W computed column by column, |L_jj W - I| <= gamma_64 |L_jj| |W| (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., ch. 14: the right residual of a computed triangular inverse), so
the computed rows satisfy X L_jj^T = A (L_jj W)^T = A + dA with |dA| of the order u |A| |W^T| |L_jj^T|, normwise
u kappa(L_jj) |A|, where a substitution gives u |X| |L_jj^T|.  Inserted into the error analysis of the blocked Cholesky
(Higham, Theorem 10.3) the componentwise bound gamma_{N+1} |L| |L^T| of a plain factorisation becomes

    |Sigma - L L^T| <= gamma_{N+1} (1 + kappa_blk) |L| |L^T|,      kappa_blk = max_j cond_2(L_jj)            (block bound)

over the diagonal blocks as the device cuts them.  (The device builds W on two levels -- inverse_two_level below --, whose right
residual carries the condition of the 16 x 16 diagonal blocks as a further factor; it stays under the block bound on every set
here, and emulate_inverse_blocked has both forms.)  Everything here that serves as truth is np.longdouble (the x87 80-bit
format where the tests run, eps 1.08e-19; the host test asserts eps < 2e-19); u = 2^-53 is the device's unit roundoff."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla

from oracle import cokrige_oracle as orc

LD = np.longdouble
U = 2.0 ** -53
EUC = 1
EPS_C = 5e-13     # the project's entry tolerance of the covariance (tests/test_gpu_joint.py: exact assembly against the oracle)
BLOCK = 64

_NEARDUP = [.99, .81, .7, 1.5, 2.2, 2.5, 2.5, 2.5, 1e-9, 1e-9, .3]
# name: (n0, n1, flat parameters (the order of tests/dense_chains.py), clusters, spread)
SETS = {
    "WELL": (130, 126, [.99, .81, .7, 1.5, 2.2, 2.5, 2.5, 2.5, .02, .025, .3], 256, 3.0),
    "SMOOTH": (130, 126, [.99, .81, 2.5, 2.5, 2.5, 6, 6, 6, 1e-8, 1e-8, .3], 40, 0.3),
    "NEARDUP": (130, 126, _NEARDUP, 30, 1e-3),
    "NEARDUP_PANELS": (513, 511, _NEARDUP[:8] + [1e-8, 1e-8, .3], 100, 1e-3),
    "UNI65": (65, 0, [_NEARDUP[0], _NEARDUP[2], _NEARDUP[5], _NEARDUP[8]], 30, 1e-3),   # process 0 of NEARDUP, its first 65 sites
}
HARD = ["SMOOTH", "NEARDUP", "NEARDUP_PANELS"]


def gamma(n):
    return n * U / (1.0 - n * U)


def sites(clusters, spread, n):
    """the recipe of the experiment: cluster centres uniform on [0, 10]^2, every site a centre plus spread x N(0, I)"""
    rng = np.random.default_rng(3)
    centres = rng.uniform(0, 10, (clusters, 2))
    return centres[rng.integers(0, clusters, n)] + spread * rng.standard_normal((n, 2))


class DataSet:
    """coords, values (z = L_ref eps: the model's own draws), the oracle's Sigma in the caller's order and its reference"""

    def __init__(self, name):
        n0, n1, params, clusters, spread = SETS[name]
        self.name, self.n0, self.n1, self.N = name, n0, n1, n0 + n1
        self.params = list(params)
        self.p = orc.Params.from_flat(self.params)
        pts = sites(clusters, spread, 256 if name == "UNI65" else n0 + n1)   # UNI65: the first sites of NEARDUP
        self.coords = [pts[:n0]] if n1 == 0 else [pts[:n0], pts[n0:n0 + n1]]
        self.S = orc.joint_cov(self.p, self.coords, EUC)
        self.ref = Reference(self.S, blocks(n0, n1))
        eps = np.random.default_rng(11).standard_normal(self.N)
        self.z = np.asarray(matvec_ld(self.ref.L, eps), dtype=np.float64)
        self.values = [self.z[:n0]] if n1 == 0 else [self.z[:n0], self.z[n0:]]


@functools.lru_cache(maxsize=None)
def data_set(name):
    return DataSet(name)


def blocks(n0, n1=0):
    """the 64-blocks as the device cuts them: every process starts a block of its own (the device pads process 0 to a multiple
    of 64 with unit diagonals, which decouple), as slices of the compact stacked index in the handle's internal order"""
    out = []
    for a, n in ((0, n0), (n0, n1)):
        out += [slice(a + b, a + min(b + BLOCK, n)) for b in range(0, n, BLOCK)]
    return out


# ---- longdouble arithmetic ---------------------------------------------------------------------------------------------------
def chol_ld(S):
    """column Cholesky in np.longdouble; raises numpy's LinAlgError at a pivot that is not positive"""
    A = np.array(S, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"leading minor {j + 1} is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def solve_lower_ld(L, B, trans=False):
    """L^-1 B (trans: L^-T B) by substitution in longdouble; B a vector or a matrix"""
    L = np.asarray(L, dtype=LD)
    X = np.array(B, dtype=LD)
    n = L.shape[0]
    if not trans:
        for j in range(n):
            X[j] = X[j] / L[j, j]
            if j + 1 < n:
                X[j + 1:] -= np.multiply.outer(L[j + 1:, j], X[j]) if X.ndim == 2 else L[j + 1:, j] * X[j]
    else:
        for j in range(n - 1, -1, -1):
            X[j] = X[j] / L[j, j]
            if j > 0:
                X[:j] -= np.multiply.outer(L[j, :j], X[j]) if X.ndim == 2 else L[j, :j] * X[j]
    return X


def matvec_ld(A, x):
    return np.dot(np.asarray(A, dtype=LD), np.asarray(x, dtype=LD))


def _tiles(n, t=128):
    return [(i, min(i + t, n), j, min(j + t, n)) for i in range(0, n, t) for j in range(0, i + 1, t)]


def llt_ld(L):
    """L L^T in longdouble, the lower triangle's tiles only (mirrored), on a few threads: numpy's longdouble loops hold no lock"""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    out = np.zeros((n, n), dtype=LD)

    def one(t):
        i0, i1, j0, j1 = t
        k = j1   # L is lower triangular: columns beyond the tile's last column index contribute nothing
        out[i0:i1, j0:j1] = np.dot(L[i0:i1, :k], L[j0:j1, :k].T)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, _tiles(n)))
    return np.tril(out) + np.tril(out, -1).T


def sym_from_lower(low):
    low = np.asarray(low)
    return np.tril(low) + np.tril(low, -1).T


# ---- the reference of one matrix ------------------------------------------------------------------------------------------------
class Reference:
    """Of a float64 symmetric S: the longdouble factor L, |L||L^T| (float64 product of the rounded factor: non-negative terms,
    relative error gamma_N, nothing against the bounds it scales), kappa_blk, cond_2(S), and the asserted bounds."""

    def __init__(self, S, blks):
        self.S = np.asarray(S, dtype=np.float64)
        self.N = self.S.shape[0]
        self.blks = blks
        self.L = chol_ld(self.S)
        self.L64 = np.asarray(self.L, dtype=np.float64)
        self.absLLt = np.abs(self.L64) @ np.abs(self.L64).T
        self.kappa_blk = kappa_blk(self.L, blks)
        self.cond2 = float(np.linalg.cond(self.S, 2))
        self.normS = float(np.linalg.norm(self.S, 2))

    def bound_b(self, with_kappa=True):
        """the block bound on |S - L L^T|, componentwise (with_kappa = False: Higham's gamma_{N+1} |L||L^T|)"""
        return gamma(self.N + 1) * ((1.0 + self.kappa_blk) if with_kappa else 1.0) * self.absLLt

    def inverse_abs(self):
        """|S^-1| in float64 from the longdouble factor rounded (its error, cond(S) u relative normwise, scales a bound only)"""
        Li = sla.solve_triangular(self.L64, np.eye(self.N), lower=True)
        return np.abs(Li.T @ Li)

    def solve(self, b):
        """S^-1 b in longdouble through the factor"""
        return solve_lower_ld(self.L, solve_lower_ld(self.L, b), trans=True)

    def logdet(self):
        return float(2 * np.sum(np.log(np.diag(self.L))))

    def quad(self, z):
        y = solve_lower_ld(self.L, z)
        return float(np.dot(y, y))


def kappa_blk(L, blks):
    """max_j cond_2(L_jj) over the diagonal blocks of the (longdouble) factor; the SVD runs on the block rounded to float64,
    which moves a condition number below 1e8 by less than 1e-8 of itself"""
    return max(float(np.linalg.cond(np.asarray(L[b, b], dtype=np.float64), 2)) for b in blks)


# ---- the yardstick: what a correct inverse-based kernel does ----------------------------------------------------------------------
def inverse_two_level(T, nb=16):
    """potrf64_body's inverse of a lower triangular block (csrc/ck_la.hip): the nb x nb diagonal blocks by substitution on the
    identity, the blocks below them by distance from the diagonal as W_ij = -W_ii (sum_{k = j}^{i - 1} T_ik W_kj) -- a product
    with the inverse W_ii once more, where a substitution with T_ii would stand in a one-level scheme"""
    n = T.shape[0]
    W = np.zeros((n, n))
    bl = [slice(a, min(a + nb, n)) for a in range(0, n, nb)]
    for b in bl:
        W[b, b] = sla.solve_triangular(T[b, b], np.eye(b.stop - b.start), lower=True)
    for d in range(1, len(bl)):
        for j in range(len(bl) - d):
            i = j + d
            W[bl[i], bl[j]] = -(W[bl[i], bl[i]] @ sum(T[bl[i], bl[k]] @ W[bl[k], bl[j]] for k in range(j, i)))
    return W


def emulate_inverse_blocked(S, blks, correct=False, two_level=False):
    """Right-looking blocked Cholesky in float64 as the kernels organise it: per diagonal block L_jj = chol(A_jj), W = L_jj^-1
    explicitly (substitution on the identity; two_level: inverse_two_level, what the device does), the rows below as the
    product X = A W^T, then A -= X X^T on everything behind.  correct: one correction step X += (A - X L_jj^T) W^T.
    Raises LinAlgError where a block fails to factor."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    for b in blks:
        Ljj = np.linalg.cholesky(A[b, b])
        L[b, b] = Ljj
        if b.stop < n:
            W = inverse_two_level(Ljj) if two_level else sla.solve_triangular(Ljj, np.eye(Ljj.shape[0]), lower=True)
            R = A[b.stop:, b]
            X = R @ W.T
            if correct:
                X = X + (R - X @ Ljj.T) @ W.T
            L[b.stop:, b] = X
            A[b.stop:, b.stop:] -= X @ X.T
    return L


# ---- residuals, all in longdouble ------------------------------------------------------------------------------------------------
def factor_errors(ref, L):
    """(componentwise, normwise) backward error of a float64 factor L of ref.S:
    max_ij |S - L L^T|_ij / (|L_ref||L_ref^T|)_ij and ||S - L L^T||_2 / ||S||_2, with |S - L L^T| itself"""
    R = np.asarray(np.asarray(ref.S, dtype=LD) - llt_ld(L), dtype=np.float64)
    Ra = np.abs(R)
    return float(np.max(Ra / ref.absLLt)), float(np.linalg.norm(R, 2) / ref.normS), Ra


def solve_residual(S, x, z):
    """|z - S x| in longdouble, rounded"""
    return np.asarray(np.abs(np.asarray(z, dtype=LD) - matvec_ld(S, x)), dtype=np.float64)


# ---- the local solvers: NEARDUP with every neighbourhood the whole subset ----------------------------------------------------------
MAX_DIST = 100.0   # beyond the domain [0, 10]^2 and its clusters' spread: every datum is every site's neighbour


def pred_sites(m=7):
    return np.random.default_rng(5).uniform(0.5, 9.5, (m, 2))


class LocalSystem:
    """The first n0 / n1 sites of NEARDUP's processes as one neighbourhood, in the caller's order (process 0 first: the order of
    the local kernels' neighbour list with option site_order = 0): the oracle's Sigma_loc, its longdouble factor, and per
    prediction site of process i the oracle's c, w = Sigma_loc^-1 c, pred and the variance in longdouble.  blks: the 64-blocks
    of the tiled route (it cuts the compacted list, processes not padded apart), or None for a solver without a block inverse."""

    def __init__(self, n0, n1, i, pc, tiled):
        ds = data_set("NEARDUP")
        self.coords = [ds.coords[0][:n0], ds.coords[1][:n1]]
        self.values = [ds.values[0][:n0], ds.values[1][:n1]]
        self.k, self.i, self.pc = n0 + n1, i, np.asarray(pc, dtype=np.float64)
        S = orc.joint_cov(ds.p, self.coords, EUC)
        self.ref = Reference(S, blocks(self.k, 0) if tiled else [slice(0, self.k)])
        self.kappa = self.ref.kappa_blk if tiled else 0.0
        self.c = orc.pred_cross_cov(ds.p, self.coords, self.pc, i, EUC)            # k x m
        self.z = np.concatenate(self.values)
        self.c0 = float(ds.p.sigma[i] ** 2 + ds.p.nugget[i])
        self.w = self.ref.solve(self.c)                                          # k x m, longdouble
        self.a = self.ref.solve(self.z)
        self.pred = np.asarray(np.dot(self.w.T, np.asarray(self.z, dtype=LD)), dtype=np.float64)
        self.var = np.asarray(LD(self.c0) - np.sum(self.w * np.asarray(self.c, dtype=LD), axis=0), dtype=np.float64)

    def weight_bound(self, t):
        """on |c - Sigma_loc w| of site t for a substitution-based solver (Higham, Theorem 10.4: gamma_{3k+1} |L||L^T| |w|) whose
        Sigma_loc and c carry the entry tolerance EPS_C"""
        w = np.abs(np.asarray(self.w[:, t], dtype=np.float64))
        return (gamma(3 * self.k + 1) * self.ref.absLLt + EPS_C * np.abs(self.ref.S)) @ w + EPS_C * np.abs(self.c[:, t])

    def forward_bounds(self, kq):
        """first-order forward bounds on pred and pred_err^2 per site from the same two terms:
        |d pred| <= |w|^T (gamma_{3 kq + 1} (1 + kappa) |L||L^T| + EPS_C |Sigma|) |a| + EPS_C |c|^T |a|,  a = Sigma^-1 z,
        and with c in place of z (a = w) for the variance"""
        E = gamma(3 * kq + 1) * (1.0 + self.kappa) * self.ref.absLLt + EPS_C * np.abs(self.ref.S)
        w = np.abs(np.asarray(self.w, dtype=np.float64))
        a = np.abs(np.asarray(self.a, dtype=np.float64))
        bp = w.T @ (E @ a) + EPS_C * (np.abs(self.c).T @ a)
        bv = np.sum(w * (E @ w), axis=0) + EPS_C * np.sum(np.abs(self.c) * w, axis=0)
        return bp, bv

    def lapack(self):
        """(pred, variance) of a float64 LAPACK solve of the same systems: the yardstick of the recorded ratios"""
        cf = sla.cho_factor(self.ref.S, lower=True)
        w = sla.cho_solve(cf, self.c)
        return w.T @ self.z, self.c0 - np.sum(w * self.c, axis=0)
