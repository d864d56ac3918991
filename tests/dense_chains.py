"""Dense float64 reference chains for the likelihood, REML, universal, block, conditional-draw, Fisher-information and
leave-group-out entry points, and the list of data sets tests/test_gpu_entry_edge_sizes.py and
tests/test_gpu_newer_entry_edge_sizes.py run them on.  Plain numpy / scipy on the oracle's covariances
(oracle/cokrige_oracle.py: joint_cov, pred_cross_cov, pred_cov) in the caller's site order; no GPU, no library call except
where a function takes the library's site order as an argument.  tests/test_dense_chains.py checks these references
themselves, and the conditioning of every data set below, on the host."""
import functools

import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc

HAV, EUC = 0, 1
PARAMS = {
    "BIV": [0.99, 0.81, 0.39, 0.75, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19],
    "BIV_EUC": [0.99, 0.81, 0.7, 1.5, 2.2, 2.5, 2.5, 2.5, 0.02, 0.025, 0.3],
    "BIV_HALF": [1.1, 0.9, 1.5, 1.5, 0.5, 400.0, 450.0, 300.0, 0.03, 0.02, 0.0],   # nu = 1.5 / 0.5 exactly, rho = 0
    "UNI": [1.1, 0.6, 380.0, 0.03],
}

# ---- the size ladder (from CkLayout: n0p = roundup(n0, 64), panels of 512) ------------------------------------------------
LADDER_BIV = [(1, 1), (5, 3), (63, 65), (64, 64), (64, 1), (448, 64), (449, 63), (511, 1), (512, 512), (513, 511), (1, 600)]
LADDER_UNI = [1, 64, 65, 512, 513]
# (n0, n1, seed, name of the parameter set, metric); n1 = 0: one process
LIK_CASES = ([(n0, n1, 40, "BIV", HAV) for n0, n1 in LADDER_BIV]
             + [(63, 65, 40, "BIV_EUC", EUC), (513, 511, 40, "BIV_EUC", EUC), (513, 511, 40, "BIV_HALF", HAV)]
             + [(n0, 0, 40, "UNI", HAV) for n0 in LADDER_UNI])
FIVE_RUNGS = [(5, 3, 40, "BIV", HAV), (63, 65, 40, "BIV", HAV), (448, 64, 40, "BIV", HAV), (513, 511, 40, "BIV", HAV),
              (65, 0, 40, "UNI", HAV)]
SMALL, LARGE = (63, 65, 40, "BIV", HAV), (513, 511, 40, "BIV", HAV)
REFIT = (700, 650, 40, "BIV", HAV)   # the size the older tests use: the last set_data step of the sequence test
REFIT_UNI = (700, 0, 40, "UNI", HAV)   # the univariate half of REFIT's sizes
# Fisher information: every rung, n0p = 576 (the boundary mid-tile in the second panel), three panels with the other metric
# and with rho = 0 (nu_12 and len_12 dead), one process down to N = 1
FISHER_CASES = ([(n0, n1, 40, "BIV", HAV) for n0, n1 in LADDER_BIV] + [(576, 100, 40, "BIV", HAV)]
                + [(513, 511, 40, "BIV_EUC", EUC), (513, 511, 40, "BIV_HALF", HAV)] + [(n0, 0, 40, "UNI", HAV) for n0 in LADDER_UNI])
FISHER_WIDE = [LARGE, SMALL]   # REML with eight columns per process, p = 16
FISHER_NOISE_CASES = [SMALL, (449, 63, 40, "BIV", HAV), (512, 512, 40, "BIV", HAV), LARGE, (64, 1, 40, "BIV", HAV),
                      (1, 600, 40, "BIV", HAV), (65, 0, 40, "UNI", HAV)]
NOISE_SCALES = (1.7, 0.6)
NOISE_CASES = [SMALL, (449, 63, 40, "BIV", HAV), (512, 512, 40, "BIV", HAV), (64, 1, 40, "BIV", HAV), (1, 600, 40, "BIV", HAV)]
# leave-group-out folds: (data set, predicted process) for every process that has data
FOLD_CASES = ([((n0, n1, 40, "BIV", HAV), i) for n0, n1 in LADDER_BIV for i in (0, 1)]
              + [((n0, 0, 40, "UNI", HAV), 0) for n0 in (1, 64, 65, 513)])
FOLD_VARIANTS = [(False, False), (True, False), (True, True)]   # (labels on the other process, some data labelled -1)
# every data set the GPU modules use: the host test checks that Sigma factors and cond(Sigma) < 1e8 for each of them
DATA_CASES = list(dict.fromkeys(LIK_CASES + FIVE_RUNGS + [(64, 64, 40, "BIV", HAV), SMALL, LARGE, REFIT] + FISHER_CASES
                                + FISHER_NOISE_CASES + NOISE_CASES + [c for c, _ in FOLD_CASES] + [REFIT_UNI]))

# conditional draws: (data set, predicted process, m, sites on data of that process, seed of the sites)
DRAW_M = [1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025]


def _n_on(m, k):
    return 20 if m >= 129 else (1 if m == 1 else 1 + k % 3)   # m = 1: the only site is on a datum -- everything deflated


DRAW_CASES = [(data, (k + d) % 2, m, _n_on(m, k), 500 + 10 * k + d)
              for d, data in enumerate((SMALL, LARGE)) for k, m in enumerate(DRAW_M)]
# (n_draws, draw_chunk): one chunk; 128 + 128 + 1; 100 + 100 + 57 in a pitch of 128
DRAW_COUNTS = [(1, 0), (127, 0), (128, 0), (129, 0), (257, 128), (257, 100)]

# block cokriging: 1300 sites in r blocks
BLOCK_M = 1300
BLOCK_R = [1, 255, 256, 257, 511, 512, 513]


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# ---- data -----------------------------------------------------------------------------------------------------------------
def make_data(seed, params, metric, n0, n1, shift=0.0):
    """The recipe of the older GPU tests (half of process 1 co-located with process 0: h == 0 off the diagonal, so the
    cross block and the nugget terms of the gradient see it), values drawn from the model (+ shift: a mean the zero-mean
    model does not know).  With a process of fewer than 64 sites: min(n0, n1) // 2 co-located sites.  n1 = 0 or a
    univariate parameter set: one process."""
    rng = np.random.default_rng(seed)
    p = orc.Params.from_flat(params)
    tot = n0 + n1
    if metric == HAV:
        pts = np.column_stack([rng.uniform(25, 50, tot), rng.uniform(-120, -70, tot)])
    else:
        pts = np.column_stack([rng.uniform(0, 10, tot), rng.uniform(0, 10, tot)])
    c0 = pts[:n0].copy()
    if p.n_procs == 1:
        coords = [c0]
    else:
        k = min(n0 - n0 // 2, n1) if min(n0, n1) >= 64 else min(n0, n1) // 2
        coords = [c0, np.vstack([c0[n0 - k:], pts[n0:n0 + n1 - k]])]
    S = orc.joint_cov(p, coords, metric)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0]) + shift
    return coords, ([z[:n0]] if p.n_procs == 1 else [z[:n0], z[n0:]])


class DataSet:
    """one entry of DATA_CASES with its dense Sigma and factor, built once"""

    def __init__(self, case):
        n0, n1, seed, name, metric = case
        self.case, self.params, self.metric = case, PARAMS[name], metric
        self.p = orc.Params.from_flat(self.params)
        self.coords, self.values = make_data(seed, self.params, metric, n0, n1)
        self.z = np.concatenate(self.values)
        self.S = orc.joint_cov(self.p, self.coords, metric)
        self.cf = cho_factor(self.S, lower=True)
        self.N = len(self.z)


@functools.lru_cache(maxsize=None)
def data_set(case):
    return DataSet(case)


def pred_sites(rng, metric, m):
    if metric == HAV:
        return np.column_stack([rng.uniform(26, 49, m), rng.uniform(-118, -72, m)])
    return np.column_stack([rng.uniform(0.5, 9.5, m), rng.uniform(0.5, 9.5, m)])


def draw_sites(ds, i, m, n_on, seed):
    """m sites of process i, n_on of them on data of process i, shuffled: (sites, mask of those on data)"""
    rng = np.random.default_rng(seed)
    mine = ds.coords[i][rng.choice(len(ds.coords[i]), n_on, replace=False)]
    pc = np.vstack([pred_sites(rng, ds.metric, m - n_on), mine])
    perm = rng.permutation(m)
    on = np.zeros(m, dtype=bool)
    on[np.argsort(perm)[m - n_on:]] = True
    return pc[perm], on


def block_labels(rng, r, m):
    """labels of m sites in r non-empty blocks, scattered by a permutation.  From six blocks on: blocks of 1, 3, 4, 5 and
    8 sites (k_block_fold's unroll by four and its tail) and one block of more than half the sites, the rest random."""
    if r == m:
        return rng.permutation(m)
    if r < 6:
        sizes = np.full(r, m // r)
        sizes[0] += m - sizes.sum()
    else:
        sizes = np.ones(r, dtype=np.int64)
        sizes[:5] = [1, 3, 4, 5, 8]
        sizes[5] = m // 2 + 1
        rest = m - sizes.sum()
        assert rest >= 0
        if r > 6:
            np.add.at(sizes, 6 + rng.integers(0, r - 6, rest), 1)
        else:
            sizes[5] += rest
    lab = np.repeat(np.arange(r), sizes)
    assert len(lab) == m
    return lab[rng.permutation(m)]


def amat(lab, w, r):
    A = np.zeros((r, len(lab)))
    A[lab, np.arange(len(lab))] = w
    return A


# ---- log-likelihood ---------------------------------------------------------------------------------------------------------
def dense_ll(params, coords, values, metric, S=None):
    """(l, log|Sigma|, z^T Sigma^-1 z) of the dense chain"""
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric) if S is None else S
    z = np.concatenate(values)
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    quad = float(z @ cho_solve(cho_factor(S, lower=True), z))
    return -0.5 * (len(z) * np.log(2 * np.pi) + logdet + quad), logdet, quad


def fd_steps(x):
    """the step of every parameter: 1e-3 relative (at least 1e-3), nuggets -- they are small -- 1e-4"""
    nug = (3,) if len(x) == 4 else (8, 9)
    return np.array([1e-4 if k in nug else 1e-3 * max(abs(x[k]), 1.0) for k in range(len(x))])


def fd_of(f, x, scale=1.0):
    """4th-order central differences of f (a scalar or an array) in every parameter, steps scale * fd_steps"""
    x = np.asarray(x, dtype=float)
    out = []
    for k, e in enumerate(scale * fd_steps(x)):
        v = []
        for d in (-2, -1, 1, 2):
            y = x.copy()
            y[k] += d * e
            v.append(f(y))
        out.append((8 * (v[2] - v[1]) - (v[3] - v[0])) / (12 * e))
    return np.array(out)


def fd_grad(params, coords, values, metric, scale=1.0):
    """4th-order central differences of the dense log-likelihood in every parameter"""
    return fd_of(lambda y: dense_ll(y, coords, values, metric)[0], params, scale)


# dSigma / dtheta_k block by block.  Sigma's blocks are sigma_i^2 R_ii + nugget_i [h == 0] and rho sigma_1 sigma_2 R_12 with
# R the oracle's Matern correlation; joint_cov_cached is orc.joint_cov with the distances and the correlations (per nu and
# length scale) kept, so that a difference in sigma, nugget or rho costs no Bessel evaluation and one in nu or the length
# scale only its own block's.  test_dense_chains.py asserts that it equals orc.joint_cov bit for bit.
BLOCK_OF = {11: [((0, 0), (0, 1)), ((1, 1), (0, 1)), ((0, 0),), ((0, 1),), ((1, 1),), ((0, 0),), ((0, 1),), ((1, 1),),
                 ((0, 0),), ((1, 1),), ((0, 1),)],
            4: [((0, 0),)] * 4}   # the blocks parameter k enters


class CovCache:
    def __init__(self, coords, metric):
        n = len(coords)
        self.n = n
        self.D = {(i, j): orc.distance_matrix(coords[i], coords[j], metric) for i in range(n) for j in range(i, n)}
        self.R = {}

    def block(self, p, i, j):
        key = (i, j, float(p.nu[i, j]), float(p.len_scale[i, j]))
        if key not in self.R:
            D = self.D[i, j]
            self.R[key] = orc.matern_correlation(p.nu[i, j], p.len_scale[i, j], D).reshape(D.shape)
        R = self.R[key]
        if i == j:   # orc.covariance
            C = p.sigma[i] ** 2 * R
            C[self.D[i, j] == 0] += p.nugget[i]
            return C
        return p.rho * np.prod(p.sigma) * R   # orc.cross_covariance

    def joint_cov(self, p):
        B = {(i, j): self.block(p, i, j) for i in range(self.n) for j in range(i, self.n)}
        return np.block([[B[i, j] if i <= j else B[j, i].T.copy() for j in range(self.n)] for i in range(self.n)])


def grad_trace(params, coords, metric, G, scale=1.0, cache=None):
    """1/2 sum_pq G_pq (dSigma/dtheta_k)_pq for a symmetric G, dSigma by 4th-order central differences of the oracle's
    covariance blocks (steps scale * fd_steps).  Linear in the differenced quantity, so its error is the FD truncation of a
    smooth matrix entry and not the cancellation of differencing l itself; a different formula from the library's analytic
    Matern derivatives.  Blocks that do not depend on theta_k are skipped: their difference is identically zero."""
    x = np.asarray(params, dtype=float)
    cache = cache or CovCache(coords, metric)
    n0 = len(coords[0])
    sl = {0: slice(0, n0), 1: slice(n0, None)}
    g = np.zeros(x.size)
    for k, e in enumerate(scale * fd_steps(x)):
        for (i, j) in BLOCK_OF[x.size][k]:
            v = []
            for d in (-2, -1, 1, 2):
                y = x.copy()
                y[k] += d * e
                v.append(cache.block(orc.Params.from_flat(y), i, j))
            dC = (8 * (v[2] - v[1]) - (v[3] - v[0])) / (12 * e)
            g[k] += (0.5 if i == j else 1.0) * np.sum(G[sl[i], sl[j]] * dC)   # the (0, 1) block stands for (1, 0) too
    return g


def dense_ll_grad(params, coords, values, metric, scale=1.0, S=None):
    """the gradient of l as 1/2 tr(G dSigma), G = alpha alpha^T - Sigma^-1 formed densely"""
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric) if S is None else S
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    a = Si @ np.concatenate(values)
    return grad_trace(params, coords, metric, np.outer(a, a) - Si, scale)


# ---- trend designs, universal cokriging, REML -------------------------------------------------------------------------------
def design(kind, coords_k, pts):
    """the library's trend designs written out: "constant", "linear" (scaled by the process's data sites); "wide": eight
    user columns, the most ck_set_trend takes for one process"""
    if kind == "constant":
        return np.ones((len(pts), 1))
    mu, sd = coords_k.mean(0), coords_k.std(0)
    u = (pts - mu) / sd
    if kind == "linear":
        return np.column_stack([np.ones(len(pts)), u])
    assert kind == "wide"
    x, y = u[:, 0], u[:, 1]
    return np.column_stack([np.ones(len(pts)), x, y, x * y, x * x - 1, y * y - 1, np.sin(2 * x), np.cos(2 * y)])


def block_X(Fs):
    p = sum(F.shape[1] for F in Fs)
    X = np.zeros((sum(len(F) for F in Fs), p))
    r = c = 0
    for F in Fs:
        X[r:r + len(F), c:c + F.shape[1]] = F
        r += len(F)
        c += F.shape[1]
    return X


def x0_of(Fs, i, F0):
    p = sum(F.shape[1] for F in Fs)
    off = sum(F.shape[1] for F in Fs[:i])
    x0 = np.zeros((len(F0), p))
    x0[:, off:off + F0.shape[1]] = F0
    return x0


def dense_universal(p, coords, values, pc, i, metric, Fs, F0, S=None):
    """the bordered (Lagrange) system [[Sigma, X], [X^T, 0]] [lam; mu] = [c0; x0^T] solved densely, and dense GLS:
    (pred, variance, beta, cov(beta))"""
    S = orc.joint_cov(p, coords, metric) if S is None else S
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    X = block_X(Fs)
    x0 = x0_of(Fs, i, F0)
    N, q = X.shape
    K = np.block([[S, X], [X.T, np.zeros((q, q))]])
    sol = np.linalg.solve(K, np.vstack([c0, x0.T]))
    lam, mu = sol[:N], sol[N:]
    z = np.concatenate(values)
    pred = lam.T @ z
    c00 = np.diag(orc.pred_cov(p, pc[:1], i, metric))[0]
    var = c00 - np.sum(lam * c0, axis=0) - np.sum(mu * x0.T, axis=0)
    cf = cho_factor(S, lower=True)
    A = X.T @ cho_solve(cf, X)
    beta = np.linalg.solve(A, X.T @ cho_solve(cf, z))
    return pred, var, beta, np.linalg.inv(A)


def gls_universal(p, coords, values, pc, i, metric, Fs, F0):
    """the same predictor in its GLS form: beta, then simple kriging of the residual plus the trend term;
    variance = simple-kriging variance + r^T (X^T Sigma^-1 X)^-1 r, r = x0 - X^T Sigma^-1 c0"""
    S = orc.joint_cov(p, coords, metric)
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    X, x0 = block_X(Fs), x0_of(Fs, i, F0)
    z = np.concatenate(values)
    cf = cho_factor(S, lower=True)
    A = X.T @ cho_solve(cf, X)
    beta = np.linalg.solve(A, X.T @ cho_solve(cf, z))
    w = cho_solve(cf, c0)
    pred = w.T @ (z - X @ beta) + x0 @ beta
    r = x0.T - X.T @ w
    c00 = np.diag(orc.pred_cov(p, pc[:1], i, metric))[0]
    return pred, c00 - np.sum(w * c0, axis=0) + np.sum(r * np.linalg.solve(A, r), axis=0), beta


def dense_reml(params, coords, values, metric, Fs):
    """(l_R, log|Sigma|, log|X^T Sigma^-1 X|, z^T P z): the convention of include/cokrige.h (no log|X^T X| term)"""
    p = orc.Params.from_flat(params)
    S = orc.joint_cov(p, coords, metric)
    X = block_X(Fs)
    z = np.concatenate(values)
    cf = cho_factor(S, lower=True)
    A = X.T @ cho_solve(cf, X)
    b = X.T @ cho_solve(cf, z)
    _, ldS = np.linalg.slogdet(S)
    _, ldA = np.linalg.slogdet(A)
    quad = float(z @ cho_solve(cf, z) - b @ np.linalg.solve(A, b))
    N, q = X.shape
    return -0.5 * ((N - q) * np.log(2 * np.pi) + ldS + ldA + quad), ldS, ldA, quad


def dense_reml_grad(params, coords, values, metric, Fs, scale=1.0, S=None):
    """the gradient of l_R as 1/2 tr(G_R dSigma), G_R = (P z)(P z)^T - P with the projection
    P = Sigma^-1 - Sigma^-1 X (X^T Sigma^-1 X)^-1 X^T Sigma^-1 formed densely"""
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric) if S is None else S
    X = block_X(Fs)
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    SX = Si @ X
    P = Si - SX @ np.linalg.solve(X.T @ SX, SX.T)
    P = 0.5 * (P + P.T)
    a = P @ np.concatenate(values)
    return grad_trace(params, coords, metric, np.outer(a, a) - P, scale)


# ---- posterior, blocks, draws ---------------------------------------------------------------------------------------------
def posterior(p, coords, values, pc, i, metric, cf=None):
    """pred and S = C_pp - c0^T Sigma^-1 c0 (src/joint_prediction.py:60-78 with the full m x m matrix)"""
    cf = cho_factor(orc.joint_cov(p, coords, metric), lower=True) if cf is None else cf
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    pred = c0.T @ cho_solve(cf, np.concatenate(values))
    return pred, orc.pred_cov(p, pc, i, metric) - c0.T @ cho_solve(cf, c0)


def dense_blocks(p, coords, values, pc, i, metric, A, cf=None):
    """A pred, the posterior A S A^T and the prior A C_pp A^T"""
    pred, S = posterior(p, coords, values, pc, i, metric, cf)
    return A @ pred, A @ S @ A.T, A @ orc.pred_cov(p, pc, i, metric) @ A.T


def internal_order(hilbert_order, pc, site_order):
    """the order in which the library lays prediction sites out: hilbert_order (native.hilbert_order) from 256 sites on
    with option site_order = 1, else the caller's"""
    return hilbert_order(pc) if site_order and len(pc) >= 256 else np.arange(len(pc))


def chain_factor(S, defl, perm, jitter_abs=0.0):
    """the Cholesky of S without the deflated sites, in the library's order: (kept sites in that order, L)"""
    kept = perm[~defl[perm]]
    if len(kept) == 0:
        return kept, np.zeros((0, 0))
    return kept, np.linalg.cholesky(S[np.ix_(kept, kept)] + jitter_abs * np.eye(len(kept)))


def chain_draws(pred, S, defl, perm, eps, jitter_abs=0.0):
    kept, L = chain_factor(S, defl, perm, jitter_abs)
    x = np.zeros_like(eps)
    x[:, kept] = eps[:, kept] @ L.T
    return pred + x


# ---- Fisher information -------------------------------------------------------------------------------------------------------
# The 13 slots of ck_loglik_fisher by the kind of their derivative: exact block expressions (sigma, nugget, rho, noise
# scales), the length scales (closed form in the library, differenced here) and nu (differenced on both sides).
SLOTS = {11: {"exact": [0, 1, 8, 9, 10, 11, 12], "len": [5, 6, 7], "nu": [2, 3, 4]},
         4: {"exact": [0, 3, 11], "len": [2], "nu": [1]}}


def _corr(nu, ls, d):
    return orc.matern_correlation(nu, ls, d).reshape(d.shape)


def _d4(f, x, scale=1.0):
    """4th-order central difference of f at x with fd_grad's step (times scale)"""
    e = scale * (1e-3 * max(abs(x), 1.0))
    return (f(x - 2 * e) - 8 * f(x - e) + 8 * f(x + e) - f(x + 2 * e)) / (12 * e)


def derivative_matrices(params, coords, metric, noise=None, scale=1.0):
    """{slot: D_slot} (N x N each) over the 13 slots of ck_loglik_fisher; noise: per process the variances d_a or None"""
    p = orc.Params.from_flat(params)
    n = [len(c) for c in coords]
    N = sum(n)
    off = [0, n[0]]
    D = {}

    def put(i, j, blk):
        M = np.zeros((N, N))
        M[off[i]:off[i] + n[i], off[j]:off[j] + n[j]] = blk
        if i != j:
            M[off[j]:off[j] + n[j], off[i]:off[i] + n[i]] = blk.T
        return M

    d00 = orc.distance_matrix(coords[0], coords[0], metric)
    if p.n_procs == 1:
        s, nu, ls = p.sigma[0], p.nu[0, 0], p.len_scale[0, 0]
        D[0] = put(0, 0, 2 * s * _corr(nu, ls, d00))
        D[1] = put(0, 0, s * s * _d4(lambda x: _corr(x, ls, d00), nu, scale))
        D[2] = put(0, 0, s * s * _d4(lambda x: _corr(nu, x, d00), ls, scale))
        D[3] = put(0, 0, (d00 == 0).astype(float))
    else:
        d01 = orc.distance_matrix(coords[0], coords[1], metric)
        d11 = orc.distance_matrix(coords[1], coords[1], metric)
        s1, s2, rho = p.sigma[0], p.sigma[1], p.rho
        R00 = _corr(p.nu[0, 0], p.len_scale[0, 0], d00)
        R01 = _corr(p.nu[0, 1], p.len_scale[0, 1], d01)
        R11 = _corr(p.nu[1, 1], p.len_scale[1, 1], d11)
        D[0] = put(0, 0, 2 * s1 * R00) + put(0, 1, rho * s2 * R01)
        D[1] = put(1, 1, 2 * s2 * R11) + put(0, 1, rho * s1 * R01)
        D[2] = put(0, 0, s1 * s1 * _d4(lambda x: _corr(x, p.len_scale[0, 0], d00), p.nu[0, 0], scale))
        D[3] = put(0, 1, rho * s1 * s2 * _d4(lambda x: _corr(x, p.len_scale[0, 1], d01), p.nu[0, 1], scale))
        D[4] = put(1, 1, s2 * s2 * _d4(lambda x: _corr(x, p.len_scale[1, 1], d11), p.nu[1, 1], scale))
        D[5] = put(0, 0, s1 * s1 * _d4(lambda x: _corr(p.nu[0, 0], x, d00), p.len_scale[0, 0], scale))
        D[6] = put(0, 1, rho * s1 * s2 * _d4(lambda x: _corr(p.nu[0, 1], x, d01), p.len_scale[0, 1], scale))
        D[7] = put(1, 1, s2 * s2 * _d4(lambda x: _corr(p.nu[1, 1], x, d11), p.len_scale[1, 1], scale))
        D[8] = put(0, 0, (d00 == 0).astype(float))
        D[9] = put(1, 1, (d11 == 0).astype(float))
        D[10] = put(0, 1, s1 * s2 * R01)
    for k in range(p.n_procs):
        if noise is not None and noise[k] is not None:
            D[11 + k] = put(k, k, np.diag(np.asarray(noise[k], dtype=float)))
    return D


def dense_sigma(params, coords, metric, noise=None, scales=(1.0, 1.0)):
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric)
    if noise is not None:
        dv = np.concatenate([scales[k] * np.asarray(noise[k], dtype=float) if noise[k] is not None else np.zeros(len(coords[k]))
                             for k in range(len(coords))])
        S = S + np.diag(dv)
    return S


def fisher_of(S, D, X=None):
    """I_jk = 1/2 tr(S^-1 D_j S^-1 D_k) over the slots of D through cho_solve (X: P formed densely in place of S^-1)"""
    cf = cho_factor(S, lower=True)
    if X is None:
        B = {k: cho_solve(cf, Dk) for k, Dk in D.items()}
    else:
        H = cho_solve(cf, X)
        P = cho_solve(cf, np.eye(S.shape[0])) - H @ np.linalg.solve(X.T @ H, H.T)
        B = {k: P @ Dk for k, Dk in D.items()}
    ref = np.zeros((13, 13))
    for j in B:
        for k in B:
            if k >= j:
                ref[j, k] = ref[k, j] = 0.5 * np.sum(B[j] * B[k].T)
    return ref


def dense_fisher(params, coords, metric, noise=None, scales=(1.0, 1.0), X=None, scale=1.0):
    """the 13 x 13 information of the dense chain (rows / columns of slots that do not exist are 0); scale multiplies the
    step of the differenced nu and length-scale derivatives, as fd_of's does"""
    return fisher_of(dense_sigma(params, coords, metric, noise, scales), derivative_matrices(params, coords, metric, noise, scale), X)


def normalised(I, ref):
    """|I - ref| / sqrt(ref_jj ref_kk) over the entries whose scale is positive; the others must be equal"""
    d = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    pos = d > 0
    assert np.array_equal(I[~pos], ref[~pos]), (I[~pos], ref[~pos])
    e = np.zeros_like(I)
    e[pos] = np.abs(I - ref)[pos] / d[pos]
    return e


def class_errors(e, npar):
    """the largest entry of a normalised() error per class of pairs: exact x exact; a length-scale slot with an exact or a
    length-scale slot; every pair with a nu slot"""
    s = SLOTS[npar]
    el = s["exact"] + s["len"]
    ln = np.zeros_like(e)
    ln[np.ix_(s["len"], el)] = e[np.ix_(s["len"], el)]
    ln[np.ix_(el, s["len"])] = e[np.ix_(el, s["len"])]
    nu = max(e[s["nu"], :].max(), e[:, s["nu"]].max())
    return {"exact": e[np.ix_(s["exact"], s["exact"])].max(), "len": ln.max(), "nu": nu}


# The reference's own floor in the length-scale class -- what halving _d4's step changes, in normalised()'s measure
# (tests/test_dense_chains.py: test_fisher_reference_floor measures and prints it for every rung of FISHER_CASES).  The bound
# of the length-scale class is max(1e-9, 10 x the rung's floor); a rung is listed here only when its floor exceeds 1e-10.
FISHER_LEN_FLOOR = {}
FISHER_TOL = {"exact": 1e-9, "nu": 1e-6}


def fisher_tol(case):
    return dict(FISHER_TOL, len=max(1e-9, 10.0 * FISHER_LEN_FLOOR.get(case, 0.0)))


def noise_of(ds, which=(0, 1), seed=5):
    """measurement-error variances uniform(0.01, 0.1) per process in `which`, None for the others"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.01, 0.1, len(ds.coords[k])) if k in which else None for k in range(ds.p.n_procs)]


def trend_kinds(ds, kind):
    """`kind` per process; a process with fewer data than the design has columns (ck_set_trend refuses it) gets "constant" """
    return [kind if len(c) >= TREND_COLUMNS[kind] else "constant" for c in ds.coords]


TREND_COLUMNS = {"constant": 1, "linear": 3, "wide": 8}


def annihilated_slots(n, kinds):
    """REML with as many trend columns on a process as it has sites (one site with the constant design, three with the
    linear one): the unit vectors of its sites lie in the span of X, so P e_a = 0 there and every D_k supported on its rows
    and columns alone has P D_k P = 0 -- sigma, nu, len, nugget and noise scale of that process and everything of the cross
    block.  Their information is 0 in exact arithmetic and rounding noise (1e-16 of the slot's scale) in any computation, the
    dense chain included, so normalised() has no scale for them: they are compared with 0 in the scale of the ML
    information (ml_scaled) and taken out of both matrices (drop_slots)"""
    if len(n) != 2 or kinds is None:
        return []
    out = []
    for k, own in ((0, [0, 2, 5, 8, 11]), (1, [1, 4, 7, 9, 12])):
        if kinds[k] is not None and n[k] == TREND_COLUMNS[kinds[k]]:
            out += own + [3, 6, 10]
    return sorted(set(out))


def ml_scaled(I, ml, slots):
    """the largest |I_jk| over the rows `slots` in the scale sqrt(ml_jj ml_kk) of the ML information (1 where that is 0)"""
    d = np.where(np.diag(ml) > 0, np.diag(ml), 1.0)
    return float(np.max(np.abs(I[slots, :]) / np.sqrt(np.outer(d[slots], d)))) if len(slots) else 0.0


def drop_slots(I, slots):
    J = I.copy()
    J[slots, :] = 0.0
    J[:, slots] = 0.0
    return J


# ---- leave-group-out cross-validation -------------------------------------------------------------------------------------------
def dense_folds(S, z, members):
    """include/cokrige.h ck_cv_folds in dense form for a Sigma that already includes the noise: Q = S^-1 through cho_solve,
    alpha = Q z; per fold (index arrays in the caller's stacked order) pred_S = z_S - Q_SS^-1 alpha_S, var_S = diag(Q_SS^-1),
    log|Q_SS| and alpha_S^T Q_SS^-1 alpha_S: a list of (pred, var, logdet, quad)"""
    cf = cho_factor(S, lower=True)
    Q = cho_solve(cf, np.eye(len(z)))
    Q = 0.5 * (Q + Q.T)
    alpha = cho_solve(cf, z)
    out = []
    for ix in members:
        ix = np.asarray(ix, dtype=np.int64)
        cq = cho_factor(Q[np.ix_(ix, ix)], lower=True)
        C = cho_solve(cq, np.eye(len(ix)))
        w = cho_solve(cq, alpha[ix])
        out.append((z[ix] - w, np.diag(C).copy(), 2.0 * np.sum(np.log(np.diag(cq[0]))), float(alpha[ix] @ w)))
    return out


def oracle_folds(p, coords, values, metric, i, fi, fo):
    """the slow truth: per fold, the data without the fold -> joint_predict at the fold's sites of process i"""
    pred, err = np.full(len(fi), np.nan), np.full(len(fi), np.nan)
    for f in range(int(fi.max()) + 1):
        sel = np.flatnonzero(fi == f)
        keep_i = fi != f
        keep_o = np.ones(len(coords[1 - i]), dtype=bool) if fo is None else fo != f
        c, v = [None, None], [None, None]
        c[i], v[i] = coords[i][keep_i], values[i][keep_i]
        c[1 - i], v[1 - i] = coords[1 - i][keep_o], values[1 - i][keep_o]
        pred[sel], err[sel] = orc.joint_predict(p, c, v, coords[i][sel], i, metric)
    return pred, err


def labels_from_sizes(rng, n, i, sizes, other=True):
    """(fi, fo, sizes): fold f holds sizes[f] data scattered by a permutation, its first a datum of process i, the others
    from both processes (other: else process i alone; fo is then None); the data left over are labelled -1"""
    n_o = n[1 - i] if len(n) == 2 and other else 0
    own = rng.permutation(n[i])
    assert len(sizes) <= n[i] and sum(sizes) <= n[i] + n_o
    lab = [np.full(n[i], -1, dtype=np.int32), np.full(n_o, -1, dtype=np.int32)]
    for f in range(len(sizes)):
        lab[0][own[f]] = f
    pool = np.concatenate([own[len(sizes):], n[i] + np.arange(n_o)])
    pool = pool[rng.permutation(len(pool))]
    at = 0
    for f, s in enumerate(sizes):
        rest = pool[at:at + s - 1]
        lab[0][rest[rest < n[i]]] = f
        lab[1][rest[rest >= n[i]] - n[i]] = f
        at += s - 1
    return lab[0], (lab[1] if n_o else None), list(sizes)


def fold_sizes(n_i, total):
    """two singleton folds, a fold of 2, one of min(64, what is left) and the rest as one fold, as far as the `total` data
    (n_i of them of the predicted process, one per fold at least) go; a process of one datum is one fold"""
    if n_i == 1:
        return [min(64, max(1, total - 1))]
    sizes, left = [], total
    for w in (1, 1, 2, 64, total):
        w = min(w, left)
        if w > 0 and len(sizes) < n_i:
            sizes.append(w)
            left -= w
    return sizes


def fold_labels(case, i, other, minus, seed=0):
    """the labels of a FOLD_CASES entry: (fi, fo, sizes).  other: the folds take data of the other process too; minus: about
    a tenth of the data (one at least) is never withheld"""
    n = [k for k in case[:2] if k > 0]
    rng = np.random.default_rng(1000 * seed + 100 * i + 10 * other + minus + case[0])
    total = n[i] + (n[1 - i] if len(n) == 2 and other else 0)
    if minus and total >= 3:
        total -= max(1, total // 10)
    return labels_from_sizes(rng, n, i, fold_sizes(n[i], total), other)


def fold_members(n, i, fi, fo):
    """the folds' index arrays in the caller's stacked order (process 0 first), and per fold the positions inside it of
    the data of process i with their indices in process i"""
    off = [0, n[0]]
    mem, mine = [], []
    for f in range(int(fi.max()) + 1):
        a = np.flatnonzero(fi == f)
        b = np.flatnonzero(fo == f) if fo is not None else np.zeros(0, dtype=np.int64)
        ix = np.concatenate([off[i] + a, off[1 - i] + b]) if len(n) == 2 else a
        mem.append(ix)
        mine.append((np.arange(len(a)), a))
    return mem, mine


def folds_references(S, z, n, calls):
    """per call (i, fi, fo): (pred, var) over the data of process i (NaN where fi == -1) and the n_folds x 3 statistics,
    from ONE dense_folds over the folds of all calls (Sigma^-1 is formed once)"""
    plans = [fold_members(n, i, fi, fo) for i, fi, fo in calls]
    res = iter(dense_folds(S, z, [ix for mem, _ in plans for ix in mem]))
    out = []
    for (i, fi, fo), (mem, mine) in zip(calls, plans):
        pred, var = np.full(len(fi), np.nan), np.full(len(fi), np.nan)
        stats = np.zeros((len(mem), 3))
        for f in range(len(mem)):
            pr, vr, ld, qf = next(res)
            at, a = mine[f]
            pred[a], var[a] = pr[at], vr[at]
            stats[f] = len(mem[f]), ld, qf
        out.append((pred, var, stats))
    return out


def folds_reference(S, z, n, i, fi, fo):
    return folds_references(S, z, n, [(i, fi, fo)])[0]
