"""Dense float64 reference chains for the likelihood, REML, universal, block and conditional-draw entry points, and the
list of data sets tests/test_gpu_entry_edge_sizes.py runs them on.  Plain numpy / scipy on the oracle's covariances
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
# every data set the GPU module uses: the host test checks that Sigma factors and cond(Sigma) < 1e8 for each of them
DATA_CASES = list(dict.fromkeys(LIK_CASES + FIVE_RUNGS + [(64, 64, 40, "BIV", HAV), SMALL, LARGE, REFIT]))

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
