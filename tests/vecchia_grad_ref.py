"""The gradient of the Vecchia likelihood (include/cokrige.h: ck_loglik_vecchia_grad) in numpy, on the sets of
tests/vecchia_ref.py: vecchia_reference.  Per datum t with set c: w = S_cc^-1 S_ct, alpha = S_cc^-1 z_c, b = (-w, 1), a = (alpha, 0),
    M_t = (e^2 / s^4 - 1 / s^2) b b^T + (e / s^2) (b a^T + a b^T),   score_t[k] = 1/2 sum_pq M_t[p, q] dSigma_k[p, q],
dSigma_k by the fourth-order block differences of dense_chains.CovCache (formed once, contracted per datum), the noise slots
1/2 sum_p M_t[p, p] d_p per process.  G_V is the sum of the M_t scattered into N x N.  A different formula from the library's
analytic Matern derivatives.  Shared by tests/test_vecchia_grad_host.py and tests/test_gpu_vecchia_grad.py."""
import numpy as np

from oracle import cokrige_oracle as orc
from tests import dense_chains as dc


def measure(g, ref):
    """the project's gradient measure (tests/test_gpu_likelihood.py: test_gradient_against_dense_differences)"""
    g, ref = np.asarray(g, dtype=float), np.asarray(ref, dtype=float)
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)


def derivative_matrices(params, coords, metric, scale=1.0, cache=None):
    """[dSigma / dtheta_k] (N x N each) over the flat parameters, blocks differenced as dense_chains.grad_trace does"""
    x = np.asarray(params, dtype=float)
    cache = cache or dc.CovCache(coords, metric)
    n = [len(c) for c in coords]
    off = [0, n[0]]
    out = []
    for k, e in enumerate(scale * dc.fd_steps(x)):
        D = np.zeros((sum(n), sum(n)))
        for (i, j) in dc.BLOCK_OF[x.size][k]:
            v = []
            for d in (-2, -1, 1, 2):
                y = x.copy()
                y[k] += d * e
                v.append(cache.block(orc.Params.from_flat(y), i, j))
            dC = (8 * (v[2] - v[1]) - (v[3] - v[0])) / (12 * e)
            D[off[i]:off[i] + n[i], off[j]:off[j] + n[j]] = dC
            if i != j:
                D[off[j]:off[j] + n[j], off[i]:off[i] + n[i]] = dC.T
        out.append(D)
    return out


def vecchia_grad_reference(params, coords, values, metric, ref, noise_d=None, scales=(1.0, 1.0), dS=None):
    """dict(score (N, 13), grad13, G_V) on the sets ref["keep"] of vecchia_reference (called with noise = scales[k] * noise_d[k]).
    A datum without a term (ref's var not > 0 or NaN) has a NaN score and makes grad13 NaN."""
    p = orc.Params.from_flat(params)
    S = orc.joint_cov(p, coords, metric)
    n = [len(c) for c in coords]
    N = sum(n)
    proc = np.concatenate([np.full(m, q) for q, m in enumerate(n)])
    dvec = np.zeros(N)
    if noise_d is not None:
        for q in range(len(coords)):
            if noise_d[q] is not None:
                dvec[proc == q] = np.asarray(noise_d[q], dtype=float)
        S = S + np.diag(dvec * np.asarray(scales, dtype=float)[proc])
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    dS = derivative_matrices(params, coords, metric) if dS is None else dS
    score = np.zeros((N, 13))
    G = np.zeros((N, N))
    for t in range(N):
        c = np.flatnonzero(ref["keep"][t])
        s2, e = ref["var"][t], z[t] - ref["mean"][t]
        if not s2 > 0:
            score[t] = np.nan
            continue
        ix = np.r_[c, t]
        b, a = np.zeros(ix.size), np.zeros(ix.size)
        b[-1] = 1.0
        if c.size:
            Scc = S[np.ix_(c, c)]
            b[:-1] = -np.linalg.solve(Scc, S[c, t])
            a[:-1] = np.linalg.solve(Scc, z[c])
        M = (e * e / s2 ** 2 - 1.0 / s2) * np.outer(b, b) + (e / s2) * (np.outer(b, a) + np.outer(a, b))
        G[np.ix_(ix, ix)] += M
        for k, D in enumerate(dS):
            score[t, k] = 0.5 * np.sum(M * D[np.ix_(ix, ix)])
        for q in range(len(coords)):
            sel = proc[ix] == q
            score[t, 11 + q] = 0.5 * np.sum(np.diag(M)[sel] * dvec[ix][sel])
    return dict(score=score, grad13=score.sum(axis=0), G_V=G)
