"""The Vecchia likelihood with a GLS trend (include/cokrige.h: ck_loglik_vecchia_trend) as a numpy loop over the sets of
tests/vecchia_ref.py: per datum v = L^-1 c, y = L^-1 z_c, U = L^-1 X_c, the row r_t = (z_t - v . y, x_t - U^T v) / s_t, then
G = sum_t r_t r_t^T = [[yy, b^T], [b, A]], beta = A^-1 b, Q = yy - b^T beta and the two totals.  Also the dense GLS quantities the
full-conditioning form must equal, and the bounds that per-datum tolerances on (mu_t, s_t^2, g_t) propagate to every sum (the
method of vecchia_ref.totals_bound).  Shared by tests/test_vecchia_trend_host.py and tests/test_gpu_vecchia_trend.py."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc
from tests import vecchia_ref as vr

LOG2PI = np.log(2.0 * np.pi)


def design(trend, coords):
    """(X (N, p) block diagonal, [F_0, F_1]): the regressors of trend.TrendDesign at the data sites"""
    from sif_xco2_cokriging_amd.trend import TrendDesign
    cs = [np.asarray(c, dtype=float)[:, :2] for c in coords]
    d = TrendDesign(trend, cs)
    F = [d.data(k, cs[k]) for k in range(len(cs))]
    return block_design(F), F


def block_design(F):
    n, p = [len(f) for f in F], [f.shape[1] for f in F]
    X = np.zeros((sum(n), sum(p)))
    r = c = 0
    for f in F:
        X[r:r + len(f), c:c + f.shape[1]] = f
        r, c = r + len(f), c + f.shape[1]
    return X


def joint_cov(params, coords, metric, noise=None):
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric)
    if noise is not None:
        S = S + np.diag(np.concatenate([np.zeros(len(c)) if d is None else np.asarray(d, dtype=float)
                                        for c, d in zip(coords, noise)]))
    return S


def totals(N, p, s1, G):
    """dict(A, b, yy, beta, cov, logdetA, Q, out5 (profile), out5_reml) from sum log s^2 and the Gram matrix"""
    yy, b, A = G[0, 0], G[1:, 0].copy(), G[1:, 1:].copy()
    cov = np.linalg.inv(A) if p else np.zeros((0, 0))
    beta = np.linalg.solve(A, b) if p else np.zeros(0)
    logdet = np.linalg.slogdet(A)[1] if p else 0.0
    Q = yy - b @ beta
    lp = -0.5 * (N * LOG2PI + s1 + Q)
    lr = -0.5 * ((N - p) * LOG2PI + s1 + logdet + Q)
    return dict(A=A, b=b, yy=yy, beta=beta, cov=cov, logdetA=logdet, Q=Q, out5=np.array([lp, s1, logdet, Q, yy]),
                out5_reml=np.array([lr, s1, logdet, Q, yy]))


def vecchia_trend_reference(params, coords, values, X, metric, ranks, max_dist, caps=(0, 0), noise=None, sets=None):
    """vecchia_reference's dict (mean = mu_t, var = s_t^2, count, keep, gap, ..) plus g (N, p) = U^T v, f = x - g, rows (N, 1 + p),
    G, totals()'s entries and mean_trend = mu_t + f_t . beta"""
    base = vr.vecchia_reference(params, coords, values, metric, ranks, max_dist, caps, noise=noise, sets=sets)
    assert base["info"] == 0
    S = joint_cov(params, coords, metric, noise)
    z, N, p = base["z"], len(base["z"]), X.shape[1]
    g = np.zeros((N, p))
    for t in range(N):
        c = np.flatnonzero(base["keep"][t])
        if c.size:
            L = np.linalg.cholesky(S[np.ix_(c, c)])
            v = solve_triangular(L, S[c, t], lower=True)
            g[t] = solve_triangular(L, X[c], lower=True).T @ v
    f = X - g
    s = np.sqrt(base["var"])
    rows = np.column_stack([(z - base["mean"]) / s, f / s[:, None]])
    G = rows.T @ rows
    out = dict(base, g=g, f=f, rows=rows, G=G, X=X, p=p)
    out.update(totals(N, p, base["logv"].sum(), G))
    out["mean_trend"] = base["mean"] + f @ out["beta"]
    return out


def dense_gls(params, coords, values, X, metric, noise=None):
    """the dense quantities: dict(logdet, A, b, beta, cov, logdetA, Q, out5, out5_reml) of z ~ N(X beta, Sigma)"""
    S = joint_cov(params, coords, metric, noise)
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    L = np.linalg.cholesky(S)
    y, U = solve_triangular(L, z, lower=True), solve_triangular(L, X, lower=True)
    G = np.column_stack([y, U]).T @ np.column_stack([y, U])
    return dict(totals(len(z), X.shape[1], 2.0 * np.log(np.diag(L)).sum(), G), logdet=2.0 * np.log(np.diag(L)).sum())


def bounds(ref, rtol, atol):
    """What per-datum errors of tol(x) = atol + rtol |x| in mu_t, s_t^2 and every g_tj can move the sums by, to first order plus
    the product of the row errors: dict(s1, G (1 + p, 1 + p), b, A, yy, beta, Q, logdetA, l, l_reml).
      r_0 = e / s:   dr_0 = tol(mu) / s + |e| tol(s^2) / (2 s^3);     r_j = f_j / s:   dr_j = tol(g_j) / s + |f_j| tol(s^2) / (2 s^3)
      dG_ab = sum_t |r_a| dr_b + |r_b| dr_a + dr_a dr_b
      dbeta <= |A^-1| (|db| + |dA| |beta|),  dCov(beta) <= 1.01 |A^-1|^2 |dA|   (2-norms, Frobenius for dA and for the result)
      dQ <= dyy + 2 |beta| . db + |beta|^T dA |beta|;   dlog|A| <= sum |A^-1| dA;   dl <= 1/2 (ds1 + dQ [+ dlog|A|])"""
    mu, s2, e = ref["mean"], ref["var"], ref["z"] - ref["mean"]
    s = np.sqrt(s2)
    tm, ts, tg = atol + rtol * np.abs(mu), atol + rtol * np.abs(s2), atol + rtol * np.abs(ref["g"])
    empty = ref["count"].sum(axis=1) == 0
    tm, tg = np.where(empty, 0.0, tm), np.where(empty[:, None], 0.0, tg)   # an empty set has mu = 0 and g = 0 exactly
    R = np.abs(ref["rows"])
    dR = np.column_stack([tm / s + np.abs(e) * ts / (2 * s ** 3), tg / s[:, None] + np.abs(ref["f"]) * (ts / (2 * s ** 3))[:, None]])
    dG = R.T @ dR + dR.T @ R + dR.T @ dR
    ab = np.abs(ref["beta"])
    db, dA = dG[1:, 0], dG[1:, 1:]
    d = dict(s1=np.sum(ts / s2), G=dG, b=db, A=dA, yy=dG[0, 0])
    d["beta"] = np.linalg.norm(ref["cov"], 2) * (np.linalg.norm(db) + np.linalg.norm(dA) * np.linalg.norm(ref["beta"])) if ref["p"] else 0.0
    d["cov"] = 1.01 * np.linalg.norm(ref["cov"], 2) ** 2 * np.linalg.norm(dA) if ref["p"] else 0.0   # d(A^-1) = -A^-1 dA A^-1
    d["Q"] = d["yy"] + 2 * ab @ db + ab @ dA @ ab
    d["logdetA"] = np.sum(np.abs(ref["cov"]) * dA)
    d["l"] = 0.5 * (d["s1"] + d["Q"])
    d["l_reml"] = d["l"] + 0.5 * d["logdetA"]
    return d


def profile_value(params, coords, values, X, metric, keep, noise=None):
    """l_P on fixed sets `keep` (for central differences in the parameters)"""
    S = joint_cov(params, coords, metric, noise)
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    N = len(z)
    rows, s1 = np.zeros((N, 1 + X.shape[1])), 0.0
    for t in range(N):
        c = np.flatnonzero(keep[t])
        m, s2, f = 0.0, S[t, t], X[t]
        if c.size:
            L = np.linalg.cholesky(S[np.ix_(c, c)])
            v = solve_triangular(L, S[c, t], lower=True)
            m, s2 = v @ solve_triangular(L, z[c], lower=True), S[t, t] - v @ v
            f = X[t] - solve_triangular(L, X[c], lower=True).T @ v
        rows[t] = np.r_[z[t] - m, f] / np.sqrt(s2)
        s1 += np.log(s2)
    return totals(N, X.shape[1], s1, rows.T @ rows)["out5"][0]
