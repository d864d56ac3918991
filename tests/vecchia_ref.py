"""The Vecchia likelihood of include/cokrige.h (ck_loglik_vecchia) as a numpy loop over the data, on oracle.joint_cov /
oracle.distance_matrix in float64: per datum and process the candidates of smaller rank within max_dist, np.partition for the
cut (ties kept), a dense Cholesky of the selected rows.  Shared by tests/test_vecchia_host.py and tests/test_gpu_vecchia.py."""
import numpy as np

from oracle import cokrige_oracle as orc


def stacked_distances(coords, metric):
    """(N, N) distances of the stacked sites (process 0 then 1) and the process of every datum"""
    allc = np.vstack(coords)
    proc = np.concatenate([np.full(len(c), q) for q, c in enumerate(coords)])
    return orc.distance_matrix(allc, allc, metric), proc


def conditioning_sets(D, proc, ranks, max_dist, caps):
    """keep (N, N) bool: keep[t, s] = datum s is in the set of datum t; gap (N,): the smallest relative distance between the
    last kept and the first dropped candidate over the processes of t (inf where no cap binds); capped (N,) bool"""
    N = D.shape[0]
    ranks = np.asarray(ranks)
    keep = np.zeros((N, N), dtype=bool)
    gap = np.full(N, np.inf)
    capped = np.zeros(N, dtype=bool)
    for t in range(N):
        for q in range(int(proc.max()) + 1):
            cand = np.flatnonzero((proc == q) & (ranks < ranks[t]) & (D[t] <= max_dist))
            cap = caps[q]
            if cap > 0 and cand.size > cap:
                d = D[t, cand]
                r = np.partition(d, cap - 1)[cap - 1]
                dropped = d[d > r]
                if dropped.size:
                    gap[t] = min(gap[t], (dropped.min() - r) / r if r > 0 else np.inf)
                cand = cand[d <= r]
                capped[t] = True
            keep[t, cand] = True
    return keep, gap, capped


def vecchia_reference(params, coords, values, metric, ranks, max_dist, caps=(0, 0), noise=None, sets=None):
    """dict(mean, var, count (N, 2), out3, info, n_empty, k_max, n_capped, gap).  noise: per process s_k * d_a (array) or None:
    added to the diagonal of every local system and to the datum's own variance.  A datum whose local system is not positive
    definite or whose variance is not > 0 has NaN terms and makes out3 NaN, info = 1 + the first such datum."""
    p = orc.Params.from_flat(params)
    S = orc.joint_cov(p, coords, metric)
    if noise is not None:
        S = S + np.diag(np.concatenate([np.zeros(len(c)) if d is None else np.asarray(d, dtype=float)
                                        for c, d in zip(coords, noise)]))
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    D, proc = stacked_distances(coords, metric)
    keep, gap, capped = conditioning_sets(D, proc, ranks, max_dist, caps) if sets is None else sets
    N = len(z)
    mean, var = np.zeros(N), np.zeros(N)
    count = np.zeros((N, 2), dtype=np.int64)
    bad = []
    for t in range(N):
        c = np.flatnonzero(keep[t])
        count[t, 0], count[t, 1] = np.count_nonzero(proc[c] == 0), np.count_nonzero(proc[c] == 1)
        if c.size == 0:
            mean[t], var[t] = 0.0, S[t, t]
        else:
            try:
                L = np.linalg.cholesky(S[np.ix_(c, c)])
            except np.linalg.LinAlgError:
                mean[t] = var[t] = np.nan
                bad.append(t)
                continue
            from scipy.linalg import solve_triangular
            v = solve_triangular(L, S[c, t], lower=True)
            y = solve_triangular(L, z[c], lower=True)
            mean[t], var[t] = v @ y, S[t, t] - v @ v
        if not var[t] > 0:
            bad.append(t)
    with np.errstate(invalid="ignore", divide="ignore"):
        logv = np.where(var > 0, np.log(np.where(var > 0, var, 1.0)), np.nan)
        quad = np.where(var > 0, (z - mean) ** 2 / np.where(var > 0, var, 1.0), np.nan)
    s1, s2 = logv.sum(), quad.sum()
    out3 = np.array([-0.5 * (N * np.log(2 * np.pi) + s1 + s2), s1, s2])
    ktot = count.sum(axis=1)
    return dict(mean=mean, var=var, count=count, out3=out3, info=(min(bad) + 1) if bad else 0, z=z, logv=logv, quad=quad,
                n_empty=int(np.count_nonzero(ktot == 0)), k_max=int(ktot.max()), n_capped=int(np.count_nonzero(capped)),
                gap=gap, keep=keep)


def dense_logpdf(params, coords, values, metric, noise=None):
    """(l, log|Sigma|, z^T Sigma^-1 z) of the zero-mean Gaussian with the joint covariance"""
    p = orc.Params.from_flat(params)
    S = orc.joint_cov(p, coords, metric)
    if noise is not None:
        S = S + np.diag(np.concatenate([np.zeros(len(c)) if d is None else np.asarray(d, dtype=float)
                                        for c, d in zip(coords, noise)]))
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    L = np.linalg.cholesky(S)
    from scipy.linalg import solve_triangular
    y = solve_triangular(L, z, lower=True)
    logdet, quad = 2.0 * np.log(np.diag(L)).sum(), y @ y
    return np.array([-0.5 * (len(z) * np.log(2 * np.pi) + logdet + quad), logdet, quad])


def totals_bound(ref, rtol, atol):
    """What per-datum errors of tol(x) = atol + rtol |x| in the mean and in the variance can move the sums by:
    (bound on out3[1], on out3[2], on l):  d log s^2 = ds^2 / s^2;  d (e^2 / s^2) = 2 |e| / s^2 dmu + e^2 / s^4 ds^2;
    for l the issue's sum_t |e_t| / s_t^2 tol(mu_t) + 1/2 |1 / s_t^2 - e_t^2 / s_t^4| tol(s_t^2)."""
    mu, s2, e = ref["mean"], ref["var"], ref["z"] - ref["mean"]
    tm, ts = atol + rtol * np.abs(mu), atol + rtol * np.abs(s2)
    b1 = np.sum(ts / s2)
    b2 = np.sum(2 * np.abs(e) / s2 * tm + e * e / s2 ** 2 * ts)
    bl = np.sum(np.abs(e) / s2 * tm + 0.5 * np.abs(1 / s2 - e * e / s2 ** 2) * ts)
    return b1, b2, bl


def half_colocated_sites(n, seed=20002):
    """unit_square-style sites: n per process uniform on the unit square, half of process 1 co-located with process 0"""
    from sif_xco2_cokriging_amd import synth
    pb = synth.unit_square_problem(n, grid_side=2, seed=seed)
    return pb["coords"], pb["values"]
