"""Both processes in the moving neighbourhood (include/cokrige.h: ck_predict_local_pair, ck_simulate_local_pair) as numpy loops
on the oracle's functions, dense solves in float64.  Shared by tests/test_local_pair_host.py and tests/test_gpu_local_pair.py.

local_pair_reference: per point the neighbour set by the header's rule (the radius, per process the cap with ties kept), Sigma_loc
from oracle.joint_cov, c^0 and c^1 from oracle.pred_cross_cov, the five outputs by dense solves.
local_cosim_reference / dense_chain_pair: tests/local_sim_ref.py's local_sim_reference and dense_chain on the STACKED sites of both
processes (stacked index k for site k of process 0, m0 + k for site k of process 1)."""
import numpy as np

from oracle import cokrige_oracle as orc
from tests import vecchia_ref as vr
from tests.local_sim_ref import levels_of


def _noise_diag(coords, noise):
    return np.concatenate([np.zeros(len(c)) if noise is None or noise[k] is None else np.asarray(noise[k], dtype=float)
                           for k, c in enumerate(coords)])


def neighbour_sets(D, proc, max_dist, caps):
    """keep (m, N) bool from the distances D (m points x N stacked data); gap: the smallest relative gap at a cut -- a cap's cut
    distance against the first dropped candidate, and the radius against the candidate nearest to it on either side"""
    m, N = D.shape
    keep = np.zeros((m, N), dtype=bool)
    gap = np.inf
    for t in range(m):
        if max_dist > 0 and N:
            gap = min(gap, np.min(np.abs(D[t] - max_dist)) / max_dist)
        for q in range(int(proc.max()) + 1):
            cand = np.flatnonzero((proc == q) & (D[t] <= max_dist))
            cap = caps[q]
            if cap > 0 and cand.size > cap:
                d = D[t, cand]
                r = np.partition(d, cap - 1)[cap - 1]
                dropped = d[d > r]
                if dropped.size:
                    gap = min(gap, (dropped.min() - r) / r if r > 0 else np.inf)
                cand = cand[d <= r]
            keep[t, cand] = True
    return keep, float(gap)


def local_pair_reference(params, coords, values, metric, sites, max_dist, caps=(0, 0), noise=None):
    """dict(pred0, err0, pred1, err1, cov (m each), k (m), count (m, 2), n_empty, n_not_pd, k_max, gap, post (m, 2, 2): the raw
    posterior matrices [[c00 - v0.v0, c01 - v0.v1], [., c11 - v1.v1]]).  noise: per process s_k * d_a (array) or None."""
    p = orc.Params.from_flat(params)
    coords = [np.asarray(c, dtype=float) for c in coords]
    sites = np.atleast_2d(np.asarray(sites, dtype=float))
    n0, m = len(coords[0]), len(sites)
    S = orc.joint_cov(p, coords, metric) + np.diag(_noise_diag(coords, noise))
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    C = [orc.pred_cross_cov(p, coords, sites, q, metric) for q in range(2)]   # N x m each
    allc = np.vstack(coords)
    proc = np.concatenate([np.full(len(c), q) for q, c in enumerate(coords)])
    D = orc.distance_matrix(sites, allc, metric)
    keep, gap = neighbour_sets(D, proc, max_dist, caps)
    prior = np.array([[p.sigma[0] ** 2 + p.nugget[0], 0.0], [0.0, p.sigma[1] ** 2 + p.nugget[1]]])
    prior[0, 1] = prior[1, 0] = float(orc.cross_covariance(p, 0, 1, np.zeros(1))[0])
    out = {k: np.full(m, np.nan) for k in ("pred0", "err0", "pred1", "err1", "cov")}
    post = np.full((m, 2, 2), np.nan)
    kk = keep.sum(axis=1)
    count = np.column_stack([keep[:, :n0].sum(axis=1), keep[:, n0:].sum(axis=1)])
    n_not_pd = 0
    for t in range(m):
        c = np.flatnonzero(keep[t])
        if c.size == 0:
            continue
        A = S[np.ix_(c, c)]
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            n_not_pd += 1
            continue
        cq = np.column_stack([C[0][c, t], C[1][c, t]])   # k x 2
        W = np.linalg.solve(A, cq)
        pr = W.T @ z[c]
        post[t] = prior - cq.T @ W
        out["pred0"][t], out["pred1"][t] = pr
        with np.errstate(invalid="ignore"):
            e = np.sqrt(np.diag(post[t]))
        out["err0"][t], out["err1"][t] = np.where(np.isnan(e), 0.0, e)
        out["cov"][t] = post[t, 0, 1]
    return dict(out, k=kk, count=count, n_empty=int(np.count_nonzero(kk == 0)), n_not_pd=n_not_pd, k_max=int(kk.max()), gap=gap,
                post=post)


# ---- the co-simulation ---------------------------------------------------------------------------------------------------
def stacked_order(ranks, m0, m1):
    """pos (m0 + m1): the position of every stacked site in the ordering (by rank, across both processes)"""
    pos = np.empty(m0 + m1, dtype=np.int64)
    pos[np.argsort(np.asarray(ranks), kind="stable")] = np.arange(m0 + m1)
    return pos


def augmented_ext(n, m):
    """The augmented set (process q: its n[q] data, then its m[q] sites) -> the caller's stacked index: a datum its stacked
    datum index, a site N + its stacked site index"""
    N = n[0] + n[1]
    return np.concatenate([np.arange(n[0]), N + np.arange(m[0]), n[0] + np.arange(n[1]), N + m[0] + np.arange(m[1])])


def local_cosim_reference(params, coords, values, metric, sites0, sites1, ranks, max_dist, caps=(0, 0), noise=None):
    """tests/local_sim_ref.local_sim_reference on the stacked sites.  Per stacked site t: members[t] (stacked caller indices,
    ascending: data 0 .. N - 1, a site N + its stacked index), weights[t], mean[t], var[t], count (m, 4: data of process 0, of
    process 1, earlier sites of process 0, of process 1), level; the scalars n_empty, k_max, n_capped, n_levels, gap, info; and
    draws(eps) for eps (n_draws, m0 + m1)."""
    p = orc.Params.from_flat(params)
    sites = [np.asarray(sites0, dtype=float).reshape(-1, 2), np.asarray(sites1, dtype=float).reshape(-1, 2)]
    n = [len(c) for c in coords]
    mq = [len(s) for s in sites]
    N, m = sum(n), sum(mq)
    aug = [np.vstack([np.asarray(coords[q], dtype=float), sites[q]]) for q in range(2)]
    S = orc.joint_cov(p, aug, metric)
    D, proc = vr.stacked_distances(aug, metric)
    ext = augmented_ext(n, mq)
    pos = stacked_order(ranks, mq[0], mq[1])
    is_s = ext >= N
    aug_rank = np.where(is_s, 0, ext)
    aug_rank[is_s] = N + pos[ext[is_s] - N]
    z = np.zeros(N + m)
    z[~is_s] = np.concatenate([np.asarray(v, dtype=float) for v in values])[ext[~is_s]]
    dd = np.zeros(N + m)
    dd[~is_s] = _noise_diag(coords, noise)[ext[~is_s]]
    S = S + np.diag(dd)
    keep, gap, capped = vr.conditioning_sets(D, proc, aug_rank, max_dist, caps)
    site_row = np.empty(m, dtype=np.int64)
    site_row[ext[is_s] - N] = np.flatnonzero(is_s)
    sproc = np.concatenate([np.zeros(mq[0], dtype=int), np.ones(mq[1], dtype=int)])
    members, weights, nbr_sites = [], [], []
    mean, var = np.zeros(m), np.zeros(m)
    count = np.zeros((m, 4), dtype=np.int64)
    bad = []
    for t in range(m):
        at = site_row[t]
        c = np.flatnonzero(keep[at])
        c = c[np.argsort(ext[c])]
        e = ext[c]
        site = e >= N
        count[t] = [np.count_nonzero(~site & (e < n[0])), np.count_nonzero(~site & (e >= n[0])),
                    np.count_nonzero(site & (e < N + mq[0])), np.count_nonzero(site & (e >= N + mq[0]))]
        members.append(e)
        nbr_sites.append(e[site] - N)
        c0var = p.sigma[sproc[t]] ** 2 + p.nugget[sproc[t]]
        if c.size == 0:
            weights.append(np.zeros(0))
            mean[t], var[t] = 0.0, c0var
            continue
        try:
            np.linalg.cholesky(S[np.ix_(c, c)])
            w = np.linalg.solve(S[np.ix_(c, c)], S[c, at])
        except np.linalg.LinAlgError:
            weights.append(np.full(c.size, np.nan))
            mean[t] = var[t] = np.nan
            bad.append(t)
            continue
        weights.append(w)
        mean[t] = w[~site] @ z[c[~site]]
        var[t] = c0var - S[c, at] @ w
        if not var[t] > 0:
            bad.append(t)
    level = levels_of(pos, nbr_sites)
    ktot = count.sum(axis=1)

    def draws(eps):
        eps = np.asarray(eps, dtype=float)
        Y = np.full(eps.shape, np.nan)
        for t in np.argsort(pos):
            sd = np.sqrt(var[t]) if var[t] > 0 else np.nan
            wsite = weights[t][members[t] >= N]
            Y[:, t] = mean[t] + Y[:, nbr_sites[t]] @ wsite + sd * eps[:, t]
        return Y

    return dict(members=members, weights=weights, mean=mean, var=var, count=count, level=level, pos=pos, nbr_sites=nbr_sites,
                n_empty=int(np.count_nonzero(ktot == 0)), k_max=int(ktot.max()), n_capped=int(np.count_nonzero(capped[site_row])),
                n_levels=int(level.max()), gap=float(gap[site_row].min()), info=(min(bad) + 1) if bad else 0, draws=draws)


def dense_chain_pair(params, coords, values, metric, sites0, sites1, ranks, noise=None):
    """(pred, L_S, order) of the stacked sites: the joint posterior mean, and its covariance C_pp - c0^T Sigma^-1 c0 (C_pp the
    joint covariance of the two site sets, c0 each site's covariances as its own process) in rank order, factored"""
    p = orc.Params.from_flat(params)
    sites = [np.asarray(sites0, dtype=float).reshape(-1, 2), np.asarray(sites1, dtype=float).reshape(-1, 2)]
    Sig = orc.joint_cov(p, coords, metric) + np.diag(_noise_diag(coords, noise))
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    c0 = np.hstack([orc.pred_cross_cov(p, coords, sites[q], q, metric) for q in range(2)])
    Cpp = orc.joint_cov(p, sites, metric)
    pred = c0.T @ np.linalg.solve(Sig, z)
    post = Cpp - c0.T @ np.linalg.solve(Sig, c0)
    order = np.argsort(ranks, kind="stable")
    L = np.linalg.cholesky(post[np.ix_(order, order)])
    return pred, L, order
