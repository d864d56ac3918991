"""Conditional simulation in the moving neighbourhood (include/cokrige.h: ck_simulate_local) as a numpy loop over the sites: the
augmented data set (the sites behind the data of process i as noise-free pseudo-data), the conditioning sets of
tests/vecchia_ref.conditioning_sets on it, dense solves on oracle.joint_cov in float64.  Shared by tests/test_local_sim_host.py
and tests/test_gpu_local_simulation.py."""
import numpy as np

from oracle import cokrige_oracle as orc
from tests import vecchia_ref as vr

# the inputs of the issue's table: (n, m, caps, max_dist), with what the sets must come out as
ROWS = {
    1: dict(n=40, m=50, caps=(6, 6), max_dist=0.12, n_empty=4, k_max=9, ns_max=3, n_levels=4),
    2: dict(n=40, m=50, caps=(6, 6), max_dist=0.2, n_empty=0, k_max=12, ns_max=4, n_levels=7),
    3: dict(n=40, m=300, caps=(8, 8), max_dist=0.2, n_empty=0, k_max=16, ns_max=8, n_levels=27),
    4: dict(n=20, m=24, caps=(0, 0), max_dist=10.0, n_empty=0, k_max=63, ns_max=23, n_levels=24),
}


def row_inputs(row):
    """The problem of a table row: unit_square_problem(n, grid_side=2, seed=20002), sites and ranks from default_rng(7)"""
    from sif_xco2_cokriging_amd import synth
    r = ROWS[row]
    pb = synth.unit_square_problem(r["n"], grid_side=2, seed=20002)
    rng = np.random.default_rng(7)
    sites = rng.random((r["m"], 2))
    ranks = rng.permutation(r["m"]).astype(np.int64)
    return dict(params=list(pb["params"]), coords=pb["coords"], values=pb["values"], metric=pb["metric"], sites=sites, ranks=ranks,
                caps=r["caps"], max_dist=r["max_dist"])


def levels_of(pos, nbr_sites):
    """level per site (the caller's order): 1 + the largest level among its site-neighbours, 1 without any.  pos: position of
    every site in the ordering; nbr_sites[t]: the caller's indices of the earlier sites in the set of site t"""
    m = len(pos)
    level = np.zeros(m, dtype=np.int64)
    for t in np.argsort(pos):
        level[t] = 1 + max((level[u] for u in nbr_sites[t]), default=0)
        assert all(pos[u] < pos[t] for u in nbr_sites[t])
    return level


def local_sim_reference(params, coords, values, metric, i, sites, ranks, max_dist, caps=(0, 0), noise=None):
    """Per site t (the caller's order): members[t] (stacked caller indices, ascending: data 0 .. N - 1, a site N + its index),
    weights[t] in that order, mean[t] = mu_t^data, var[t] = s_t^2 raw, count (m, 3), level; the scalars n_empty, k_max,
    n_capped, n_levels, gap (the smallest relative gap at a cut over the sites) and info; and draws(eps) for eps (n_draws, m).
    noise: per process s_k * d_a (array) or None, on the data's diagonal only."""
    p = orc.Params.from_flat(params)
    n = [len(c) for c in coords]
    N, m = sum(n), len(sites)
    sites = np.asarray(sites, dtype=float)
    aug = [np.asarray(c, dtype=float) for c in coords]
    aug[i] = np.vstack([aug[i], sites])
    S = orc.joint_cov(p, aug, metric)
    D, proc = vr.stacked_distances(aug, metric)
    # augmented stacked index -> the caller's stacked index; the ordering: every datum in front of every site
    off_i = 0 if i == 0 else n[0]
    ext = np.empty(N + m, dtype=np.int64)
    a = 0
    for k in range(len(coords)):
        ext[a:a + n[k]] = (0 if k == 0 else n[0]) + np.arange(n[k])
        a += n[k]
        if k == i:
            ext[a:a + m] = N + np.arange(m)
            a += m
    pos = np.empty(m, dtype=np.int64)
    pos[np.argsort(ranks, kind="stable")] = np.arange(m)
    aug_rank = np.where(ext < N, ext, 0)
    aug_rank[ext >= N] = N + pos[ext[ext >= N] - N]
    z = np.zeros(N + m)
    z[ext < N] = np.concatenate([np.asarray(v, dtype=float) for v in values])[ext[ext < N]]
    if noise is not None:
        d_all = np.concatenate([np.zeros(n[k]) if noise[k] is None else np.asarray(noise[k], dtype=float) for k in range(len(coords))])
        dd = np.zeros(N + m)
        dd[ext < N] = d_all[ext[ext < N]]
        S = S + np.diag(dd)
    keep, gap, capped = vr.conditioning_sets(D, proc, aug_rank, max_dist, caps)
    site_row = off_i + n[i] + np.arange(m)   # the augmented index of the caller's site t
    members, weights, nbr_sites = [], [], []
    mean, var = np.zeros(m), np.zeros(m)
    count = np.zeros((m, 3), dtype=np.int64)
    bad = []
    for t in range(m):
        at = site_row[t]
        c = np.flatnonzero(keep[at])
        c = c[np.argsort(ext[c])]
        e = ext[c]
        is_site = e >= N
        count[t] = [np.count_nonzero(~is_site & (e < n[0])), np.count_nonzero(~is_site & (e >= n[0])), np.count_nonzero(is_site)]
        members.append(e)
        nbr_sites.append(e[is_site] - N)
        c0var = p.sigma[i] ** 2 + p.nugget[i]
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
        mean[t] = w[~is_site] @ z[c[~is_site]]
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
                n_levels=int(level.max()), gap=float(gap[site_row].min()), info=(min(bad) + 1) if bad else 0, draws=draws,
                ns_max=int(count[:, 2].max()))


def dense_chain(params, coords, values, metric, i, sites, ranks, noise=None):
    """(pred, L_S, order): the joint predictor's posterior at the sites, its covariance S = pred_cov - c0^T Sigma^-1 c0 permuted to
    rank order and factored.  draws = pred + (eps[:, order] L_S^T) put back into the caller's order (dense_draws)."""
    p = orc.Params.from_flat(params)
    Sig = orc.joint_cov(p, coords, metric)
    if noise is not None:
        Sig = Sig + np.diag(np.concatenate([np.zeros(len(c)) if d is None else np.asarray(d, dtype=float)
                                            for c, d in zip(coords, noise)]))
    z = np.concatenate([np.asarray(v, dtype=float) for v in values])
    c0 = orc.pred_cross_cov(p, coords, sites, i, metric)
    Cpp = orc.pred_cov(p, sites, i, metric)
    pred = c0.T @ np.linalg.solve(Sig, z)
    post = Cpp - c0.T @ np.linalg.solve(Sig, c0)
    order = np.argsort(ranks, kind="stable")
    L = np.linalg.cholesky(post[np.ix_(order, order)])
    return pred, L, order


def dense_draws(pred, L, order, eps):
    Y = np.empty(np.shape(eps))
    Y[:, order] = np.asarray(eps)[:, order] @ L.T
    return pred + Y
