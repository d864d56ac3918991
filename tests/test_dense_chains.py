"""Host-only tests of tests/dense_chains.py: the references of tests/test_gpu_entry_edge_sizes.py against each other, and
the conditioning of every data set that module runs on (so that a tolerance missed on the GPU is the library's doing)."""
import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import dense_chains as dc


def err(a, b):
    """the measure of test_gradient_against_dense_differences: relative where the reference exceeds 1, else absolute"""
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))


@pytest.mark.parametrize("name,metric", [("BIV", dc.HAV), ("BIV_EUC", dc.EUC), ("BIV_HALF", dc.HAV), ("UNI", dc.HAV)])
@pytest.mark.parametrize("n0,n1", [(5, 3), (40, 37)])
def test_cached_blocks_are_the_oracles_joint_cov(n0, n1, name, metric):
    coords, _ = dc.make_data(40, dc.PARAMS[name], metric, n0, n1)
    cache = dc.CovCache(coords, metric)
    x = np.array(dc.PARAMS[name])
    for k in range(-1, x.size):   # the base point and one shifted point per parameter, on one cache
        y = x.copy()
        if k >= 0:
            y[k] += dc.fd_steps(x)[k]
        p = orc.Params.from_flat(y)
        assert np.array_equal(cache.joint_cov(p), orc.joint_cov(p, coords, metric)), k


@pytest.mark.parametrize("name,metric", [("BIV", dc.HAV), ("BIV_EUC", dc.EUC), ("BIV_HALF", dc.HAV), ("UNI", dc.HAV)])
@pytest.mark.parametrize("n0,n1", [(5, 3), (40, 37)])
def test_trace_gradient_against_differences_of_the_likelihood(n0, n1, name, metric):
    par = dc.PARAMS[name]
    coords, values = dc.make_data(40, par, metric, n0, n1)
    g = dc.dense_ll_grad(par, coords, values, metric)
    fd = dc.fd_grad(par, coords, values, metric)
    floor = err(dc.fd_grad(par, coords, values, metric, 0.5), fd)   # what halving the step changes: fd_grad's own accuracy
    print(f"N = ({n0}, {n1}) {name}: tr(G dSigma) against fd_grad {err(g, fd):.2e}, fd_grad's floor {floor:.2e}")
    # measured floors: (5, 3) 6.0e-11 BIV, 3.3e-11 BIV_EUC, 3.2e-11 BIV_HALF, 6.2e-12 UNI;
    # (40, 37) 5.6e-11, 6.6e-10, 1.3e-10, 2.1e-10 -- the agreement was 6.4e-11, 2.2e-11, 3.5e-11, 6.6e-12 and
    # 4.1e-11, 7.1e-10, 5.7e-11, 3.6e-11
    assert err(g, fd) <= 10 * floor
    # the full difference of orc.joint_cov (every block, not only those theta_k enters) gives the same contraction
    S = orc.joint_cov(orc.Params.from_flat(par), coords, metric)
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    a = Si @ np.concatenate(values)
    dS = dc.fd_of(lambda y: orc.joint_cov(orc.Params.from_flat(y), coords, metric), par)
    full = 0.5 * np.einsum("pq,kpq->k", np.outer(a, a) - Si, dS)
    assert err(g, full) < 1e-12   # the same differences, summed block by block: rounding of the sums only


@pytest.mark.parametrize("name,metric,kind,n0,n1", [("BIV", dc.HAV, "linear", 40, 37), ("BIV_EUC", dc.EUC, "constant", 40, 37),
                                                    ("UNI", dc.HAV, "wide", 45, 0), ("BIV", dc.HAV, "constant", 5, 3)])
def test_reml_gradient_against_differences_of_reml(name, metric, kind, n0, n1):
    """the value as test_reml_value_and_gradient computes it (dense_reml is that test's), the gradient against its FD"""
    par = dc.PARAMS[name]
    coords, values = dc.make_data(41, par, metric, n0, n1, shift=0.3)
    Fs = [dc.design(kind, c, c) for c in coords]
    g = dc.dense_reml_grad(par, coords, values, metric, Fs)
    fd = dc.fd_of(lambda y: dc.dense_reml(y, coords, values, metric, Fs)[0], par)
    floor = err(dc.fd_of(lambda y: dc.dense_reml(y, coords, values, metric, Fs)[0], par, 0.5), fd)
    print(f"{name} {kind}: tr(G_R dSigma) against FD of l_R {err(g, fd):.2e}, FD floor {floor:.2e}")
    assert err(g, fd) <= 10 * floor
    # l_R through the projection: z^T P z and log|X^T Sigma^-1 X| against the bordered determinant identity
    # log|[[Sigma, X], [X^T, 0]]| = log|Sigma| + log|X^T Sigma^-1 X| (sign (-1)^q)
    S = orc.joint_cov(orc.Params.from_flat(par), coords, metric)
    X = dc.block_X(Fs)
    q = X.shape[1]
    _, ld = np.linalg.slogdet(np.block([[S, X], [X.T, np.zeros((q, q))]]))
    lR, ldS, ldA, quad = dc.dense_reml(par, coords, values, metric, Fs)
    assert abs(ld - (ldS + ldA)) < 1e-9 * max(1.0, abs(ld))
    # no trend columns at all: REML is the likelihood
    l0 = dc.dense_ll(par, coords, values, metric)
    assert abs(dc.dense_reml(par, coords, values, metric, [np.zeros((len(c), 0)) for c in coords])[0] - l0[0]) < 1e-12 * abs(l0[0])


@pytest.mark.parametrize("kind", ["constant", "linear", "wide"])
def test_bordered_solve_is_the_gls_form(kind):
    par = dc.PARAMS["BIV"]
    p = orc.Params.from_flat(par)
    coords, values = dc.make_data(42, par, dc.HAV, 12, 10, shift=0.3)
    Fs = [dc.design(kind, c, c) for c in coords]
    for i in (0, 1):
        pc = np.vstack([dc.pred_sites(np.random.default_rng(i), dc.HAV, 9), coords[i][:2]])   # two sites on data
        F0 = dc.design(kind, coords[i], pc)
        pred, var, beta, cov = dc.dense_universal(p, coords, values, pc, i, dc.HAV, Fs, F0)
        gp, gv, gb = dc.gls_universal(p, coords, values, pc, i, dc.HAV, Fs, F0)
        assert dc.rel(pred, gp) < 1e-10 and np.max(np.abs(var - gv)) < 1e-10 and dc.rel(beta, gb) < 1e-10
        assert np.max(np.abs(pred[-2:] - values[i][:2])) < 1e-9 and np.max(np.abs(var[-2:])) < 1e-9   # exact on data


def test_chain_draws_have_the_posterior_covariance():
    """L L^T of the kept sites is S there, a deflated site's draw is pred, and the order of the sites does not change
    the distribution (two orders give the same L L^T)"""
    ds = dc.data_set(dc.SMALL)
    pc, on = dc.draw_sites(ds, 1, 40, 3, 7)
    pred, S = dc.posterior(ds.p, ds.coords, ds.values, pc, 1, ds.metric, ds.cf)
    assert np.max(np.abs(np.diag(S)[on])) < 1e-12 and np.min(np.diag(S)[~on]) > 1e-3
    for perm in (np.arange(40), np.random.default_rng(1).permutation(40)):
        kept, L = dc.chain_factor(S, on, perm)
        assert np.max(np.abs(L @ L.T - S[np.ix_(kept, kept)])) < 1e-14
        eps = np.eye(40)
        d = dc.chain_draws(pred, S, on, perm, eps) - pred
        assert not d[:, on].any()
        assert np.max(np.abs(d.T @ d - np.where(np.outer(on, on) | np.outer(on, ~on) | np.outer(~on, on), 0.0, S))) < 1e-13


def test_block_labels_cover_the_fold_kernels_cases():
    rng = np.random.default_rng(0)
    for r in dc.BLOCK_R:
        n = np.bincount(dc.block_labels(rng, r, dc.BLOCK_M), minlength=r)
        assert n.sum() == dc.BLOCK_M and n.min() >= 1
        if r >= 6:
            assert list(n[:5]) == [1, 3, 4, 5, 8] and n[5] > dc.BLOCK_M // 2
    assert sorted(dc.block_labels(rng, 40, 40)) == list(range(40))


# ---- the conditioning condition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.DATA_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[3]}")
def test_every_data_set_is_well_conditioned(case):
    ds = dc.data_set(case)
    np.linalg.cholesky(ds.S)
    cond = np.linalg.cond(ds.S)
    print(f"{case}: cond(Sigma) = {cond:.3g}")
    assert cond < 1e8
    n0, n1 = case[:2]
    assert [len(c) for c in ds.coords] == ([n0, n1] if ds.p.n_procs == 2 else [n0])
    if ds.p.n_procs == 2 and min(n0, n1) >= 2:   # co-located pairs across the processes: h == 0 off the diagonal
        assert (orc.distance_matrix(ds.coords[0], ds.coords[1], ds.metric) == 0).sum() >= min(n0, n1) // 2


@pytest.mark.parametrize("case", dc.DRAW_CASES, ids=lambda c: f"{c[0][0]}-{c[0][1]}-i{c[1]}-m{c[2]}")
def test_every_draw_case_factors_without_jitter(case):
    data, i, m, n_on, seed = case
    ds = dc.data_set(data)
    pc, on = dc.draw_sites(ds, i, m, n_on, seed)
    assert len(pc) == m and on.sum() == n_on and len(np.unique(pc, axis=0)) == m
    pred, S = dc.posterior(ds.p, ds.coords, ds.values, pc, i, ds.metric, ds.cf)
    c0 = ds.p.sigma[i] ** 2 + ds.p.nugget[i]
    assert np.array_equal(np.diag(S) <= 1e-10 * c0, on)   # the library's deflation rule picks exactly the sites on data
    dc.chain_factor(S, on, np.arange(m))               # numpy's Cholesky of the kept part, no jitter
