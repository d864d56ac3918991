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


# ---- the Fisher reference -----------------------------------------------------------------------------------------------------
def fisher_id(c):
    return f"{c[0]}-{c[1]}-{c[3]}"


# Measured floors of dense_fisher -- what halving _d4's step changes, in normalised()'s measure -- per class (exact,
# length scale, nu); the exact class does not see the step at all:
#   BIV (1, 1) 0 / 2.3e-11 / 5.7e-11, (5, 3) 0 / 3.2e-12 / 2.9e-11, (63, 65) 0 / 2.2e-12 / 4.4e-11, (64, 64) 0 / 2.1e-12 / 4.3e-11,
#   (64, 1) 0 / 8.3e-13 / 8.4e-11, (448, 64) 0 / 3.6e-12 / 7.1e-11, (449, 63) 0 / 3.6e-12 / 7.1e-11, (511, 1) 0 / 3.9e-12 / 7.4e-11,
#   (512, 512) 0 / 8.9e-12 / 7.1e-11, (513, 511) 0 / 8.9e-12 / 7.1e-11, (1, 600) 0 / 9.8e-12 / 2.1e-11, (576, 100) 0 / 3.8e-12 / 7.8e-11,
#   (513, 511) BIV_EUC 0 / 3.2e-11 / 7.3e-11, BIV_HALF 0 / 1.5e-11 / 1.1e-10; UNI 1: no live differenced slot, 64 0 / 9.8e-13 / 6.5e-11,
#   65 0 / 9.7e-13 / 6.3e-11, 512 0 / 4.7e-12 / 7.0e-11, 513 0 / 5.0e-12 / 7.2e-11.
# Over all differenced slots together the largest is 1.1e-10; every length-scale floor is below 1e-10, so dc.FISHER_LEN_FLOOR is
# empty and the length-scale bound is 1e-9 on every rung.
@pytest.mark.parametrize("case", dc.FISHER_CASES, ids=fisher_id)
def test_fisher_reference_floor(case):
    ds = dc.data_set(case)
    ref = dc.dense_fisher(ds.params, ds.coords, ds.metric)
    half = dc.dense_fisher(ds.params, ds.coords, ds.metric, scale=0.5)
    e = dc.class_errors(dc.normalised(half, ref), len(ds.params))
    print(f"{case}: floor of dense_fisher exact {e['exact']:.2e} length scale {e['len']:.2e} nu {e['nu']:.2e}")
    tol = dc.fisher_tol(case)
    assert e["exact"] == 0.0          # the exact block expressions do not see the step
    assert 10.0 * e["len"] <= tol["len"]   # the bound of the GPU module is at least ten floors
    assert e["nu"] < tol["nu"] / 10
    dead = [k for k in range(13) if ref[k, k] == 0.0]
    n = [k for k in case[:2] if k > 0]
    s = dc.SLOTS[len(ds.params)]
    want = [k for k in range(13) if k not in s["exact"] + s["len"] + s["nu"] or k >= 11]
    if len(n) == 1:
        want += [1, 2] if n[0] == 1 else []
    else:   # a process of one site: its nu and length scale do not enter; rho = 0: nor do nu_12 and len_12
        want += ([2, 5] if n[0] == 1 else []) + ([4, 7] if n[1] == 1 else []) + ([3, 6] if ds.p.rho == 0.0 else [])
    assert sorted(dead) == sorted(set(want)), (dead, want)


@pytest.mark.parametrize("n0,n1", [(5, 3), (63, 65), (64, 1)])
def test_fisher_reference_identities(n0, n1):
    """symmetric, positive semi-definite on the live slots, and -- v = (sigma, 0 .., 2 nugget, 0): sum_k v_k D_k = 2 Sigma --
    v^T I v = 2 N (ML) and 2 (N - p) (REML)"""
    ds = dc.data_set((n0, n1, 40, "BIV", dc.HAV))
    par = ds.params
    v = np.zeros(13)
    v[0], v[1], v[8], v[9] = par[0], par[1], 2 * par[8], 2 * par[9]
    for kind in (None, "constant", "wide"):
        X = None if kind is None else dc.block_X([dc.design(k, c, c) for k, c in zip(dc.trend_kinds(ds, kind), ds.coords)])
        q = 0 if X is None else X.shape[1]   # "wide": 16 at (63, 65); 9 at (64, 1) and 2 at (5, 3), where a process with
        assert ds.N - q >= 2                  # fewer than eight data gets the constant design (dc.trend_kinds)
        ref = dc.dense_fisher(par, ds.coords, ds.metric, X=X)
        assert np.array_equal(ref, ref.T)
        gone = dc.annihilated_slots([n0, n1], None if kind is None else dc.trend_kinds(ds, kind))
        if gone:   # (64, 1) with a column on the one-site process: 0 up to rounding in the scale of the ML information
            assert dc.ml_scaled(ref, dc.dense_fisher(par, ds.coords, ds.metric), gone) <= 1e-12
            ref = dc.drop_slots(ref, gone)
        live = np.flatnonzero(np.diag(ref) > 0)
        s = 1.0 / np.sqrt(np.diag(ref)[live])
        w = np.linalg.eigvalsh(ref[np.ix_(live, live)] * np.outer(s, s))
        print(f"({n0}, {n1}) {kind}: p = {q}, smallest eigenvalue of the unit-diagonal scaling {w.min():.2e}, "
              f"v^T I v / 2(N - p) - 1 = {v @ ref @ v / (2 * (ds.N - q)) - 1:.2e}")
        assert w.min() >= -1e-12
        assert abs(v @ ref @ v - 2 * (ds.N - q)) <= 1e-9 * 2 * (ds.N - q)


# ---- the fold reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(63, 65), (5, 3)])
def test_dense_folds_against_refitting_without_the_fold(n0, n1):
    ds = dc.data_set((n0, n1, 40, "BIV", dc.HAV))
    for i in (0, 1):
        for other, minus in dc.FOLD_VARIANTS:
            fi, fo, sizes = dc.fold_labels(ds.case, i, other, minus)
            pred, var, stats = dc.folds_reference(ds.S, ds.z, [n0, n1], i, fi, fo)
            rp, re = dc.oracle_folds(ds.p, ds.coords, ds.values, ds.metric, i, fi, fo)
            sel = fi >= 0
            assert np.array_equal(np.isnan(pred), ~sel) and np.array_equal(np.isnan(rp), ~sel)
            dp, dv = np.max(np.abs(pred[sel] - rp[sel])), np.max(np.abs(var[sel] - re[sel] ** 2))
            print(f"({n0}, {n1}) i={i} other={other} minus={minus}: folds {sizes}, pred {dp:.2e} variance {dv:.2e}")
            assert dp < 1e-9 and dv < 1e-10
            assert list(stats[:, 0]) == sizes


def test_fold_labels_cover_every_fold_and_size():
    for case, i in dc.FOLD_CASES:
        n = [k for k in case[:2] if k > 0]
        for other, minus in dc.FOLD_VARIANTS:
            if len(n) == 1 and other:
                continue
            fi, fo, sizes = dc.fold_labels(case, i, other, minus)
            assert len(fi) == n[i] and (fo is None) == (not other or len(n) == 1)
            assert fo is None or len(fo) == n[1 - i]
            cnt_i = np.bincount(fi[fi >= 0], minlength=len(sizes))
            cnt = cnt_i + (np.bincount(fo[fo >= 0], minlength=len(sizes)) if fo is not None else 0)
            assert cnt_i.min() >= 1 and list(cnt) == sizes, (case, i, other, minus, cnt, sizes)
            total = n[i] + (n[1 - i] if fo is not None else 0)
            if n[i] == 1:
                assert len(sizes) == 1
            elif n[i] >= 5 and total >= 70:   # the advertised sizes: two singletons, a pair, 64 and the rest
                assert sizes[:4] == [1, 1, 2, 64] and sizes[4] == total - 68 - (max(1, total // 10) if minus else 0)
            if minus:
                assert (fi < 0).sum() + (0 if fo is None else (fo < 0).sum()) >= (1 if total >= 3 else 0)
            if other and fo is not None and n[i] >= 5 and total >= 70:
                assert (fo >= 0).any()   # the folds reach the other process


# ---- what the GPU tests would notice, shown on the references -----------------------------------------------------------------
def test_references_move_with_the_errors_the_gpu_tests_are_for():
    """an indexing error at the process boundary moves the references by more than 100 x the bounds the GPU module holds
    the library to (1e-8 / 1e-9 for folds, 1e-9 for the exact and length-scale Fisher slots)"""
    ds = dc.data_set(dc.SMALL)
    n0, n1 = ds.case[:2]
    d = dc.noise_of(ds)
    Sn = ds.S + np.diag(np.concatenate([s * x for s, x in zip(dc.NOISE_SCALES, d)]))
    fi, fo, _ = dc.fold_labels(ds.case, 0, True, False)
    pred, var, stats = dc.folds_reference(Sn, ds.z, [n0, n1], 0, fi, fo)
    # 1. one fold label across the n0 boundary: the last datum of process 0 in the largest fold gives its label to the first
    # datum of process 1 outside that fold
    f2, o2 = fi.copy(), fo.copy()
    big = int(np.argmax(np.bincount(fi[fi >= 0])))
    a, b = np.flatnonzero(fo != big)[0], np.flatnonzero(fi == big)[-1]
    f2[b], o2[a] = fo[a], big
    pred2, var2, _ = dc.folds_reference(Sn, ds.z, [n0, n1], 0, f2, o2)
    keep = (fi == big) & (f2 == big)
    dp = np.max(np.abs(pred2[keep] - pred[keep]) / np.maximum(1.0, np.abs(pred[keep])))
    dv = np.max(np.abs(var2[keep] - var[keep]))
    print(f"a fold label moved across the boundary: pred {dp:.2e} variance {dv:.2e} (datum {b} of process 0 <-> {a} of process 1)")
    assert dp > 100 * 1e-8 and dv > 100 * 1e-9
    # 2. the noise variances of the last datum of process 0 and the first of process 1 swapped
    dv2 = np.concatenate([s * x for s, x in zip(dc.NOISE_SCALES, d)])
    dv2[[n0 - 1, n0]] = dv2[[n0, n0 - 1]]
    singles = (np.arange(n0, dtype=np.int32), None)
    p1, v1, _ = dc.folds_reference(Sn, ds.z, [n0, n1], 0, *singles)
    p2, v2, _ = dc.folds_reference(ds.S + np.diag(dv2), ds.z, [n0, n1], 0, *singles)
    dp = np.max(np.abs(p2 - p1) / np.maximum(1.0, np.abs(p1)))
    dv = np.max(np.abs(v2 - v1))
    print(f"two noise variances swapped across the boundary: pred {dp:.2e} variance {dv:.2e}")
    assert dp > 100 * 1e-8 and dv > 100 * 1e-9
    # 3. column n0 - 1 dropped from a D_k
    S = dc.dense_sigma(ds.params, ds.coords, ds.metric)
    D = dc.derivative_matrices(ds.params, ds.coords, ds.metric)
    ref = dc.fisher_of(S, D)
    for k in (0, 5, 10):   # sigma_11 (exact), len_11 (length scale), rho (exact, the cross block)
        D2 = dict(D)
        D2[k] = D[k].copy()
        D2[k][:, n0 - 1] = 0.0
        e = dc.normalised(dc.fisher_of(S, D2), ref)
        print(f"column n0 - 1 dropped from D_{k}: slot ({k}, {k}) moves by {e[k, k]:.2e}, the largest entry by {e.max():.2e}")
        assert e[k, k] > 100 * 1e-9
