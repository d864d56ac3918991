"""GPU tests of universal cokriging in the moving neighbourhood: include/cokrige.h ck_predict_local_universal,
native.Handle.predict_local_universal and point_prediction.Predictor(trend=...) against a per-site numpy chain built from the
oracle's distances and covariances, in two independent forms: Cholesky + GLS, and the bordered Lagrange system
[[Sigma_loc, X], [X^T, 0]].

Tolerances are the local path's own (tests/test_gpu_local.py): rtol 1e-8, atol 1e-10 on pred and on pred_err^2; beta at rtol
1e-8 against the GLS form.  A site is left out of the numeric comparison -- its NaN pattern and the counters are still
checked -- only where the two numpy forms disagree with each other by more than a tenth of that tolerance (the conditioning of
that neighbourhood's system, not the code under test, then decides the digits); a case may leave out at most 5 % of its sites."""
import warnings

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_EUC = [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.02, 0.025, -0.19]
BIV_NONUG = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.0, 0.0, -0.19]
UNI = [1.1, 0.6, 380.0, 0.03]
OK, EMPTY, NOT_PD, RANK_DEF = 0, 1, 2, 3
RTOL, ATOL = 1e-8, 1e-10
TREND_TOL = 1e-10


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_data(seed, params, metric, n0=700, n1=650):
    """as make_data of tests/test_gpu_universal.py"""
    rng = np.random.default_rng(seed)
    p = orc.Params.from_flat(params)
    m = n0 + n1
    if metric == HAV:
        pts = np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])
    else:
        pts = np.column_stack([rng.uniform(0, 10, m), rng.uniform(0, 10, m)])
    coords = [pts[:n0].copy()] if p.n_procs == 1 else [pts[:n0].copy(), pts[n0 // 2:n0 // 2 + n1].copy()]
    S = orc.joint_cov(p, coords, metric)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
    values = np.split(z, np.cumsum([len(c) for c in coords])[:-1])
    return p, coords, [v + 0.3 for v in values]   # a mean the zero-mean model does not know


def pred_sites(rng, metric, m=120):
    """slightly beyond the data's bounding box"""
    if metric == HAV:
        return np.column_stack([rng.uniform(24, 51, m), rng.uniform(-122, -68, m)])
    return np.column_stack([rng.uniform(-0.4, 10.4, m), rng.uniform(-0.4, 10.4, m)])


def handle(native, p, coords, values, metric, site_order=1):
    h = native.Handle(0)
    if site_order != 1:
        h.set_option("site_order", site_order)
    if p.n_procs == 2:
        h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                    p.nugget, p.rho)
    else:
        h.set_model(1, p.sigma, [p.nu[0, 0]] * 3, [p.len_scale[0, 0]] * 3, p.nugget, 0.0)
    h.set_metric(metric)
    for k in range(p.n_procs):
        h.set_data(k, coords[k], values[k])
    return h


def design(kind, coords_k, pts):
    """the library's trend designs, written out here: "constant", "linear" (scaled by the process's data sites), "cov"
    (constant + a non-coordinate covariate)"""
    if kind == "constant":
        return np.ones((len(pts), 1))
    if kind == "linear":
        mu, sd = coords_k.mean(0), coords_k.std(0)
        return np.column_stack([np.ones(len(pts)), (pts - mu) / sd])
    return np.column_stack([np.ones(len(pts)), np.sin(pts[:, 0] / 7.0) * np.cos(pts[:, 1] / 11.0)])


def chol_threshold(A, tol=TREND_TOL):
    """left-looking Cholesky with the relative pivot threshold of the rules; None: rank deficient"""
    n = len(A)
    R = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - R[j, :j] @ R[j, :j]
        if not (A[j, j] > 0.0) or not (d > tol * A[j, j]) or not np.isfinite(d):
            return None
        R[j, j] = np.sqrt(d)
        R[j + 1:, j] = (A[j + 1:, j] - R[j + 1:, :j] @ R[j, :j]) / R[j, j]
    return R


class Reference:
    """per-site numpy chain: neighbours by the oracle's distance, the rules of include/cokrige.h, two forms"""

    def __init__(self, p, coords, values, metric, Fs):
        self.p, self.coords, self.values, self.metric, self.Fs = p, coords, values, metric, Fs
        n = p.n_procs
        self.Sigma = {}
        for a in range(n):
            for b in range(a, n):
                d = orc.distance_matrix(coords[a], coords[b], metric)
                self.Sigma[a, b] = orc.covariance(p, a, d) if a == b else orc.cross_covariance(p, a, b, d)
        self.pk = [F.shape[1] for F in Fs]

    def __call__(self, pc, i, max_dist, F0, cv=False):
        p, n = self.p, self.p.n_procs
        m, P = len(pc), sum(self.pk)
        off = [0, self.pk[0]]
        c00 = p.sigma[i] ** 2 + p.nugget[i]
        out = dict(pred=np.full(m, np.nan), var=np.full(m, np.nan), beta=np.full((m, P), np.nan), status=np.zeros(m, int),
                   pred2=np.full(m, np.nan), var2=np.full(m, np.nan), k=np.zeros(m, int), simple_var=np.full(m, np.nan),
                   dropped=np.zeros(m, bool))
        for s in range(m):
            if not np.all(np.isfinite(F0[s])):
                out["status"][s] = -1   # rule 5: NaN, in no counter
                continue
            dists = [orc.distance_matrix(pc[s], c, self.metric)[0] for c in self.coords]
            ix = [d <= max_dist for d in dists]
            if cv:
                ix[i] = (dists[i] > 0) & (dists[i] <= max_dist)
            nk = [int(x.sum()) for x in ix]
            k = sum(nk)
            out["k"][s] = k
            if k == 0:
                out["status"][s] = EMPTY
                continue
            z = np.hstack([np.asarray(self.values[a])[ix[a]] for a in range(n)])
            c = np.hstack([orc.covariance(p, i, dists[a][ix[a]], use_nugget=True) if a == i else
                           orc.cross_covariance(p, i, a, dists[a][ix[a]]) for a in range(n)])
            blk = {}
            for a in range(n):
                for b in range(n):
                    blk[a, b] = self.Sigma[a, b][np.ix_(ix[a], ix[b])] if a <= b else self.Sigma[b, a][np.ix_(ix[b], ix[a])].T
            S = np.block([[blk[a, b] for b in range(n)] for a in range(n)])
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                out["status"][s] = NOT_PD
                continue
            X = np.zeros((k, P))
            x0 = np.zeros(P)
            r0 = 0
            for a in range(n):
                X[r0:r0 + nk[a], off[a]:off[a] + self.pk[a]] = self.Fs[a][ix[a]]
                r0 += nk[a]
            x0[off[i]:off[i] + self.pk[i]] = F0[s]
            gone = [a for a in range(n) if self.pk[a] > 0 and nk[a] == 0]
            if i in gone:
                out["status"][s] = RANK_DEF
                continue
            keep = np.array([j for a in range(n) if a not in gone for j in range(off[a], off[a] + self.pk[a])], dtype=int)
            out["dropped"][s] = len(gone) > 0
            v, y = solve_triangular(L, c, lower=True), solve_triangular(L, z, lower=True)
            out["simple_var"][s] = c00 - v @ v
            U = solve_triangular(L, X[:, keep], lower=True) if len(keep) else np.zeros((k, 0))
            A, b = U.T @ U, U.T @ y
            if len(keep) and chol_threshold(A) is None:
                out["status"][s] = RANK_DEF
                continue
            r = x0[keep] - U.T @ v
            beta = np.linalg.solve(A, b) if len(keep) else np.zeros(0)
            out["pred"][s] = v @ y + r @ beta
            out["var"][s] = c00 - v @ v + (r @ np.linalg.solve(A, r) if len(keep) else 0.0)
            out["beta"][s, keep] = beta
            # second form: the bordered Lagrange system
            q = len(keep)
            K = np.block([[S, X[:, keep]], [X[:, keep].T, np.zeros((q, q))]])
            sol = np.linalg.solve(K, np.concatenate([c, x0[keep]]))
            lam, mu = sol[:k], sol[k:]
            out["pred2"][s] = lam @ z
            out["var2"][s] = c00 - lam @ c - mu @ x0[keep]
        return out


def compare(pred, err, info, ref, beta=None, max_left_out=0.05):
    """NaN pattern and counters exactly; numbers at the local path's tolerances where the two numpy forms agree"""
    st = ref["status"]
    assert np.array_equal(np.isnan(pred), st != OK) and np.array_equal(np.isnan(err), st != OK)
    assert info["n_empty"] == int((st == EMPTY).sum())
    assert info["n_not_pd"] == int((st == NOT_PD).sum())
    assert info["n_rank_def"] == int((st == RANK_DEF).sum())
    assert info["k_max"] == int(ref["k"].max())
    ok = st == OK
    agree = ok.copy()
    agree[ok] = ((np.abs(ref["pred"][ok] - ref["pred2"][ok]) <= 0.1 * (RTOL * np.abs(ref["pred"][ok]) + ATOL)) &
                 (np.abs(ref["var"][ok] - ref["var2"][ok]) <= 0.1 * (RTOL * np.abs(ref["var"][ok]) + ATOL)))
    n_out = int(ok.sum() - agree.sum())
    print(f"sites {len(st)} finite {int(ok.sum())} left out {n_out} rank_def {info['n_rank_def']} empty {info['n_empty']} "
          f"dropped {int(ref['dropped'][ok].sum())} k {int(ref['k'].min())}..{int(ref['k'].max())} "
          f"max |dpred| {np.max(np.abs(pred[agree] - ref['pred'][agree]), initial=0):.2e} "
          f"max |dvar| {np.max(np.abs(err[agree] ** 2 - np.maximum(ref['var'][agree], 0)), initial=0):.2e}")
    assert n_out <= max_left_out * len(st)
    np.testing.assert_allclose(pred[agree], ref["pred"][agree], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err[agree] ** 2, np.maximum(ref["var"][agree], 0.0), rtol=RTOL, atol=ATOL)
    if beta is not None:
        assert np.array_equal(np.isnan(beta), np.isnan(ref["beta"]))   # dropped columns, and whole rows where pred is NaN
        fin = agree[:, None] & ~np.isnan(ref["beta"])
        np.testing.assert_allclose(beta[fin], ref["beta"][fin], rtol=RTOL, atol=ATOL)
    return agree


def run_case(native, params, metric, kind, i, max_dist, data=None, pc=None, cv=False, tile_min=None, bad_rows=()):
    p, coords, values = data if data is not None else make_data(3, params, metric)
    if pc is None:
        pc = pred_sites(np.random.default_rng(17), metric)
    Fs = [design(kind, c, c) for c in coords]
    F0 = design(kind, coords[i], pc)
    for s in bad_rows:
        F0[s, -1] = np.nan
    h = handle(native, p, coords, values, metric)
    if tile_min is not None:
        h.set_option("local_tile_min", tile_min)
    for k in range(p.n_procs):
        h.set_trend(k, Fs[k])
    pred, err, info = h.predict_local_universal(i, pc, F0, max_dist=max_dist, cv=cv, want_beta=True)
    ref = Reference(p, coords, values, metric, Fs)(pc, i, max_dist, F0, cv=cv)
    compare(pred, err, info, ref, beta=info["beta"])
    h.close()
    return pred, err, info, ref


# ---- 1. parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist", [250.0, 400.0, 900.0])   # LDS class | both classes in one call | tiled class
@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("kind", ["constant", "linear", "cov"])
def test_parity_haversine(native, kind, i, max_dist):
    pred, err, info, ref = run_case(native, BIV, HAV, kind, i, max_dist)
    if max_dist == 250.0:
        assert ref["k"].max() <= 64
        if kind == "linear":   # both degenerate rules are exercised by these inputs
            assert info["n_rank_def"] > 0
    if max_dist == 400.0:
        assert ref["k"].min() <= 64 < ref["k"].max()
    if max_dist == 900.0:
        assert ref["k"].min() > 64


def test_parity_dropped_columns_and_nonfinite_regressors(native):
    """250 km: some sites see one process only (rule 3), two have no neighbour (rule 1), two get a NaN regressor (rule 5)"""
    seen = 0
    pc = np.vstack([pred_sites(np.random.default_rng(17), HAV, 118), [[10.0, -170.0], [62.0, -95.0]]])   # two sites far away
    for i in (0, 1):
        pred, err, info, ref = run_case(native, BIV, HAV, "cov", i, 250.0, pc=pc, bad_rows=(3, 77))
        assert np.isnan(pred[3]) and np.isnan(pred[77]) and ref["status"][3] == -1 and info["n_empty"] >= 2
        seen += int(ref["dropped"][ref["status"] == OK].sum())
    assert seen > 0


@pytest.mark.parametrize("tile_min", [None, 0])   # 0: everything on the tiled path, the smallest systems included
def test_parity_euclidean(native, tile_min):
    run_case(native, BIV_EUC, EUC, "linear", 1, 1.6, tile_min=tile_min)


@pytest.mark.parametrize("kind,max_dist", [("constant", 250.0), ("linear", 500.0)])
def test_parity_univariate(native, kind, max_dist):
    run_case(native, UNI, HAV, kind, 0, max_dist)


# ---- 2. padding boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes", [
    ("constant", [(31, 31), (32, 31), (32, 32), (33, 32), (62, 62), (63, 62), (94, 94), (95, 94)]),   # k + 4: 66 .. 69, 128, 129, 192, 193
    ("linear", [(28, 28), (29, 28), (60, 60), (61, 60), (92, 92), (93, 92)]),                         # k + 8: 64, 65, 128, 129, 192, 193
])
def test_padding_boundaries(native, kind, sizes):
    p, coords, values = make_data(41, BIV, HAV, n0=120, n1=110)
    pc = pred_sites(np.random.default_rng(5), HAV, 9)
    for n0, n1 in sizes:
        data = (p, [coords[0][:n0], coords[1][:n1]], [values[0][:n0], values[1][:n1]])
        for i in (0, 1):
            pred, err, info, ref = run_case(native, BIV, HAV, kind, i, 1e9, data=data, pc=pc)
            assert info["k_max"] == n0 + n1 and info["n_rank_def"] == 0


# ---- 3. the whole data set as the neighbourhood: the joint universal predictor --------------------------------------
@pytest.mark.parametrize("kind", ["constant", "linear"])
def test_infinite_radius_matches_joint(native, kind):
    p, coords, values = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    Fs = [design(kind, c, c) for c in coords]
    h = handle(native, p, coords, values, HAV)
    for k in range(2):
        h.set_trend(k, Fs[k])
    h.assemble_joint()
    assert h.factor() == 0
    for i in (0, 1):
        F0 = design(kind, coords[i], pc)
        jp, je, jb, _ = h.predict_universal(i, pc, F0)
        pred, err, info = h.predict_local_universal(i, pc, F0, max_dist=1e9, want_beta=True)
        assert info["k_max"] == 1350 and info["n_empty"] == info["n_not_pd"] == info["n_rank_def"] == 0
        print(f"{kind} i={i}: pred {np.max(np.abs(pred - jp)) / np.max(np.abs(jp)):.2e} var {np.max(np.abs(err ** 2 - je ** 2)):.2e}")
        assert np.max(np.abs(pred - jp)) / np.max(np.abs(jp)) < 1e-8
        assert np.max(np.abs(err ** 2 - je ** 2)) < 1e-9
        np.testing.assert_allclose(info["beta"], np.broadcast_to(jb, info["beta"].shape), rtol=1e-8, atol=1e-10)


# ---- 4. no trend -------------------------------------------------------------------------------------------------
def test_no_trend_is_predict_local(native):
    p, coords, values = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    h = handle(native, p, coords, values, HAV)
    base = h.predict_local(0, pc, max_dist=400.0)
    pred, err, info = h.predict_local_universal(0, pc, None, max_dist=400.0, want_beta=True)
    assert np.array_equal(pred, base[0], equal_nan=True) and np.array_equal(err, base[1], equal_nan=True)
    assert info["n_rank_def"] == 0 and info["beta"].shape == (120, 0)
    assert {k: info[k] for k in base[2]} == base[2]
    for k in range(2):
        h.set_trend(k, np.ones((len(coords[k]), 1)))
    h.predict_local_universal(0, pc, np.ones((120, 1)), max_dist=400.0)
    again = h.predict_local(0, pc, max_dist=400.0)   # the simple call ignores the trend and is not disturbed by it
    assert np.array_equal(again[0], base[0], equal_nan=True) and np.array_equal(again[1], base[1], equal_nan=True)
    assert again[2] == base[2]


# ---- 5. determinism ------------------------------------------------------------------------------------------------
def test_determinism(native):
    p, coords, values = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    Fs = [design("linear", c, c) for c in coords]
    F0 = design("linear", coords[0], pc)
    res = {}
    for order in (1, 0):
        h = handle(native, p, coords, values, HAV, site_order=order)
        for k in range(2):
            h.set_trend(k, Fs[k])
        res[order] = [h.predict_local_universal(0, pc, F0, max_dist=md, want_beta=True) for md in (250.0, 400.0, 900.0)]
        if order == 1:
            for md, first in zip((250.0, 400.0, 900.0), res[1]):
                a = h.predict_local_universal(0, pc, F0, max_dist=md, want_beta=True)
                assert np.array_equal(a[0], first[0], equal_nan=True) and np.array_equal(a[1], first[1], equal_nan=True)
                assert np.array_equal(a[2]["beta"], first[2]["beta"], equal_nan=True)
            h.set_option("local_slab_mb", 3)   # several batches of the tiled class through one small slab
            for md, first in zip((400.0, 900.0), res[1][1:]):
                a = h.predict_local_universal(0, pc, F0, max_dist=md, want_beta=True)
                assert np.array_equal(a[0], first[0], equal_nan=True) and np.array_equal(a[1], first[1], equal_nan=True)
                assert np.array_equal(a[2]["beta"], first[2]["beta"], equal_nan=True)
        h.close()
    for a, b in zip(res[1], res[0]):
        assert {k: v for k, v in a[2].items() if k != "beta"} == {k: v for k, v in b[2].items() if k != "beta"}
        assert np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
        np.testing.assert_allclose(a[0], b[0], rtol=1e-9, atol=1e-11, equal_nan=True)
        np.testing.assert_allclose(a[1] ** 2, b[1] ** 2, rtol=1e-9, atol=1e-11, equal_nan=True)


# ---- 6. properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist", [250.0, 400.0, 900.0])
def test_constant_shift_and_variance(native, max_dist):
    p, coords, values = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    ones = [np.ones((len(c), 1)) for c in coords]
    f0 = np.ones((len(pc), 1))
    for i in (0, 1):
        h = handle(native, p, coords, values, HAV)
        simple = h.predict_local(i, pc, max_dist=max_dist)
        for k in range(2):
            h.set_trend(k, ones[k])
        a = h.predict_local_universal(i, pc, f0, max_dist=max_dist)
        h.close()
        h = handle(native, p, coords, [v + (5.0 if k == i else 0.0) for k, v in enumerate(values)], HAV)
        for k in range(2):
            h.set_trend(k, ones[k])
        b = h.predict_local_universal(i, pc, f0, max_dist=max_dist)
        fin = ~np.isnan(a[0])
        assert fin.sum() > 100 and np.array_equal(np.isnan(b[0]), ~fin)
        assert np.max(np.abs(b[0][fin] - a[0][fin] - 5.0)) < 1e-9
        assert np.array_equal(a[1], b[1], equal_nan=True)
        # an estimated mean never lowers the variance of the same neighbourhood
        assert np.all(a[1][fin] ** 2 >= simple[1][fin] ** 2 - 1e-12)
        h.close()


@pytest.mark.parametrize("n0,n1,max_dist", [(12, 10, 1e9), (40, 37, 1e9), (40, 37, 1200.0)])   # LDS, tiled, moving window
def test_unbiasedness_of_the_weights(native, n0, n1, max_dist):
    """the kriging weights, recovered by predicting unit data vectors, sum to 1 over process i and to 0 over the other"""
    p, coords, _ = make_data(8, BIV, HAV, n0=n0, n1=n1)
    pc = pred_sites(np.random.default_rng(2), HAV, 6)
    ones = [np.ones((n0, 1)), np.ones((n1, 1))]
    for i in (0, 1):
        W = np.zeros((len(pc), n0 + n1))
        for e in range(n0 + n1):
            u = np.zeros(n0 + n1)
            u[e] = 1.0
            h = handle(native, p, coords, [u[:n0], u[n0:]], HAV)   # a handle's data are fixed once laid out
            for k in range(2):
                h.set_trend(k, ones[k])
            W[:, e] = h.predict_local_universal(i, pc, np.ones((len(pc), 1)), max_dist=max_dist)[0]
            h.close()
        fin = ~np.isnan(W[:, 0])
        assert fin.sum() >= 3
        sums = [W[fin, :n0].sum(1), W[fin, n0:].sum(1)]
        assert np.max(np.abs(sums[i] - 1.0)) < 1e-10 and np.max(np.abs(sums[1 - i])) < 1e-10


# ---- 7. cross-validation rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,max_dist", [("constant", 300.0), ("linear", 700.0)])
def test_cross_validation_rule(native, kind, max_dist):
    """cv at data sites of process i, nugget 0: the co-located datum is withheld (without the rule pred would be the datum)"""
    data = make_data(3, BIV_NONUG, HAV)
    for i in (0, 1):
        pc = data[1][i][::9]
        pred, err, info, ref = run_case(native, BIV_NONUG, HAV, kind, i, max_dist, data=data, pc=pc, cv=True)
        fin = ~np.isnan(pred)
        assert np.min(np.abs(pred[fin] - data[2][i][::9][fin])) > 1e-6


# ---- 8. Predictor(trend=...) end to end ---------------------------------------------------------------------------------
def test_predictor_end_to_end():
    import pandas as pd
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    p, coords, values = make_data(3, BIV, HAV)
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    mf = fields.MultiField([fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])])
    pc = pred_sites(np.random.default_rng(17), HAV)
    df = pd.DataFrame(pc, columns=["lat", "lon"])
    ref = Reference(p, coords, values, HAV, [np.ones((700, 1)), np.ones((650, 1))])(pc, 0, 250.0, np.ones((120, 1)))
    P0 = point_prediction.Predictor(mod, mf)
    P = point_prediction.Predictor(mod, mf, trend="constant")
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        out = P(0, df, max_dist=250.0, postprocess=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out0 = P0(0, df, max_dist=250.0, postprocess=False)
    fr = out.to_dataframe().reset_index() if hasattr(out, "to_dataframe") else out.reset_index()
    fr0 = out0.to_dataframe().reset_index() if hasattr(out0, "to_dataframe") else out0.reset_index()
    assert list(fr.columns) == list(fr0.columns) and len(fr) == len(fr0)
    assert P.trend_coef.shape == (120, 2)
    assert set(P.info) >= {"n_empty", "n_not_pd", "n_rank_def", "k_max"}
    assert P.info["n_rank_def"] == int((ref["status"] == RANK_DEF).sum())
    said = any("Trend not estimable" in str(w.message) for w in wlist)
    assert said == (P.info["n_rank_def"] > 0)
    got = fr.set_index(["lat", "lon"]).loc[list(map(tuple, pc))]
    ok = ref["status"] == OK
    assert np.array_equal(np.isnan(got["pred"].values), ~ok)
    ok &= np.abs(ref["pred"] - ref["pred2"]) <= 0.1 * (RTOL * np.abs(ref["pred"]) + ATOL)
    assert ok.sum() > 100
    np.testing.assert_allclose(got["pred"].values[ok], ref["pred"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got["pred_err"].values[ok] ** 2, np.maximum(ref["var"][ok], 0), rtol=RTOL, atol=ATOL)
    # linear trend at 250 km: rank-deficient neighbourhoods exist, and the warning carries their number
    PL = point_prediction.Predictor(mod, mf, trend="linear")
    with pytest.warns(UserWarning, match="Trend not estimable .* larger max_dist or a smaller trend"):
        PL.predict_arrays(0, pc, max_dist=250.0)
    assert PL.info["n_rank_def"] > 0 and PL.trend_coef.shape == (120, 6)
    # cross_validation works through the cv rule, with the frame of the no-trend form
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cv = P.cross_validation(0, max_dist=400.0, postprocess=False)
        cv0 = P0.cross_validation(0, max_dist=400.0, postprocess=False)
    assert list(cv.columns) == list(cv0.columns) == ["d1", "d2", "data", "pred", "residual", "pred_err"] and len(cv) == len(cv0) == 700
    refcv = Reference(p, coords, values, HAV, [np.ones((700, 1)), np.ones((650, 1))])(coords[0][:40], 0, 400.0, np.ones((40, 1)), cv=True)
    got = cv.set_index(["d1", "d2"]).loc[list(map(tuple, coords[0][:40]))]
    okc = refcv["status"] == OK
    okc &= np.abs(refcv["pred"] - refcv["pred2"]) <= 0.1 * (RTOL * np.abs(refcv["pred"]) + ATOL)
    np.testing.assert_allclose(got["pred"].values[okc], refcv["pred"][okc], rtol=RTOL, atol=ATOL)
    for q in (P, P0, PL):
        q.close()
