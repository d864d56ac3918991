"""GPU tests of per-observation measurement-error variances in the local-neighbourhood predictor: include/cokrige.h
ck_set_noise with ck_predict_local / ck_predict_local_universal, in every size class.

A per-site numpy reference in this file: neighbours by the oracle's distance, the neighbours' rows and columns of the dense
Sigma_noise = orc.joint_cov + diag(s d) (the noise sits on the true diagonal by datum index), a dense Cholesky solve, the NaN
rules of the library (no neighbour: NaN, counted in n_empty; local Sigma not positive definite: NaN, counted in n_not_pd).
Tolerances are the local path's own (tests/test_gpu_local_universal.py): rtol 1e-8, atol 1e-10 on pred and pred_err^2.

Largest deviations seen on an MI355X over all cases of this file: |d pred| and |d pred_err^2| 6.2e-14 against the per-site chain;
the infinite radius against the joint noisy predictor 6.3e-15 relative in pred, 8.9e-16 in pred_err^2."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_NONUG = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.0, 0.0, -0.19]
RTOL, ATOL = 1e-8, 1e-10
SCALE = (1.5, 0.7)
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_data(seed, params, metric, n0=700, n1=650):
    """the generator of tests/test_gpu_local_universal.py, with d: log-uniform over two decades around 1e-2 sigma_k^2, about
    10 % exact zeros; the dense noisy Sigma is computed once"""
    key = (seed, tuple(params), metric, n0, n1)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        p = orc.Params.from_flat(params)
        m = n0 + n1
        if metric == HAV:
            pts = np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])
        else:
            pts = np.column_stack([rng.uniform(0, 10, m), rng.uniform(0, 10, m)])
        coords = [pts[:n0].copy(), pts[n0 // 2:n0 // 2 + n1].copy()]
        S = orc.joint_cov(p, coords, metric)
        z = np.linalg.cholesky(S + 1e-12 * np.eye(m)) @ rng.standard_normal(m)
        values = [z[:n0] + 0.3, z[n0:] + 0.3]
        d = []
        for k, n in enumerate((n0, n1)):
            x = 1e-2 * p.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, n)
            x[rng.random(n) < 0.1] = 0.0
            d.append(x)
        Sn = S + np.diag(np.concatenate([SCALE[0] * d[0], SCALE[1] * d[1]]))
        _cache[key] = (p, coords, values, d, Sn)
    return _cache[key]


def pred_sites(rng, metric, m=120):
    if metric == HAV:
        return np.column_stack([rng.uniform(24, 51, m), rng.uniform(-122, -68, m)])
    return np.column_stack([rng.uniform(-0.4, 10.4, m), rng.uniform(-0.4, 10.4, m)])


def handle(native, p, coords, values, metric, d=None, scale=SCALE):
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
        if d is not None:
            h.set_noise(k, d[k], scale[k])
    return h


def reference(p, coords, values, Sn, pc, i, metric, max_dist, cv=False, universal=False):
    """per site: (pred, var, k, status) with status 0 ok, 1 empty, 2 not positive definite"""
    n0 = len(coords[0])
    m = len(pc)
    z = np.concatenate(values)
    c00 = p.sigma[i] ** 2 + p.nugget[i]
    pred, var = np.full(m, np.nan), np.full(m, np.nan)
    kk, st = np.zeros(m, int), np.zeros(m, int)
    for s in range(m):
        dists = [orc.distance_matrix(pc[s], c, metric)[0] for c in coords]
        ix = [x <= max_dist for x in dists]
        if cv:
            ix[i] = (dists[i] > 0) & (dists[i] <= max_dist)
        idx = np.concatenate([np.flatnonzero(ix[0]), n0 + np.flatnonzero(ix[1])])
        kk[s] = len(idx)
        if len(idx) == 0:
            st[s] = 1
            continue
        c = np.hstack([orc.covariance(p, i, dists[a][ix[a]], use_nugget=True) if a == i else
                       orc.cross_covariance(p, i, a, dists[a][ix[a]]) for a in range(2)])
        try:
            L = np.linalg.cholesky(Sn[np.ix_(idx, idx)])
        except np.linalg.LinAlgError:
            st[s] = 2
            continue
        v, y = solve_triangular(L, c, lower=True), solve_triangular(L, z[idx], lower=True)
        pred[s], var[s] = v @ y, c00 - v @ v
        if universal:   # a constant per process; a process without neighbours loses its column (it must not be process i)
            nk = [int(ix[0].sum()), int(ix[1].sum())]
            if nk[i] == 0:
                st[s], pred[s], var[s] = 3, np.nan, np.nan
                continue
            cols = [a for a in range(2) if nk[a] > 0]
            X = np.zeros((len(idx), 2))
            X[:nk[0], 0], X[nk[0]:, 1] = 1.0, 1.0
            X = X[:, cols]
            x0 = np.array([1.0 if a == i else 0.0 for a in cols])
            U = solve_triangular(L, X, lower=True)
            A, b = U.T @ U, U.T @ y
            r = x0 - U.T @ v
            pred[s] += r @ np.linalg.solve(A, b)
            var[s] += r @ np.linalg.solve(A, r)
    return pred, var, kk, st


def compare(pred, err, info, ref, what):
    rp, rv, kk, st = ref
    assert np.array_equal(np.isnan(pred), st != 0) and np.array_equal(np.isnan(err), st != 0), what
    assert info["n_empty"] == int((st == 1).sum()) and info["n_not_pd"] == int((st == 2).sum()), what
    assert info["k_max"] == int(kk.max()), what
    ok = st == 0
    dp = np.max(np.abs(pred[ok] - rp[ok]), initial=0)
    dv = np.max(np.abs(err[ok] ** 2 - np.maximum(rv[ok], 0.0)), initial=0)
    print(f"{what}: sites {len(st)} finite {int(ok.sum())} k {int(kk.min())}..{int(kk.max())} max |d pred| {dp:.2e} max |d var| {dv:.2e}")
    np.testing.assert_allclose(pred[ok], rp[ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err[ok] ** 2, np.maximum(rv[ok], 0.0), rtol=RTOL, atol=ATOL)


def run(native, max_dist, i, cv=False, options=(), universal=False, pc=None, data=None):
    p, coords, values, d, Sn = data if data is not None else make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV) if pc is None else pc
    h = handle(native, p, coords, values, HAV, d)
    for name, val in options:
        h.set_option(name, val)
    if universal:
        for k in range(2):
            h.set_trend(k, np.ones((len(coords[k]), 1)))
        pred, err, info = h.predict_local_universal(i, pc, np.ones((len(pc), 1)), max_dist=max_dist, cv=cv)
        assert info["n_rank_def"] == 0
    else:
        pred, err, info = h.predict_local(i, pc, max_dist=max_dist, cv=cv)
    # without the noise the same call differs: the vector reaches this size class
    h0 = handle(native, p, coords, values, HAV)
    for name, val in options:
        h0.set_option(name, val)
    if universal:
        for k in range(2):
            h0.set_trend(k, np.ones((len(coords[k]), 1)))
        q = h0.predict_local_universal(i, pc, np.ones((len(pc), 1)), max_dist=max_dist, cv=cv)[0]
    else:
        q = h0.predict_local(i, pc, max_dist=max_dist, cv=cv)[0]
    fin = ~np.isnan(pred) & ~np.isnan(q)
    assert np.max(np.abs(pred[fin] - q[fin])) > 1e-6
    h.close()
    h0.close()
    ref = reference(p, coords, values, Sn, pc, i, HAV, max_dist, cv=cv, universal=universal)
    compare(pred, err, info, ref, f"{max_dist} km i={i} cv={cv} {options} universal={universal}")
    return ref


# ---- 1. the three radii -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist", [250.0, 400.0, 900.0])   # LDS class | both classes in one call | tiled class
@pytest.mark.parametrize("i", [0, 1])
def test_parity_haversine(native, i, max_dist):
    kk = run(native, max_dist, i)[2]
    if max_dist == 250.0:
        assert kk.max() <= 64
    if max_dist == 400.0:
        assert kk.min() <= 64 < kk.max()
    if max_dist == 900.0:
        assert kk.min() > 64


# ---- 2. / 3. the other routes -----------------------------------------------------------------------------------------------
def test_everything_on_the_tiled_path(native):
    run(native, 400.0, 0, options=(("local_tile_min", 0),))


def test_slab_kernel_route(native):
    """local_tile_min far above every neighbourhood: k > 64 goes through k_local_solve_big"""
    kk = run(native, 400.0, 1, options=(("local_tile_min", 1 << 20),))[2]
    assert kk.max() > 64


# ---- 4. cv ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist", [250.0, 900.0])
def test_cv_withholds_as_before(native, max_dist):
    p, coords, values, d, Sn = make_data(3, BIV, HAV)
    run(native, max_dist, 0, cv=True, pc=coords[0][:60].copy())


# ---- 5. universal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist", [250.0, 400.0, 900.0])
def test_universal_constant(native, max_dist):
    p, coords, values, d, Sn = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    # keep the sites that see their own process (rule 3 of the universal form is not what this file is about)
    keep = np.array([(orc.distance_matrix(s, coords[0], HAV)[0] <= max_dist).any() for s in pc])
    run(native, max_dist, 0, universal=True, pc=pc[keep])


# ---- 6. padding sizes -------------------------------------------------------------------------------------------------------
def test_padding_sizes(native):
    p, coords, values, d, Sn = make_data(41, BIV, HAV, n0=120, n1=110)
    pc = pred_sites(np.random.default_rng(5), HAV, 9)
    for n0, n1 in [(31, 31), (32, 31), (32, 32), (33, 32), (62, 62), (63, 62), (94, 94), (95, 94)]:
        ix = np.concatenate([np.arange(n0), 120 + np.arange(n1)])
        data = (p, [coords[0][:n0], coords[1][:n1]], [values[0][:n0], values[1][:n1]], [d[0][:n0], d[1][:n1]], Sn[np.ix_(ix, ix)])
        for i in (0, 1):
            for universal in (False, True):
                kk = run(native, 1e9, i, pc=pc, data=data, universal=universal)[2]
                assert kk.max() == n0 + n1


# ---- 7. infinite radius = the joint noisy predictor -------------------------------------------------------------------------
def test_infinite_radius_matches_joint(native):
    p, coords, values, d, Sn = make_data(3, BIV, HAV)
    pc = pred_sites(np.random.default_rng(17), HAV)
    h = handle(native, p, coords, values, HAV, d)
    h.assemble_joint()
    assert h.factor() == 0
    for i in (0, 1):
        jp, je = h.predict(i, pc)
        pred, err, info = h.predict_local(i, pc, max_dist=1e9)
        assert info["k_max"] == 1350 and info["n_empty"] == info["n_not_pd"] == 0
        print(f"i={i}: pred {np.max(np.abs(pred - jp)) / np.max(np.abs(jp)):.2e} var {np.max(np.abs(err ** 2 - je ** 2)):.2e}")
        assert np.max(np.abs(pred - jp)) / np.max(np.abs(jp)) < 1e-8
        assert np.max(np.abs(err ** 2 - je ** 2)) < 1e-9
    h.close()


# ---- 8. co-located copies with zero nugget ----------------------------------------------------------------------------------
def test_not_pd_counter_drops_to_zero(native):
    """data of process 0 at identical coordinates with nugget 0 (five pairs): a neighbourhood that holds a pair is singular
    -- the copy's pivot is pure rounding, of either sign, so many different neighbourhoods are asked; with measurement error on
    the copies every one is positive definite"""
    rng = np.random.default_rng(23)
    p = orc.Params.from_flat(BIV_NONUG)
    pts = np.column_stack([rng.uniform(30, 40, 80), rng.uniform(-100, -85, 80)])
    c0 = np.vstack([pts[:40], pts[[3, 11, 19, 27, 35]]])
    coords = [c0, pts[40:]]
    values = [rng.standard_normal(45), rng.standard_normal(40)]
    pc = np.column_stack([rng.uniform(31, 39, 40), rng.uniform(-99, -86, 40)])
    h = handle(native, p, coords, values, HAV)
    pred, err, info = h.predict_local(0, pc, max_dist=700.0)
    assert info["n_not_pd"] > 0
    d = [np.zeros(45), np.zeros(40)]
    d[0][40:] = 0.02
    for k in range(2):
        h.set_noise(k, d[k], 1.0)
    pred, err, info = h.predict_local(0, pc, max_dist=700.0)
    assert info["n_not_pd"] == 0 and not np.isnan(pred).any()
    Sn = orc.joint_cov(p, coords, HAV) + np.diag(np.concatenate(d))
    compare(pred, err, info, reference(p, coords, values, Sn, pc, 0, HAV, 700.0), "co-located copies")
    h.close()


def test_point_predictor_end_to_end(native):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    p, coords, values, d, Sn = make_data(3, BIV, HAV)
    mf = fields.MultiField([fields.Field(coords[k], values[k], variance_estimate=d[k]) for k in range(2)])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(BIV)
    P = point_prediction.Predictor(mod, mf, measurement_error=True, noise_scale=SCALE)
    pc = pred_sites(np.random.default_rng(17), HAV)[:40]
    pred, err = P.predict_arrays(0, pc, max_dist=400.0)
    rp, rv, kk, st = reference(p, coords, values, Sn, pc, 0, HAV, 400.0)
    assert (st == 0).all()
    np.testing.assert_allclose(pred, rp, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err ** 2, np.maximum(rv, 0.0), rtol=RTOL, atol=ATOL)
    P.close()
