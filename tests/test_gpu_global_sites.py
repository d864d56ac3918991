"""GPU tests on whole-globe sites (tests/global_sites.py): the haversine paths that only start working beyond the distances of
the continental fixtures.

1. Sigma entry by entry where half of the pairs lie beyond the tables' upper end (q >= 2, 10 007.5 km): the table kernels defer
   them to the exact pass (K1), proven by the fallback count;
2. joint prediction (K2 and the Schur complement of verify_model with far pairs), the likelihood's exact-formula kernels;
3. the local predictor at reaches of 3 000 km .. everything (culling on, `2 sin` near its top, the "no culling" switch), its
   LDS / slab / tiled systems with entries beyond the table, cross-validation across the antimeridian, caps, a trend; Vecchia;
4. the variogram beyond half the circumference;
5. exact antipodes and lon -+ 360 copies;
6. more deferred pairs than the worklist holds (2 ** 22): the second, exact attempt of the assembly in K1 and K2;
7. the Euclidean twin: prediction sites beyond two box diagonals.

References and bounds are the neighbouring files': the oracle (numpy / scipy / sklearn), 5e-13 relative on covariance entries
(test_cov_dense_blocks), the table gate's measure between the table and the exact handle
(test_table_path_across_the_parameter_box), pred 1e-8 relative and variance 1e-9 absolute on the joint path, rtol 1e-8 / atol
1e-10 on the local one.  tests/test_global_sites_host.py pins the inputs' guarantees without a GPU.

Against orc.joint_cov the bound is entry-wise rtol 5e-13 plus the move of the oracle's own entry under the rounding of the
haversine formula (gs.joint_cov_tolerance): near the antipode asin(sqrt(r)) is at its branch point, and the oracle itself moves
by 1.55e-7 relative (exact antipodes, len_scale 2000) and 2.6e-12 (GLOBE, len_scale 100) when its inputs are nudged by one ulp.

Seen on an MI355X.  Sigma: the exact handle against the oracle 3.4e-13 (A), 1.0e-13 (long), 1.8e-13 (closed), 3.4e-12 (short: 132
entries beyond plain rtol 5e-13, the largest a quarter of its bound); the table handle against the exact one 4.2e-13 (A); 154 893
deferred entries in the caller's order and 152 907 in the Hilbert order for 96 276 lower-triangle pairs strictly outside the tables.
Joint prediction: pred 6.9e-14 relative, variance 1.2e-14; K2 deferred 21 677 (m = 70) and 93 059 (m = 300) pairs.  Likelihood:
values 1.6e-15 relative, gradient measure 2.0e-10.  Local predictor: pred 7.8e-13 relative, variance 6.9e-15 over every reach,
route and site order; Vecchia gradient measure 2.2e-10, scores 3.8e-10.  Variogram: counts, edges and centres identical, means
1.1e-14.  Antipodes: every entry finite, antipodal entries 7.6e-5 as the oracle's, 12 entries beyond plain rtol 5e-13 (up to
1.55e-7, half of their bound); no lon -+ 360 copy at exactly 0 and none carries a nugget.  Overflow: K1 counted 4 437 616 deferred
entries and K2 4 300 850 (capacity 4 194 304), both bit-equal to the exact_cov handle; Euclid: 21 600 deferred pairs per call."""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc
from tests import dense_chains as dc
from tests import global_sites as gs
from tests import vecchia_grad_ref as vgr
from tests import vecchia_ref as vr

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10                      # the local path's own (tests/test_gpu_local.py)
MAX_DISTS = [3000.0, 9000.0, 12000.0, 19500.0, 1e9]
TILE_MIN = [None, 0, 10 ** 6]                 # default classes | everything tiled | LDS + slab kernels
LOCAL_SET = "long"                            # len_scale 2 000 km: an entry beyond the table is exp(-5) of the variance and
                                              # a wrong one moves a local prediction far beyond rtol 1e-8
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_handle(native, params, coords, values, metric=HAV, noise=None, scales=(1.0, 1.0), **options):
    p = orc.Params.from_flat(params)
    h = native.Handle(0)
    for name, value in options.items():
        h.set_option(name, value)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
    if noise is not None:
        for k in range(2):
            h.set_noise(k, noise[k], scales[k])
    return h, p


def globe_sigma(name):
    if ("S", name) not in _cache:
        _cache["S", name] = orc.joint_cov(orc.Params.from_flat(gs.GLOBE_PARAMS[name]), gs.GLOBE["coords"], HAV)
    return _cache["S", name]


def globe_tolerance(name):
    if ("tol", name) not in _cache:
        _cache["tol", name] = gs.joint_cov_tolerance(orc.Params.from_flat(gs.GLOBE_PARAMS[name]), gs.GLOBE["coords"], globe_sigma(name))
    return _cache["tol", name]


def internal_index(h, coords):
    n0 = len(coords[0])
    return np.concatenate([h.debug_site_order(0, n0), n0 + h.debug_site_order(1, len(coords[1]))])


def max_rel(a, b):
    """largest |a - b| / |b| over the entries with b != 0 (inf where a != 0 = b)"""
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    nz = b != 0
    worst = np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]), initial=0.0)
    return np.inf if np.any(a[~nz] != 0) else worst


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def tables_of(h):
    return [h.table_info(b) for b in range(3)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. Sigma entries (K1)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("name", list(gs.GLOBE_PARAMS))
def test_sigma_entries_beyond_the_table(native, name, site_order):
    """The table handle against the exact one at the table gate's measure, the exact one against the oracle at 5e-13, and the
    fallback count: at least every lower-triangle pair strictly outside its block's table was deferred -- more than 30 % of
    all pairs, which only the upper end can supply (the lower end holds the diagonal and the co-located sites: < 1 %)."""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    N = gs.N0 + gs.N1
    pv = gs.GLOBE_PARAMS[name]
    h, p = make_handle(native, pv, coords, values, site_order=site_order)
    h.table_fallbacks()
    h.assemble_joint()
    fb = h.table_fallbacks()
    tabs = tables_of(h)
    low = h.debug_get_lower(N)
    hx, _ = make_handle(native, pv, coords, values, site_order=site_order, exact_cov=1)
    hx.assemble_joint()
    assert hx.table_fallbacks() == 0
    lowx = hx.debug_get_lower(N)
    idx = internal_index(h, coords)
    assert np.array_equal(idx, internal_index(hx, coords))
    if site_order == 0:
        assert np.array_equal(idx, np.arange(N))
    S = np.tril(globe_sigma(name)[np.ix_(idx, idx)])
    scale = np.max(np.diag(lowx))
    enabled = all(t["enabled"] for t in tabs)
    n_out = gs.count_outside_sigma(coords, tabs) if enabled else 0
    print(f"{name} site_order {site_order}: tables {'on' if enabled else 'gated out'}, q_hi {[t['q_hi'] for t in tabs]}, "
          f"fallbacks {fb}, pairs strictly outside {n_out} of {N * (N + 1) // 2}; table vs exact max rel "
          f"{max_rel(low, lowx):.2e}, exact vs oracle max rel {max_rel(lowx, S):.2e}, table vs oracle max rel {max_rel(low, S):.2e}")
    assert np.all(np.isfinite(low)) and np.all(np.isfinite(lowx))
    if enabled:
        assert max(t["max_rel_err"] for t in tabs) < 2e-13
        assert all(t["q_hi"] == 2.0 for t in tabs)
        np.testing.assert_allclose(low, lowx, rtol=5e-13, atol=5e-19 * scale)
        assert n_out > 0.3 * N * (N + 1) / 2
        assert fb >= n_out
    else:   # a gated-out table: the whole assembly went through the exact kernel
        assert np.array_equal(low, lowx) and fb == 0
    # the oracle's entry itself moves by 2.6e-12 relative (`short`) under a 1-ulp nudge of its inputs, near the antipode: the
    # bound is rtol 5e-13 plus that move, entry by entry (gs.joint_cov_tolerance; floors in tests/test_global_sites_host.py)
    tol = np.tril(globe_tolerance(name)[np.ix_(idx, idx)])
    worst = np.max(np.abs(lowx - S) / np.maximum(tol, 1e-300))
    print(f"{name} site_order {site_order}: exact vs oracle, largest |difference| / bound {worst:.3f}; entries beyond plain rtol "
          f"5e-13: {np.count_nonzero(np.abs(lowx - S) > 5e-13 * np.abs(S))}")
    assert np.all(np.abs(lowx - S) <= tol)
    h.close()
    hx.close()


def test_tables_are_in_use_on_the_globe(native):
    """the count above proves something only where the tables passed their gate: they do for the three long-range sets"""
    for name in ("A", "long", "closed"):
        h, _ = make_handle(native, gs.GLOBE_PARAMS[name], gs.GLOBE["coords"], gs.GLOBE["values"])
        h.assemble_joint()
        assert all(t["enabled"] for t in tables_of(h)), name
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. joint prediction, the Schur complement, the likelihood
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [70, 300])          # 300: the library sorts the prediction sites along its Hilbert curve
@pytest.mark.parametrize("name", ["A", "long", "closed"])
def test_joint_prediction_on_the_globe(native, name, m):
    """factor + predict and factor_predict against the oracle; K2 defers at least every (site, datum) pair strictly outside the
    table; verify_model (the Schur complement with far pairs) gives the verdict of the exact handle.  The verdict is taken for
    process 1: for process 0 a prediction site sits on a datum, where the Schur complement is singular up to rounding."""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pv = gs.GLOBE_PARAMS[name]
    pc = gs.globe_pred_sites(np.random.default_rng(1000 + m), m)
    h, p = make_handle(native, pv, coords, values)
    h.assemble_joint()
    assert h.factor() == 0
    hx, _ = make_handle(native, pv, coords, values, exact_cov=1)
    hx.assemble_joint()
    assert hx.factor() == 0
    tabs = tables_of(h)
    for i in (0, 1):
        rp, re = orc.joint_predict(p, coords, values, pc, i, HAV)
        h.table_fallbacks()
        pred, err = h.predict(i, pc)
        fb = h.table_fallbacks()
        n_out = gs.count_outside_aux(coords, pc, i, tabs)
        px, ex = hx.predict(i, pc)
        h2, _ = make_handle(native, pv, coords, values)
        h2.assemble_joint()
        info, p2, e2 = h2.factor_predict(i, pc)
        assert info == 0
        for what, (a, b) in (("predict", (pred, err)), ("factor_predict", (p2, e2)), ("exact_cov", (px, ex))):
            dp, dv = rel(a, rp), np.max(np.abs(b ** 2 - re ** 2))
            print(f"{name} m {m} i {i} {what}: pred rel {dp:.2e}, |d var| {dv:.2e}; fallbacks {fb}, strictly outside {n_out}")
            assert dp < 1e-8 and dv < 1e-9, (what, i)
        assert fb >= n_out > 0.3 * m * (gs.N0 + gs.N1)
        if i == 1:
            v, vx, v2 = h.verify_model(), hx.verify_model(), h2.verify_model()
            S = globe_sigma(name)
            c0 = orc.pred_cross_cov(p, coords, pc, 1, HAV)
            sch = orc.pred_cov(p, pc, 1, HAV) - c0.T @ np.linalg.solve(S, c0)
            print(f"{name} m {m}: verify_model {v} / exact {vx} / factor_predict {v2}; smallest eigenvalue of the oracle's Schur "
                  f"complement {np.linalg.eigvalsh(sch).min():.3e}")
            assert np.linalg.eigvalsh(sch).min() > 1e-6
            assert v == vx == v2 == 0
        h2.close()
    h.close()
    hx.close()


def test_joint_prediction_with_noise_on_the_globe(native):
    """measurement-error variances on both processes against the dense noisy Sigma (dense_chains.dense_sigma)"""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pv = gs.GLOBE_PARAMS["long"]
    rng = np.random.default_rng(77)
    d = [1e-2 * 10.0 ** rng.uniform(-1, 1, gs.N0), 1e-2 * 10.0 ** rng.uniform(-1, 1, gs.N1)]
    scales = (1.5, 0.7)
    Sn = dc.dense_sigma(pv, coords, HAV, noise=d, scales=scales)
    cf = cho_factor(Sn, lower=True)
    z = np.concatenate(values)
    pc = gs.globe_pred_sites(np.random.default_rng(1070), 70)
    h, p = make_handle(native, pv, coords, values, noise=d, scales=scales)
    h.assemble_joint()
    assert h.factor() == 0
    for i in (0, 1):
        c0 = orc.pred_cross_cov(p, coords, pc, i, HAV)
        w = cho_solve(cf, c0)
        rp, rvar = w.T @ z, p.sigma[i] ** 2 + p.nugget[i] - np.einsum("ij,ij->j", c0, w)
        pred, err = h.predict(i, pc)
        dp, dv = rel(pred, rp), np.max(np.abs(err ** 2 - np.maximum(rvar, 0.0)))
        print(f"noise i {i}: pred rel {dp:.2e}, |d var| {dv:.2e}")
        assert dp < 1e-8 and dv < 1e-9
    h.close()


@pytest.mark.parametrize("name", ["short", "long"])
def test_likelihood_on_the_globe(native, name):
    """ck_loglik's exact-formula kernels at lags up to 20 000 km (scaled lags up to 530 under `short`) against the dense chain"""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pv = gs.GLOBE_PARAMS[name]
    S = globe_sigma(name)
    ref = dc.dense_ll(pv, coords, values, HAV, S=S)
    gref = dc.dense_ll_grad(pv, coords, values, HAV, S=S)
    h, _ = make_handle(native, pv, coords, values)
    h.assemble_joint()
    info, out3, g = h.loglik(True)
    assert info == 0
    eg = np.abs(g - gref) / np.maximum(np.abs(gref), 1.0)
    print(f"{name}: l, log|Sigma|, quad rel {[abs(a - b) / abs(b) for a, b in zip(out3, ref)]}, gradient measure {eg.max():.2e}")
    for a, b in zip(out3, ref):
        assert abs(a - b) <= 1e-8 * abs(b)
    assert eg.max() < 1e-6, (g, gref)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the local predictor and Vecchia
# ---------------------------------------------------------------------------------------------------------------------
def local_sites():
    if "local_pc" not in _cache:
        _cache["local_pc"] = gs.globe_pred_sites(np.random.default_rng(100), 40)
    return _cache["local_pc"]


def local_reference(max_dist):
    """oracle.local_predict and numpy's neighbour counts at local_sites(), once per reach"""
    key = ("local", max_dist)
    if key not in _cache:
        coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
        pc = local_sites()
        p = orc.Params.from_flat(gs.GLOBE_PARAMS[LOCAL_SET])
        rp, re = orc.local_predict(p, coords, values, pc, 0, HAV, max_dist)[:2]
        cnt = np.column_stack([np.count_nonzero(orc.haversine_km(pc, c) <= max_dist, axis=1) for c in coords])
        assert np.all(np.isfinite(rp)) and np.all(np.isfinite(re)) and cnt.sum(axis=1).min() > 0
        _cache[key] = (rp, re, cnt)
    return _cache[key]


@pytest.mark.parametrize("tile_min", TILE_MIN)
@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_local_prediction_at_every_reach(native, max_dist, tile_min):
    """3 000 km: culling on | 9 000: the reach holds pairs beyond the table | 12 000: 2 sin(max_dist / 2R) near its top |
    19 500: past the `half >= 1.5` switch to no culling | 1e9: everything.  Both site orders (chunks of a Hilbert order over
    a 360 x 180 degree box; the caller's order, whose chunk balls are centred near the origin of chord space)."""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pc = local_sites()
    rp, re, cnt = local_reference(max_dist)
    opts = {} if tile_min is None else {"local_tile_min": tile_min}
    for site_order in (0, 1):
        h, _ = make_handle(native, gs.GLOBE_PARAMS[LOCAL_SET], coords, values, site_order=site_order, **opts)
        count, rcut = h.local_neighbours(0, pc, max_dist)
        assert np.array_equal(count, cnt), (site_order, np.flatnonzero((count != cnt).any(axis=1)))
        pred, err, info = h.predict_local(0, pc, max_dist=max_dist)
        print(f"max_dist {max_dist:g} tile_min {tile_min} site_order {site_order}: k {cnt.sum(axis=1).min()} .. "
              f"{cnt.sum(axis=1).max()}, max rel pred {np.max(np.abs(pred - rp) / np.maximum(np.abs(rp), ATOL / RTOL)):.2e}, "
              f"max |d var| {np.max(np.abs(err ** 2 - re ** 2)):.2e}")
        assert info["n_empty"] == 0 and info["n_not_pd"] == 0 and info["k_max"] == cnt.sum(axis=1).max(), info
        np.testing.assert_allclose(pred, rp, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(err ** 2, re ** 2, rtol=RTOL, atol=ATOL)
        h.close()
    if max_dist == 1e9:
        assert cnt.sum(axis=1).min() == gs.N0 + gs.N1
    if max_dist == 3000.0:
        assert cnt.sum(axis=1).max() <= 64               # the LDS class


@pytest.mark.parametrize("cv", [False, True])
def test_radius_search_culling_on_the_globe(native, cv):
    """GLOBE has two 256-site chunks per process, which the bounding-ball test can hardly ever skip.  Here 3 000 + 2 600 sites
    make 12 + 11 chunks: compact caps of the sphere in the Hilbert order (computed over a 360 x 180 degree box), balls centred
    near the origin of chord space in the caller's order.  The neighbour counts of both orders equal numpy's at every reach from
    1 500 km (most chunks skipped) through 2 sin(max_dist / 2R) near its top to the `no culling` switch, with the poles, the
    antimeridian and (cv) the d > 0 rule among the points."""
    rng = np.random.default_rng(4)
    coords = [gs.sphere_sites(rng, 3000), gs.sphere_sites(rng, 2600)]
    coords[0][:len(gs.SPECIAL_0)] = gs.SPECIAL_0
    coords[1][:len(gs.SPECIAL_1)] = gs.SPECIAL_1
    values = [np.zeros(3000), np.zeros(2600)]
    pc = np.vstack([coords[0][:40], gs.globe_pred_sites(rng, 40)]) if cv else gs.globe_pred_sites(rng, 80)
    D = [orc.haversine_km(pc, c) for c in coords]
    reaches = [1500.0, 3000.0, 9000.0, 12000.0, 19500.0, 20015.0, 1e9]
    for site_order in (0, 1):
        h, _ = make_handle(native, gs.GLOBE_PARAMS[LOCAL_SET], coords, values, site_order=site_order)
        for md in reaches:
            cnt = np.column_stack([np.count_nonzero(((D[0] > 0) if cv else True) & (D[0] <= md), axis=1),
                                   np.count_nonzero(D[1] <= md, axis=1)])
            assert min(np.min(np.abs(d - md)) for d in D) > 1e-9 * md          # no distance within rounding of the reach
            count, _ = h.local_neighbours(0, pc, md, cv=cv)
            assert np.array_equal(count, cnt), (site_order, md, np.flatnonzero((count != cnt).any(axis=1)))
        h.close()
    print(f"culling cv {cv}: neighbour counts of {len(pc)} points identical to numpy's at {len(reaches)} reaches in both site orders")


@pytest.mark.parametrize("max_dist", [3000.0, 12000.0])
def test_local_cross_validation_across_the_antimeridian(native, max_dist):
    """cv at the first 60 data sites of process 0: (10, 180) and (10, -180) are each other's neighbour at 1.5e-12 km and neither
    is its own; the poles and (0, 180) are among them"""
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pc = coords[0][:60]
    assert tuple(pc[2]) == (10.0, 180.0) and tuple(pc[3]) == (10.0, -180.0)
    p = orc.Params.from_flat(gs.GLOBE_PARAMS[LOCAL_SET])
    rp, re = orc.local_predict(p, coords, values, pc, 0, HAV, max_dist, True)[:2]
    D = [orc.haversine_km(pc, c) for c in coords]
    cnt = np.column_stack([np.count_nonzero((D[0] > 0) & (D[0] <= max_dist), axis=1), np.count_nonzero(D[1] <= max_dist, axis=1)])
    assert 0 < D[0][2, 3] < 1e-9 and D[0][2, 2] == 0 and D[0][3, 3] == 0
    for site_order in (0, 1):
        h, _ = make_handle(native, gs.GLOBE_PARAMS[LOCAL_SET], coords, values, site_order=site_order)
        count, _ = h.local_neighbours(0, pc, max_dist, cv=True)
        assert np.array_equal(count, cnt), np.flatnonzero((count != cnt).any(axis=1))
        pred, err, info = h.predict_local(0, pc, max_dist=max_dist, cv=True)
        print(f"cv max_dist {max_dist:g} site_order {site_order}: max |d pred| {np.max(np.abs(pred - rp)):.2e}, max |d var| "
              f"{np.max(np.abs(err ** 2 - re ** 2)):.2e}")
        assert info["n_empty"] == 0 and info["n_not_pd"] == 0
        np.testing.assert_allclose(pred, rp, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(err ** 2, re ** 2, rtol=RTOL, atol=ATOL)
        h.close()


@pytest.mark.parametrize("tile_min", TILE_MIN)
def test_local_capped_neighbourhoods_on_the_globe(native, tile_min):
    """caps (40, 25) inside a reach of 12 000 km: numpy's selection (tests/test_gpu_local_nmax.py: select), the oracle on it"""
    from tests.test_gpu_local_nmax import select
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pc = local_sites()
    caps = (40, 25)
    if "capped" not in _cache:
        sel = [select(orc.haversine_km(pc, coords[q]), 12000.0, caps[q], False) for q in range(2)]
        assert min(s[3].min() for s in sel) > 1e-9            # every cut lies in a gap of the distances
        p = orc.Params.from_flat(gs.GLOBE_PARAMS[LOCAL_SET])
        ref = np.array([[x[0] for x in orc.local_predict(p, [coords[q][sel[q][0][s]] for q in range(2)],
                                                         [values[q][sel[q][0][s]] for q in range(2)], pc[s:s + 1], 0, HAV, np.inf)[:2]]
                        for s in range(len(pc))])
        _cache["capped"] = (sel, ref)
    sel, ref = _cache["capped"]
    h, _ = make_handle(native, gs.GLOBE_PARAMS[LOCAL_SET], coords, values, **({} if tile_min is None else {"local_tile_min": tile_min}))
    h.set_local_neighbours(*caps)
    count, rcut = h.local_neighbours(0, pc, 12000.0)
    assert np.array_equal(count, np.column_stack([s[0].sum(axis=1) for s in sel]))
    # the cut distance to the last bits only: the device's sin / cos are not libm's (the sets agree: every cut lies in a gap)
    np.testing.assert_allclose(rcut, np.column_stack([s[1] for s in sel]), rtol=1e-12, atol=0)
    pred, err, info = h.predict_local(0, pc, max_dist=12000.0)
    print(f"capped tile_min {tile_min}: k_max {info['k_max']}, max |d pred| {np.max(np.abs(pred - ref[:, 0])):.2e}, max |d var| "
          f"{np.max(np.abs(err ** 2 - ref[:, 1] ** 2)):.2e}")
    assert info["k_max"] == 65 and info["n_empty"] == 0 and info["n_not_pd"] == 0
    np.testing.assert_allclose(pred, ref[:, 0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err ** 2, ref[:, 1] ** 2, rtol=RTOL, atol=ATOL)
    h.close()


def test_local_universal_on_the_globe(native):
    """a constant trend per process in a reach of 12 000 km against tests/test_gpu_local_universal.py: Reference"""
    from tests.test_gpu_local_universal import Reference, compare
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pc = local_sites()[:24]
    values = [v + 0.3 for v in values]
    Fs = [np.ones((len(c), 1)) for c in coords]
    F0 = np.ones((len(pc), 1))
    h, p = make_handle(native, gs.GLOBE_PARAMS[LOCAL_SET], coords, values)
    for k in range(2):
        h.set_trend(k, Fs[k])
    pred, err, info = h.predict_local_universal(0, pc, F0, max_dist=12000.0, want_beta=True)
    ref = Reference(p, coords, values, HAV, Fs)(pc, 0, 12000.0, F0)
    compare(pred, err, info, ref, beta=info["beta"])
    h.close()


def test_vecchia_on_the_globe(native):
    """value, terms and the analytic gradient with conditioning sets of up to 16 + 16 data inside 12 000 km, in a random order,
    against tests/vecchia_ref.py and tests/vecchia_grad_ref.py at those files' bounds"""
    from tests.test_gpu_vecchia import check_against
    from tests.test_gpu_vecchia_grad import check_scores
    coords, values = gs.GLOBE["coords"], gs.GLOBE["values"]
    pv = gs.GLOBE_PARAMS[LOCAL_SET]
    # the two spellings (10, 180) / (10, -180) of process 0 are equidistant from every third site up to rounding: under this
    # order no cut falls between them (asserted: numpy and the device agree on every set)
    ranks = np.random.default_rng(3).permutation(gs.N0 + gs.N1).astype(np.int64)
    ref = vr.vecchia_reference(pv, coords, values, HAV, ranks, 12000.0, (16, 16))
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0 and ref["k_max"] == 32 and ref["n_capped"] > 500
    want = vgr.vecchia_grad_reference(pv, coords, values, HAV, ref)
    h, _ = make_handle(native, pv, coords, values)
    h.set_local_neighbours(16, 16)
    out3, info, st = h.loglik_vecchia(ranks, 12000.0, terms=True)
    check_against(ref, out3, info, st, "globe")
    g3, grad, ginfo, gst = h.loglik_vecchia_grad(ranks, 12000.0, scores=True)
    assert ginfo == 0 and np.array_equal(g3, out3)
    check_scores(grad, gst["score"], want, np.arange(11), "globe")
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the variogram beyond half the circumference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("max_dist", [3000.0, 12000.0, 20015.0, 1e9])
def test_variogram_on_the_globe(native, max_dist, same):
    from sif_xco2_cokriging_amd.variogram import variogram_arrays
    ci, vi = gs.vario_sites(700, 5)
    cj, vj = gs.vario_sites(650, 6)
    ref = orc.variogram(ci, vi, ci if same else cj, vi if same else vj, same, HAV, max_dist, 20)
    h = native.Handle(0)
    h.set_metric(HAV)
    try:
        with np.errstate(all="ignore"):
            got = variogram_arrays(h, ci, vi, None if same else cj, None if same else vj, same, max_dist, 20)
    finally:
        h.close()
    has = ref[3] > 0
    print(f"variogram max_dist {max_dist:g} same {same}: {int(ref[3].sum())} pairs, last edge {ref[1][-1]:.1f} km, max rel mean "
          f"{np.max(np.abs(got[2][has] - ref[2][has]) / np.abs(ref[2][has])):.2e}")
    assert np.array_equal(got[3], ref[3])
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    np.testing.assert_allclose(got[2][has], ref[2][has], rtol=1e-10, atol=1e-13)
    if max_dist >= 20015.0:
        assert ref[1][-1] > np.pi * orc.EARTH_RADIUS


# ---------------------------------------------------------------------------------------------------------------------
# 5. antipodes and periodic duplicates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("site_order", [0, 1])
def test_antipodes_and_periodic_copies(native, site_order, exact):
    """32 sites, their exact antipodes and their lon -+ 360 copies: every entry finite and the oracle's; an antipodal entry is
    exp(-10) of the variance, not 0; a copy is a different site (no nugget) unless the oracle's distance is exactly 0"""
    ap = gs.antipodes()
    coords = ap["coords"]
    n = len(ap["base"])
    pv = gs.GLOBE_PARAMS["long"]
    p = orc.Params.from_flat(pv)
    values = [np.zeros(2 * n), np.zeros(2 * n)]
    h, _ = make_handle(native, pv, coords, values, site_order=site_order, exact_cov=exact)
    h.assemble_joint()
    idx = internal_index(h, coords)
    inv = np.argsort(idx)
    low = h.debug_get_lower(4 * n)
    full = np.tril(low) + np.tril(low, -1).T
    got = full[np.ix_(inv, inv)]                              # the caller's stacked order
    S = orc.joint_cov(p, coords, HAV)
    a = np.arange(n)
    anti_got, anti_ref = got[n + a, a], S[n + a, a]           # process 0: site a against its antipode n + a
    copy_got = got[2 * n + a, 3 * n + a]                      # process 1: copy a against site a
    d_copy = orc.haversine_km(ap["copy"], ap["base"]).diagonal()
    print(f"antipodes site_order {site_order} exact {exact}: max rel to the oracle {max_rel(np.tril(got), np.tril(S)):.2e}, antipodal "
          f"entries {anti_got.min():.3e} .. {anti_got.max():.3e} (oracle {anti_ref.min():.3e} .. {anti_ref.max():.3e}), "
          f"copies at exactly 0: {np.count_nonzero(d_copy == 0)}")
    assert np.all(np.isfinite(low))
    assert np.all(anti_got > 1e-5)
    has_nugget = copy_got > p.sigma[1] ** 2 + 0.5 * p.nugget[1]
    assert np.array_equal(has_nugget, d_copy == 0)
    # one rounding of r at the antipode moves the oracle's own entry by 1.55e-7 relative (measured in
    # tests/test_global_sites_host.py): rtol 5e-13 plus that move, entry by entry
    tol = gs.joint_cov_tolerance(p, coords, S)
    diff = np.abs(np.tril(got) - np.tril(S))
    print(f"antipodes site_order {site_order} exact {exact}: largest |difference| / bound {np.max(diff / np.maximum(np.tril(tol), 1e-300)):.3f}; "
          f"entries beyond plain rtol 5e-13: {np.count_nonzero(diff > 5e-13 * np.abs(np.tril(S)))}")
    assert np.all(diff <= np.tril(tol))
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. more deferred pairs than the worklist holds
# ---------------------------------------------------------------------------------------------------------------------
def cluster_sample():
    """20 000 (row, col) of the stacked order, 5 000 from each of the four blocks, 200 of them on the diagonal"""
    if "sample" not in _cache:
        rng = np.random.default_rng(5)
        n = 2100
        rows = np.concatenate([rng.integers(0, n, 5000) + a for a in (0, 0, n, n)])
        cols = np.concatenate([rng.integers(0, n, 5000) + b for b in (0, n, 0, n)])
        cols[:100] = rows[:100]
        cols[15000:15100] = rows[15000:15100]
        _cache["sample"] = (rows, cols)
    return _cache["sample"]


def oracle_entries(p, coords, rows, cols):
    """orc.joint_cov at the given pairs only (the oracle's distance on chunks of 250 pairs, its covariances element-wise)"""
    allc = np.vstack(coords)
    n0 = len(coords[0])
    d = np.empty(len(rows))
    for s in range(0, len(rows), 250):
        d[s:s + 250] = orc.haversine_km(allc[rows[s:s + 250]], allc[cols[s:s + 250]]).diagonal()
    pr, pc = (rows >= n0).astype(int), (cols >= n0).astype(int)
    out = np.empty(len(rows))
    for i in (0, 1):
        k = (pr == i) & (pc == i)
        out[k] = orc.covariance(p, i, d[k])
    k = pr != pc
    out[k] = orc.cross_covariance(p, 0, 1, d[k])
    return out


@pytest.mark.parametrize("noise", [False, True])
def test_worklist_overflow_in_the_sigma_assembly(native, noise):
    """CLUSTERS: every cross pair is beyond the table and there are more of them than the worklist holds, so the table attempt is
    thrown away and the exact kernels write every entry: the bits of an exact_cov handle.  A second assembly on the same handle
    gives the same bits and the same count (the alternating counters), and with noise the diagonal carries s d once."""
    coords, values = gs.CLUSTERS["coords"], gs.CLUSTERS["values"]
    pv = gs.CLUSTERS["params"]
    p = orc.Params.from_flat(pv)
    rows, cols = cluster_sample()
    d, scales = None, (1.7, 0.6)
    if noise:
        rng = np.random.default_rng(9)
        d = [1e-2 * 10.0 ** rng.uniform(-1, 1, 2100), 1e-2 * 10.0 ** rng.uniform(-1, 1, 2100)]
    h, _ = make_handle(native, pv, coords, values, noise=d, scales=scales)
    h.table_fallbacks()
    h.assemble_joint()
    fb = h.table_fallbacks()
    assert all(t["enabled"] for t in tables_of(h))
    got = h.debug_get_entries(rows, cols)
    hx, _ = make_handle(native, pv, coords, values, noise=d, scales=scales, exact_cov=1)
    hx.assemble_joint()
    gotx = hx.debug_get_entries(rows, cols)
    ref = oracle_entries(p, coords, rows, cols)
    if noise:
        dv = np.concatenate([scales[0] * d[0], scales[1] * d[1]])
        ref = ref + np.where(rows == cols, dv[rows], 0.0)
    h.assemble_joint()
    fb2 = h.table_fallbacks()
    again = h.debug_get_entries(rows, cols)
    print(f"K1 overflow noise {noise}: fallbacks {fb} then {fb2} (capacity {gs.WORKLIST_CAP}), sample max rel to the oracle "
          f"{max_rel(got, ref):.2e}, bit-equal to the exact handle: {np.array_equal(got, gotx)}")
    assert fb > gs.WORKLIST_CAP and fb2 == fb
    assert np.array_equal(got, gotx)
    assert np.array_equal(again, got)
    np.testing.assert_allclose(got, ref, rtol=5e-13, atol=1e-300)
    h.close()
    hx.close()


def test_worklist_overflow_in_the_right_hand_sides(native):
    """K2 after an overflow: process 0 at 2 048 sites inside B's box -- 2 100 x 2 048 pairs beyond the table.  The second
    attempt runs the exact kernels on the site transforms the discarded table launch stored (the strips of block column 0),
    where the exact_cov handle transforms the sites in a launch of their own: pred / pred_err have the bits of the exact_cov
    handle (seen on an MI355X: the two transforms agree in every bit).  Afterwards an ordinary predict gives the bits and the fallback count of a fresh
    handle: the overflow left no state behind."""
    coords, values = gs.CLUSTERS["coords"], gs.CLUSTERS["values"]
    pv = gs.CLUSTERS["params"]
    rng = np.random.default_rng(6)
    (la, lb), (oa, ob) = gs.CLUSTERS["box_b"]
    pc = np.column_stack([rng.uniform(la, lb, 2048), rng.uniform(oa, ob, 2048)])
    h, p = make_handle(native, pv, coords, values)
    h.assemble_joint()
    assert h.factor() == 0
    tabs = tables_of(h)
    n_out = gs.count_outside_aux(coords, pc, 0, tabs)
    assert n_out > gs.WORKLIST_CAP
    h.table_fallbacks()
    pred, err = h.predict(0, pc)
    fb = h.table_fallbacks()
    hx, _ = make_handle(native, pv, coords, values, exact_cov=1)
    hx.assemble_joint()
    assert hx.factor() == 0
    px, ex = hx.predict(0, pc)
    pick = np.arange(0, 2048, 32)
    rp, re = orc.joint_predict(p, coords, values, pc[pick], 0, HAV)
    same = np.array_equal(pred, px) and np.array_equal(err, ex)
    print(f"K2 overflow: fallbacks {fb} (strictly outside {n_out}, capacity {gs.WORKLIST_CAP}); bit-equal to the exact handle: "
          f"{same}; pred rel to the oracle {rel(pred[pick], rp):.2e}, |d var| {np.max(np.abs(err[pick] ** 2 - re ** 2)):.2e}")
    assert fb > gs.WORKLIST_CAP and fb >= n_out
    assert rel(pred[pick], rp) < 1e-8 and np.max(np.abs(err[pick] ** 2 - re ** 2)) < 1e-9
    assert same
    # the handle afterwards
    pg = gs.globe_pred_sites(np.random.default_rng(1070), 70)
    h.table_fallbacks()
    p1, e1 = h.predict(0, pg)
    fb1 = h.table_fallbacks()
    hf, _ = make_handle(native, pv, coords, values)
    hf.assemble_joint()
    assert hf.factor() == 0
    hf.table_fallbacks()
    pf, ef = hf.predict(0, pg)
    fbf = hf.table_fallbacks()
    print(f"after the overflow: fallbacks {fb1}, a fresh handle's {fbf}")
    assert np.array_equal(p1, pf) and np.array_equal(e1, ef) and fb1 == fbf
    assert fb1 >= gs.count_outside_aux(coords, pg, 0, tabs)
    for x in (h, hx, hf):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the Euclidean twin
# ---------------------------------------------------------------------------------------------------------------------
def euclid_problem():
    if "euclid" not in _cache:
        from sif_xco2_cokriging_amd import synth
        pb = synth.unit_square_problem(450, grid_side=2)
        rng = np.random.default_rng(8)
        allc = np.vstack(pb["coords"])
        lo, hi = allc.min(axis=0), allc.max(axis=0)
        diag = float(np.hypot(*(hi - lo)))
        ang = rng.uniform(0, 2 * np.pi, 24)
        # 3.5 .. 50 diagonals from the centre of the box: at least 3 from every datum, q >= 9 squared diagonals
        far = 0.5 * (lo + hi) + (diag * np.geomspace(3.5, 50.0, 24))[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
        pc = np.vstack([rng.random((24, 2)), far])[rng.permutation(48)]
        _cache["euclid"] = (pb, pc, diag)
    return _cache["euclid"]


def test_euclid_prediction_sites_beyond_the_table(native):
    """prediction sites 3 to 50 box diagonals away from the data lie beyond q_hi (at most 8 squared diagonals): K2 defers them"""
    pb, pc, diag = euclid_problem()
    coords, values = pb["coords"], pb["values"]
    h, p = make_handle(native, pb["params"], coords, values, metric=EUC)
    h.assemble_joint()
    assert h.factor() == 0
    tabs = tables_of(h)
    assert all(t["enabled"] for t in tabs) and all(4 * diag ** 2 <= t["q_hi"] < 9 * diag ** 2 for t in tabs), (tabs, diag)
    for i in (0, 1):
        n_out = gs.count_outside_aux(coords, pc, i, tabs, EUC)
        h.table_fallbacks()
        pred, err = h.predict(i, pc)
        fb = h.table_fallbacks()
        rp, re = orc.joint_predict(p, coords, values, pc, i, EUC)
        print(f"euclid i {i}: fallbacks {fb}, strictly outside {n_out}; pred rel {rel(pred, rp):.2e}, |d var| "
              f"{np.max(np.abs(err ** 2 - re ** 2)):.2e}")
        assert fb >= n_out >= 24 * 900
        assert rel(pred, rp) < 1e-8 and np.max(np.abs(err ** 2 - re ** 2)) < 1e-9
    h.close()


@pytest.mark.parametrize("tile_min", TILE_MIN)
def test_euclid_local_systems_beyond_the_table(native, tile_min):
    pb, pc, diag = euclid_problem()
    coords, values = pb["coords"], pb["values"]
    if "euclid_local" not in _cache:
        _cache["euclid_local"] = orc.local_predict(orc.Params.from_flat(pb["params"]), coords, values, pc, 0, EUC, 1e9)[:2]
    rp, re = _cache["euclid_local"]
    h, _ = make_handle(native, pb["params"], coords, values, metric=EUC, **({} if tile_min is None else {"local_tile_min": tile_min}))
    pred, err, info = h.predict_local(0, pc, max_dist=1e9)
    print(f"euclid local tile_min {tile_min}: max |d pred| {np.max(np.abs(pred - rp)):.2e}, max |d var| "
          f"{np.max(np.abs(err ** 2 - re ** 2)):.2e}")
    assert info["k_max"] == 900 and info["n_empty"] == 0 and info["n_not_pd"] == 0
    np.testing.assert_allclose(pred, rp, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err ** 2, re ** 2, rtol=RTOL, atol=ATOL)
    h.close()
