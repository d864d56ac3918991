"""GPU tests of the Gaussian log-likelihood and its gradient: include/cokrige.h ck_loglik, native.Handle.loglik and
model.MultivariateMatern.log_likelihood / fit_likelihood against a dense numpy chain (oracle covariances, slogdet,
cho_solve), and the state the call leaves on the handle."""
import numpy as np
import pytest
from numpy.linalg import LinAlgError
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import minimize

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.75, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_EUC = [0.99, 0.81, 0.7, 1.5, 2.2, 2.5, 2.5, 2.5, 0.02, 0.025, 0.3]
BIV_HALF = [1.1, 0.9, 1.5, 1.5, 0.5, 400.0, 450.0, 300.0, 0.03, 0.02, 0.0]   # nu = 1.5 / 0.5 exactly, rho = 0
UNI = [1.1, 0.6, 380.0, 0.03]
UNI_EUC = [1.1, 2.5, 2.0, 0.03]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_data(seed, params, metric, n0=700, n1=650):
    """two processes whose sites overlap (co-located pairs across the processes: h == 0 off the diagonal), sizes that are not
    multiples of 64 and N over several 512-wide panels; values drawn from the model.  (A site repeated inside one process
    makes Sigma exactly singular: the nugget enters every pair at h == 0, so the two rows are equal.)"""
    rng = np.random.default_rng(seed)
    p = orc.Params.from_flat(params)
    m = n0 + n1
    if metric == HAV:
        pts = np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])
    else:
        pts = np.column_stack([rng.uniform(0, 10, m), rng.uniform(0, 10, m)])
    c0 = pts[:n0].copy()
    if p.n_procs == 1:
        coords = [c0]
    else:
        c1 = pts[n0 // 2:n0 // 2 + n1].copy()            # half of process 1 co-located with process 0
        coords = [c0, c1]
    S = orc.joint_cov(p, coords, metric)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
    values = [z[:n0]] if p.n_procs == 1 else [z[:n0], z[n0:]]
    return coords, values


def dense_ll(params, coords, values, metric):
    """(l, log|Sigma|, z^T Sigma^-1 z) of the dense chain"""
    S = orc.joint_cov(orc.Params.from_flat(params), coords, metric)
    z = np.concatenate(values)
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    quad = float(z @ cho_solve(cho_factor(S, lower=True), z))
    return -0.5 * (len(z) * np.log(2 * np.pi) + logdet + quad), logdet, quad


def fd_grad(params, coords, values, metric):
    """4th-order central differences of the dense log-likelihood in every parameter"""
    x = np.asarray(params, dtype=float)
    g = np.empty(x.size)
    nug = (3,) if x.size == 4 else (8, 9)
    for k in range(x.size):
        e = 1e-4 if k in nug else 1e-3 * max(abs(x[k]), 1.0)   # nuggets are small
        f = []
        for d in (-2, -1, 1, 2):
            y = x.copy()
            y[k] += d * e
            f.append(dense_ll(y, coords, values, metric)[0])
        g[k] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * e)
    return g


def handle(native, params, coords, values, metric, site_order=1):
    p = orc.Params.from_flat(params)
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
    h.assemble_joint()
    return h


@pytest.mark.parametrize("params,metric", [(BIV, HAV), (BIV_EUC, EUC), (UNI, HAV), (UNI_EUC, EUC)])
def test_loglik_against_dense(native, params, metric):
    coords, values = make_data(11, params, metric)
    ref = dense_ll(params, coords, values, metric)
    outs = []
    for so in (1, 0):
        h = handle(native, params, coords, values, metric, site_order=so)
        info, out3, g = h.loglik(False)
        assert info == 0 and g is None
        outs.append(out3)
        for a, b in zip(out3, ref):
            assert abs(a - b) <= 1e-8 * abs(b), (so, out3, ref)
        h.close()
    assert abs(outs[0][0] - outs[1][0]) <= 1e-11 * abs(outs[1][0])   # site orders agree to rounding


@pytest.mark.parametrize("params,metric", [(BIV, HAV), (BIV_HALF, HAV), (BIV_EUC, EUC), (UNI, HAV), (UNI_EUC, EUC)])
def test_gradient_against_dense_differences(native, params, metric):
    coords, values = make_data(12, params, metric, n0=600, n1=570)
    h = handle(native, params, coords, values, metric)
    info, out3, g = h.loglik(True)
    assert info == 0 and g.shape == (len(params),)
    ref = fd_grad(params, coords, values, metric)
    err = np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)
    assert np.max(err) < 1e-6, (err, g, ref)
    assert abs(out3[0] - dense_ll(params, coords, values, metric)[0]) <= 1e-8 * abs(out3[0])
    t = h.loglik_timings()
    assert t["sweep_ms"] > 0 and t["syrk_ms"] > 0 and t["contract_ms"] > 0 and t["factor_ms"] > 0
    h.close()


def test_determinism_and_state(native):
    coords, values = make_data(13, BIV, HAV)
    grid = np.column_stack([np.linspace(26, 49, 300), np.linspace(-118, -72, 300)])
    h0 = handle(native, BIV, coords, values, HAV)
    assert h0.factor() == 0
    p0, e0 = h0.predict(1, grid)
    h0.close()
    h = handle(native, BIV, coords, values, HAV)
    r1 = h.loglik(True)
    r2 = h.loglik(True)            # the resident factor of the first call
    assert r1[1] == r2[1] and np.array_equal(r1[2], r2[2])
    assert h.loglik_timings()["factor_ms"] == 0.0
    with pytest.raises(native.NativeError, match="ck_loglik"):
        h.verify_model()
    p1, e1 = h.predict(1, grid)    # the factor stayed resident: the same bits as without the call
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1)
    assert h.verify_model() == 0   # a ck_predict makes the check possible again
    h.assemble_joint()
    r3 = h.loglik(True)            # assembled and factored again by the call itself
    assert r3[1] == r1[1] and np.array_equal(r3[2], r1[2])
    h.close()


def test_refusals(native):
    from sif_xco2_cokriging_amd import fields, model
    coords, values = make_data(14, BIV, HAV, n0=300, n1=280)
    bad = list(BIV)
    bad[10] = 1.5                  # |rho| > 1 with co-located sites: Sigma is not positive definite
    h = handle(native, bad, coords, values, HAV)
    info, out3, g = h.loglik(True)
    assert info > 0 and np.all(np.isnan(out3)) and np.all(np.isnan(g))
    try:
        np.linalg.cholesky(orc.joint_cov(orc.Params.from_flat(bad), coords, HAV))
        assert False, "the dense chain should fail too"
    except LinAlgError:
        pass
    h.close()
    mod = model.MultivariateMatern(2)
    mod.params.set_values(bad)
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    with pytest.raises(LinAlgError, match=r"^\d+-th leading minor of the array is not positive definite$"):
        mod.log_likelihood(mf)
    hp = native.Handle(devices=[0, 0], rank=0)   # a partitioned handle: the single-process form only
    with pytest.raises(native.NativeError, match="single-process form"):
        hp.loglik(False)
    hp.close()


def test_model_log_likelihood_reuses_its_handle(native):
    from sif_xco2_cokriging_amd import fields, model
    coords, values = make_data(15, BIV, HAV, n0=300, n1=280)
    mod = model.MultivariateMatern(2)
    mod.params.set_values(BIV)
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    ll, g = mod.log_likelihood(mf, gradient=True)
    h = mod._lik[1]
    x = np.array(BIV)
    x[5] = 470.0
    mod.params.set_values(x)
    ll2 = mod.log_likelihood(mf)
    assert mod._lik[1] is h
    assert abs(ll2 - dense_ll(x, coords, values, HAV)[0]) <= 1e-8 * abs(ll2)
    assert abs(ll - dense_ll(BIV, coords, values, HAV)[0]) <= 1e-8 * abs(ll)
    assert list(mod.params.get_names()) == ["sigma_11", "sigma_22", "nu_11", "nu_12", "nu_22", "len_scale_11",
                                            "len_scale_12", "len_scale_22", "nugget_11", "nugget_22", "rho_12"]


def _projected_gradient(x, g, bounds):
    """the components of the ascent direction g that stay inside the box at x"""
    pg = np.array(g, dtype=float)
    for k, (lo, hi) in enumerate(bounds):
        if x[k] <= lo and pg[k] < 0 or x[k] >= hi and pg[k] > 0:
            pg[k] = 0.0
    return pg


def test_fit_likelihood_bivariate(native):
    from sif_xco2_cokriging_amd import fields, model
    truth = [1.0, 0.8, 0.8, 1.1, 1.4, 450.0, 450.0, 450.0, 0.02, 0.03, 0.5]
    coords, values = make_data(16, truth, HAV, n0=1000, n1=1000)
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    mod = model.MultivariateMatern(2)
    start = [1.2, 1.0, 1.0, 1.3, 1.5, 600.0, 600.0, 600.0, 0.05, 0.05, 0.2]
    mod.params.set_values(start)
    ll_start = mod.log_likelihood(mf)
    mod.params.set_values(truth)
    ll_truth = mod.log_likelihood(mf)
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params)
    r = mod.fit_result
    x = mod.params.get_values().astype(float)
    bounds = mod.params.get_bounds()
    assert all(lo <= v <= hi for v, (lo, hi) in zip(x, bounds))
    assert r.loglik >= ll_truth and r.loglik >= ll_start, (r.loglik, ll_truth, ll_start)
    assert abs(r.aic - (2 * 11 - 2 * r.loglik)) < 1e-9 * abs(r.aic)
    pg = _projected_gradient(x, r.gradient, bounds) * np.array([hi - lo for lo, hi in bounds])
    assert np.max(np.abs(pg)) < 0.5, (pg, r.message)
    assert r.n_eval > 5 and r.n_not_pd >= 0


def test_fit_likelihood_univariate_matches_dense_scipy(native):
    from sif_xco2_cokriging_amd import fields, model
    truth = [1.1, 1.2, 380.0, 0.05]
    coords, values = make_data(17, truth, HAV, n0=400)
    mf = fields.MultiField([fields.Field(coords[0], values[0])])
    mod = model.MultivariateMatern(1)
    start = np.array([1.0, 1.5, 500.0, 0.02])
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params)
    bounds = mod.params.get_bounds()
    lo = np.array([b[0] for b in bounds])
    wd = np.array([b[1] - b[0] for b in bounds])

    def cost(u):
        return -dense_ll(lo + wd * u, coords, values, HAV)[0]

    res = minimize(cost, (start - lo) / wd, method="L-BFGS-B", bounds=[(0.0, 1.0)] * 4,
                   options={"ftol": 1e-14, "gtol": 1e-9, "eps": 1e-9, "maxiter": 1000})
    ll_scipy = -res.fun
    assert mod.fit_result.loglik >= ll_scipy - 1e-4, (mod.fit_result.loglik, ll_scipy, mod.params.get_values(), res.x)
    assert abs(mod.fit_result.loglik - dense_ll(mod.params.get_values(), coords, values, HAV)[0]) < 1e-8 * abs(ll_scipy)


def test_fit_likelihood_survives_non_pd_steps(native):
    from sif_xco2_cokriging_amd import fields, model
    # nu_12 below the marginals' mean: rho = +-0.9 and beyond is not positive definite on these co-located sites
    truth = [1.0, 1.0, 1.0, 0.9, 1.0, 300.0, 300.0, 300.0, 0.01, 0.01, 0.7]
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(30, 45, 600), rng.uniform(-110, -90, 600)])
    coords = [pts[:400], pts[200:600]]
    S = orc.joint_cov(orc.Params.from_flat(truth), coords, HAV)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
    values = [z[:400], z[400:]]
    edge = list(truth)
    edge[10] = 1.0
    with pytest.raises(LinAlgError):
        np.linalg.cholesky(orc.joint_cov(orc.Params.from_flat(edge), coords, HAV))
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    mod = model.MultivariateMatern(2)
    start = list(truth)
    start[10] = 0.8
    mod.params.set_values(start)
    ll_start = mod.log_likelihood(mf)
    names = list(mod.params.get_names())
    mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n != "rho_12"])
    r = mod.fit_result
    x = mod.params.get_values()
    assert r.n_not_pd > 0 and r.n_free == 1 and r.free == ["rho_12"]
    assert np.array_equal(np.delete(x, 10), np.delete(np.array(start), 10))   # the fixed ones stayed
    assert -1.0 <= x[10] <= 1.0 and np.isfinite(r.loglik) and r.loglik >= ll_start


def test_fullsize_gradient(native):
    """BASELINE configs[2]: N = 40 000 on the CONUS lattice; the l_11 and rho components against central differences of
    the device log-likelihood itself"""
    from sif_xco2_cokriging_amd import synth
    pb = synth.conus_problem(20000)
    params = list(pb["params"])
    h = handle(native, params, pb["coords"], pb["values"], HAV)
    info, out3, g = h.loglik(True)
    assert info == 0 and np.isfinite(out3[0]) and np.all(np.isfinite(g))
    t = h.loglik_timings()
    print("N = 40 000 loglik + gradient:", t)
    h.close()
    for k, e in ((5, 1e-3 * params[5]), (10, 1e-3)):
        f = []
        for d in (-2, -1, 1, 2):
            y = list(params)
            y[k] += d * e
            hk = handle(native, y, pb["coords"], pb["values"], HAV)
            info, o, _ = hk.loglik(False)
            hk.close()
            assert info == 0
            f.append(o[0])
        fd = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * e)
        assert abs(g[k] - fd) <= 1e-5 * max(abs(fd), 1.0), (k, g[k], fd)
