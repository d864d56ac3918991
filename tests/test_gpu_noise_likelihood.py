"""GPU tests of the likelihood with per-observation measurement-error variances: include/cokrige.h ck_set_noise with ck_loglik /
ck_loglik_reml, ck_loglik_noise_grad, and MultivariateMatern.log_likelihood / fit_likelihood(measurement_error=..., fit_noise_scale=...).

Truth is dense numpy in this file: Sigma_noise = orc.joint_cov(p, coords, metric) + diag(s d), cho_factor / cho_solve / slogdet.
The 11 parameter derivatives against fourth-order differences of that dense noisy likelihood (the scheme of fd_grad in
tests/test_gpu_likelihood.py, copied) at n0 = 600, n1 = 570; the noise-scale derivatives against the exact dense
1/2 sum_a (alpha_a^2 - (Sigma^-1)_aa) d_a (REML: P in place of Sigma^-1).  Bounds: 1e-8 relative for l, log|Sigma| and the quadratic
form, 1e-6 max(|ref|, 1) for gradient entries (tests/test_gpu_likelihood.py).

Largest deviations seen on an MI355X over all cases of this file: l, log|Sigma| and the quadratic form 1.0e-14 relative (REML
5.7e-15); the 11 gradient entries 7.1e-9 of max(|ref|, 1) against the differences; the noise-scale derivatives 2.3e-13 (REML
1.4e-13).  The fit from scales (1, 1) on data simulated with (2.0, 0.5) ended at (2.75, 0.63) with l = -501.2 against -505.2 at
the true parameters, 77 evaluations, projected gradient 3.0e-4 (the recovered scales are printed, not asserted: their
sampling spread at N = 980 has not been measured)."""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.75, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_ZERO = [0.99, 0.81, 0.39, 0.75, 1.0, 460.0, 460.0, 460.0, 0.0, 0.0, -0.19]
BIV_EUC = [0.99, 0.81, 0.7, 1.5, 2.2, 2.5, 2.5, 2.5, 0.02, 0.025, 0.3]
SCALE = (1.5, 0.7)
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_data(seed, params, metric, n0, n1, scale=SCALE):
    key = (seed, tuple(params), metric, n0, n1, scale)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        p = orc.Params.from_flat(params)
        m = n0 + n1
        if metric == HAV:
            pts = np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])
        else:
            pts = np.column_stack([rng.uniform(0, 10, m), rng.uniform(0, 10, m)])
        coords = [pts[:n0].copy(), pts[n0 // 2:n0 // 2 + n1].copy()]   # half of process 1 co-located with process 0
        d = []
        for k, n in enumerate((n0, n1)):
            x = 1e-2 * p.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, n)
            x[rng.random(n) < 0.1] = 0.0
            d.append(x)
        S = orc.joint_cov(p, coords, metric) + np.diag(np.concatenate([scale[0] * d[0], scale[1] * d[1]]))
        z = np.linalg.cholesky(S) @ rng.standard_normal(m)
        _cache[key] = (coords, [z[:n0].copy(), z[n0:].copy()], d)
    return _cache[key]


def noisy_cov(params, coords, d, metric, scale=SCALE):
    return orc.joint_cov(orc.Params.from_flat(params), coords, metric) + np.diag(np.concatenate([scale[0] * d[0], scale[1] * d[1]]))


def dense_ll(params, coords, values, d, metric, scale=SCALE):
    """(l, log|Sigma|, z^T Sigma^-1 z) of the dense noisy chain"""
    S = noisy_cov(params, coords, d, metric, scale)
    z = np.concatenate(values)
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    quad = float(z @ cho_solve(cho_factor(S, lower=True), z))
    return -0.5 * (len(z) * np.log(2 * np.pi) + logdet + quad), logdet, quad


def fd_grad(params, coords, values, d, metric):
    """4th-order central differences of the dense noisy log-likelihood in every parameter"""
    x = np.asarray(params, dtype=float)
    g = np.empty(x.size)
    nug = (8, 9)
    for k in range(x.size):
        e = 1e-4 if k in nug else 1e-3 * max(abs(x[k]), 1.0)   # nuggets are small
        f = []
        for s in (-2, -1, 1, 2):
            y = x.copy()
            y[k] += s * e
            f.append(dense_ll(y, coords, values, d, metric)[0])
        g[k] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * e)
    return g


def handle(native, params, coords, values, d, metric, scale=SCALE, site_order=1):
    p = orc.Params.from_flat(params)
    h = native.Handle(0)
    if site_order != 1:
        h.set_option("site_order", site_order)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
        if d is not None and d[k] is not None:
            h.set_noise(k, d[k], scale[k])
    h.assemble_joint()
    return h


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- 1. values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,metric", [(BIV, HAV), (BIV_ZERO, HAV), (BIV_EUC, EUC)])
@pytest.mark.parametrize("site_order", [0, 1])
def test_values_match_the_dense_chain(native, params, metric, site_order):
    coords, values, d = make_data(5, params, metric, 300, 290)
    h = handle(native, params, coords, values, d, metric, site_order=site_order)
    info, out3, _ = h.loglik(False)
    assert info == 0
    ref = dense_ll(params, coords, values, d, metric)
    errs = [rel(a, b) for a, b in zip(out3, ref)]
    print(f"l, log|Sigma|, quad: rel {errs}")
    assert max(errs) < 1e-8
    info, again, _ = h.loglik(True)
    assert again == out3   # the same bits with the gradient
    h.close()


# ---- 2. / 3. the gradients --------------------------------------------------------------------------------------------------
def test_gradient_against_fourth_order_differences(native):
    coords, values, d = make_data(9, BIV, HAV, 600, 570)
    h = handle(native, BIV, coords, values, d, HAV)
    info, out3, g = h.loglik(True)
    assert info == 0
    gs = h.loglik_noise_grad()
    ref = fd_grad(BIV, coords, values, d, HAV)
    dev = np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)
    print(f"gradient: max dev {dev.max():.3e} (entries {dev})")
    assert np.all(dev < 1e-6)
    # the noise-scale derivatives, exact: 1/2 sum_a (alpha_a^2 - (Sigma^-1)_aa) d_a
    S = noisy_cov(BIV, coords, d, HAV)
    Si = np.linalg.inv(S)
    a = Si @ np.concatenate(values)
    w = 0.5 * (a * a - np.diag(Si)) * np.concatenate(d)
    rs = np.array([w[:600].sum(), w[600:].sum()])
    ds = np.abs(gs - rs) / np.maximum(np.abs(rs), 1.0)
    print(f"noise-scale gradient: {gs} against {rs}, dev {ds}")
    assert np.all(ds < 1e-6)
    g2 = h.loglik(True)[2]
    assert np.array_equal(g, g2) and np.array_equal(gs, h.loglik_noise_grad())   # repeated calls: the same bits
    h.close()


@pytest.mark.parametrize("params,metric", [(BIV_ZERO, HAV), (BIV_EUC, EUC)])
@pytest.mark.parametrize("site_order", [0, 1])
def test_noise_scale_gradient_exact(native, params, metric, site_order):
    """N = 590 over two panels; process 1 without noise gives 0; a scale of 0 keeps its derivative"""
    coords, values, d = make_data(5, params, metric, 300, 290)
    for dd, sc in ((d, SCALE), ([d[0], None], SCALE), (d, (0.0, 0.7))):
        h = handle(native, params, coords, values, dd, metric, scale=sc, site_order=site_order)
        info, out3, g = h.loglik(True)
        assert info == 0
        gs = h.loglik_noise_grad()
        dz = [x if x is not None else np.zeros(len(c)) for x, c in zip(dd, coords)]
        Si = np.linalg.inv(noisy_cov(params, coords, dz, metric, sc))
        a = Si @ np.concatenate(values)
        w = 0.5 * (a * a - np.diag(Si)) * np.concatenate(dz)
        rs = np.array([w[:300].sum(), w[300:].sum()])
        ds = np.abs(gs - rs) / np.maximum(np.abs(rs), 1.0)
        print(f"noise-scale gradient {gs} against {rs}: dev {ds}")
        assert np.all(ds < 1e-6)
        if dd[1] is None:
            assert gs[1] == 0.0
        h.assemble_joint()
        with pytest.raises(native.NativeError, match="ck_loglik_noise_grad"):
            h.loglik_noise_grad()
        h.close()


# ---- 4. REML ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,metric", [(BIV, HAV), (BIV_EUC, EUC)])
def test_reml_noise_scale_gradient(native, params, metric):
    coords, values, d = make_data(5, params, metric, 300, 290)
    values = [v + 0.4 for v in values]
    h = handle(native, params, coords, values, d, metric)
    for k in range(2):
        h.set_trend(k, np.ones((len(coords[k]), 1)))
    info, out4, g = h.loglik_reml(True)
    assert info == 0
    gs = h.loglik_noise_grad()
    S = noisy_cov(params, coords, d, metric)
    X = np.zeros((590, 2))
    X[:300, 0], X[300:, 1] = 1.0, 1.0
    z = np.concatenate(values)
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    SX = Si @ X
    A = X.T @ SX
    P = Si - SX @ np.linalg.solve(A, SX.T)
    a = P @ z
    _, ldS = np.linalg.slogdet(S)
    _, ldA = np.linalg.slogdet(A)
    quad = float(z @ a)
    ref = (-0.5 * (588 * np.log(2 * np.pi) + ldS + ldA + quad), ldS, ldA, quad)
    errs = [rel(x, y) for x, y in zip(out4, ref)]
    print(f"REML values: rel {errs}")
    assert max(errs) < 1e-8
    w = 0.5 * (a * a - np.diag(P)) * np.concatenate(d)
    rs = np.array([w[:300].sum(), w[300:].sum()])
    ds = np.abs(gs - rs) / np.maximum(np.abs(rs), 1.0)
    print(f"REML noise-scale gradient {gs} against {rs}: dev {ds}")
    assert np.all(ds < 1e-6)
    h.close()


# ---- 5. the fit -------------------------------------------------------------------------------------------------------------
def test_fit_noise_scale(native):
    from sif_xco2_cokriging_amd import fields, model
    truth = [1.0, 0.8, 0.8, 1.1, 1.4, 450.0, 450.0, 450.0, 0.02, 0.03, 0.5]
    true_scale = (2.0, 0.5)
    coords, values, d = make_data(16, truth, HAV, 500, 480, scale=true_scale)
    mf = fields.MultiField([fields.Field(coords[k], values[k], variance_estimate=d[k]) for k in range(2)])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(truth)
    ll_truth = mod.log_likelihood(mf, measurement_error=True, noise_scale=true_scale)
    ref = dense_ll(truth, coords, values, d, HAV, true_scale)[0]
    assert rel(ll_truth, ref) < 1e-8
    ll, g, gs = mod.log_likelihood(mf, gradient=True, measurement_error=True, noise_scale=true_scale)
    assert ll == ll_truth and len(g) == 11 and len(gs) == 2
    assert isinstance(mod.log_likelihood(mf, gradient=True), tuple) and len(mod.log_likelihood(mf, gradient=True)) == 2
    start = [1.2, 1.0, 1.0, 1.3, 1.5, 600.0, 600.0, 600.0, 0.05, 0.05, 0.2]
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params, measurement_error=True, noise_scale=(1.0, 1.0), fit_noise_scale=True)
    r = mod.fit_result
    print(f"fitted noise scales {r.noise_scale} (truth {true_scale}), loglik {r.loglik} against {ll_truth} at the truth, "
          f"{r.n_eval} evaluations: {r.message}")
    assert r.loglik >= ll_truth, (r.loglik, ll_truth)
    assert r.n_free == 13 and abs(r.aic - (2 * 13 - 2 * r.loglik)) < 1e-9 * abs(r.aic)
    x = mod.params.get_values().astype(float)
    bounds = mod.params.get_bounds()
    pg = np.array(r.gradient, dtype=float)
    for k, (lo, hi) in enumerate(bounds):
        if x[k] <= lo and pg[k] < 0 or x[k] >= hi and pg[k] > 0:
            pg[k] = 0.0
    pg = pg * np.array([hi - lo for lo, hi in bounds])
    # the scales are optimised as log s over [log 1e-3, log 1e3] mapped onto [0, 1]: the same unit-box gradient
    ps = np.array(r.noise_gradient) * np.array(r.noise_scale) * (np.log(1e3) - np.log(1e-3))
    for k, s in enumerate(r.noise_scale):
        if s <= 1e-3 and ps[k] < 0 or s >= 1e3 and ps[k] > 0:
            ps[k] = 0.0
    print(f"projected gradient {pg}, of the scales {ps}")
    assert np.max(np.abs(pg)) < 0.5 and np.max(np.abs(ps)) < 0.5, (pg, ps, r.message)
