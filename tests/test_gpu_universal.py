"""GPU tests of universal cokriging and REML: include/cokrige.h ck_set_trend / ck_predict_universal / ck_loglik_reml,
native.Handle.set_trend / predict_universal / loglik_reml, Predictor(trend=...) and log_likelihood / fit_likelihood(trend=...)
against dense numpy chains (oracle covariances, the bordered Lagrange system, dense GLS and REML)."""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import minimize

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_EUC = [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.02, 0.025, -0.19]
UNI = [1.1, 0.6, 380.0, 0.03]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_data(seed, params, metric, n0=700, n1=650):
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


def pred_sites(rng, metric, m):
    if metric == HAV:
        return np.column_stack([rng.uniform(26, 49, m), rng.uniform(-118, -72, m)])
    return np.column_stack([rng.uniform(0.5, 9.5, m), rng.uniform(0.5, 9.5, m)])


def handle(native, p, coords, values, metric, site_order=1, factor=True):
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
    if factor:
        assert h.factor() == 0
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


def block_X(Fs):
    p = sum(F.shape[1] for F in Fs)
    X = np.zeros((sum(len(F) for F in Fs), p))
    r = c = 0
    for F in Fs:
        X[r:r + len(F), c:c + F.shape[1]] = F
        r += len(F)
        c += F.shape[1]
    return X


def x0_of(Fs, i, F0):
    p = sum(F.shape[1] for F in Fs)
    off = sum(F.shape[1] for F in Fs[:i])
    x0 = np.zeros((len(F0), p))
    x0[:, off:off + F0.shape[1]] = F0
    return x0


def dense_universal(p, coords, values, pc, i, metric, Fs, F0):
    """the bordered (Lagrange) system [[Sigma, X], [X^T, 0]] [lam; mu] = [c0; x0^T] solved densely, and dense GLS"""
    S = orc.joint_cov(p, coords, metric)
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    X = block_X(Fs)
    x0 = x0_of(Fs, i, F0)
    N, q = X.shape
    K = np.block([[S, X], [X.T, np.zeros((q, q))]])
    sol = np.linalg.solve(K, np.vstack([c0, x0.T]))
    lam, mu = sol[:N], sol[N:]
    z = np.concatenate(values)
    pred = lam.T @ z
    c00 = np.diag(orc.pred_cov(p, pc[:1], i, metric))[0]
    var = c00 - np.sum(lam * c0, axis=0) - np.sum(mu * x0.T, axis=0)
    cf = cho_factor(S, lower=True)
    A = X.T @ cho_solve(cf, X)
    beta = np.linalg.solve(A, X.T @ cho_solve(cf, z))
    return pred, var, beta, np.linalg.inv(A)


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


CASES = [  # params, metric, trend, i, m  (m + 1 + p on both sides of 16- and 256-row boundaries)
    (BIV, HAV, "constant", 0, 253), (BIV, HAV, "constant", 1, 254), (BIV, HAV, "linear", 0, 9), (BIV, HAV, "linear", 1, 10),
    (BIV_EUC, EUC, "linear", 0, 249), (BIV_EUC, EUC, "linear", 1, 250), (BIV_EUC, EUC, "cov", 1, 300),
    (UNI, HAV, "linear", 0, 300), (UNI, HAV, "cov", 0, 12), (UNI, HAV, "constant", 0, 14),
]


@pytest.mark.parametrize("params,metric,kind,i,m", CASES)
def test_dense_parity(native, params, metric, kind, i, m):
    p, coords, values = make_data(3, params, metric)
    pc = pred_sites(np.random.default_rng(m), metric, m)
    Fs = [design(kind, c, c) for c in coords]
    F0 = design(kind, coords[i], pc)
    h = handle(native, p, coords, values, metric)
    for k in range(p.n_procs):
        h.set_trend(k, Fs[k])
    pred, err, beta, cov = h.predict_universal(i, pc, F0)
    rp, rv, rb, rc = dense_universal(p, coords, values, pc, i, metric, Fs, F0)
    assert rel(pred, rp) < 1e-9
    assert np.max(np.abs(err ** 2 - rv)) < 1e-10
    assert rel(beta, rb) < 1e-9 and rel(cov, rc) < 1e-9
    # repeated calls: the same bits; the factor is untouched
    pred2, err2, beta2, _ = h.predict_universal(i, pc, F0)
    assert np.array_equal(pred, pred2) and np.array_equal(err, err2) and np.array_equal(beta, beta2)
    h.close()


def test_ordinary_cokriging_weights_and_interpolation(native):
    """nugget 0, prediction sites on the data of process i: pred = z, pred_err ~ 0"""
    par = list(BIV)
    par[8] = par[9] = 0.0
    p, coords, values = make_data(5, par, HAV, n0=500, n1=450)
    h = handle(native, p, coords, values, HAV)
    for k in range(2):
        h.set_trend(k, np.ones((len(coords[k]), 1)))
    for i in (0, 1):
        pred, err, _, _ = h.predict_universal(i, coords[i][:300], np.ones((300, 1)))
        assert np.max(np.abs(pred - values[i][:300])) < 1e-7
        assert np.max(err) < 1e-4
    h.close()


def test_ordinary_cokriging_weight_sums(native):
    """one constant column per process: the weights on process i sum to 1 and those on the other process to 0, read off
    the device predictor with indicator data (z = 1 on one process, 0 on the other)"""
    p, coords, _ = make_data(6, BIV, HAV, n0=500, n1=450)
    pc = pred_sites(np.random.default_rng(6), HAV, 300)
    for on in (0, 1):
        ind = [np.full(len(c), 1.0 if k == on else 0.0) for k, c in enumerate(coords)]
        h = handle(native, p, coords, ind, HAV)
        for k in range(2):
            h.set_trend(k, np.ones((len(coords[k]), 1)))
        for i in (0, 1):
            pred, _, _, _ = h.predict_universal(i, pc, np.ones((len(pc), 1)))
            assert np.max(np.abs(pred - (1.0 if i == on else 0.0))) < 1e-9, (on, i)
        h.close()


def test_relayout_keeps_the_trend_in_order(native):
    """a handle laid out again in another site order (option site_order; ck_factor's retry does the same) lays X out in
    the new order too: the same results as a fresh handle in that order"""
    p, coords, values = make_data(8, BIV, HAV)
    pc = pred_sites(np.random.default_rng(8), HAV, 300)
    Fs = [design("linear", c, c) for c in coords]
    F0 = design("linear", coords[0], pc)
    h = handle(native, p, coords, values, HAV)
    for k in range(2):
        h.set_trend(k, Fs[k])
    r1 = h.predict_universal(0, pc, F0)
    h.set_option("site_order", 0)
    h.assemble_joint()
    assert h.factor() == 0
    r2 = h.predict_universal(0, pc, F0)
    h.assemble_joint()
    l2 = h.loglik_reml(True)
    h0 = handle(native, p, coords, values, HAV, site_order=0)
    for k in range(2):
        h0.set_trend(k, Fs[k])
    r0 = h0.predict_universal(0, pc, F0)
    h0.assemble_joint()
    l0 = h0.loglik_reml(True)
    for a, b, c in zip(r2[:3], r0[:3], r1[:3]):
        assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))
        assert np.max(np.abs(a - c)) <= 1e-10 * max(1.0, np.max(np.abs(c)))
    assert l2[0] == l0[0] == 0
    assert np.allclose(l2[1], l0[1], rtol=1e-12, atol=0) and np.allclose(l2[2], l0[2], rtol=1e-10, atol=1e-10)
    h.close()
    h0.close()


def test_equivariance(native):
    p, coords, values = make_data(7, BIV, HAV)
    pc = pred_sites(np.random.default_rng(1), HAV, 400)
    Fs = [design("linear", c, c) for c in coords]
    F0 = design("linear", coords[1], pc)
    h = handle(native, p, coords, values, HAV)
    for k in range(2):
        h.set_trend(k, Fs[k])
    pred, err, beta, _ = h.predict_universal(1, pc, F0)
    gamma = np.array([0.5, -1.0, 2.0, 3.0, 0.25, -0.75])
    shifted = [values[0] + Fs[0] @ gamma[:3], values[1] + Fs[1] @ gamma[3:]]
    h2 = handle(native, p, coords, shifted, HAV)
    for k in range(2):
        h2.set_trend(k, Fs[k])
    pred2, err2, beta2, _ = h2.predict_universal(1, pc, F0)
    assert np.max(np.abs(pred2 - (pred + F0 @ gamma[3:]))) < 1e-9 * max(1.0, np.max(np.abs(pred2)))
    assert np.max(np.abs(beta2 - (beta + gamma))) < 1e-9 * max(1.0, np.max(np.abs(beta2)))
    assert np.max(np.abs(err2 - err)) < 1e-10
    h.close()
    h2.close()


def test_no_behaviour_change(native):
    p, coords, values = make_data(9, BIV, HAV)
    pc = pred_sites(np.random.default_rng(2), HAV, 500)
    h = handle(native, p, coords, values, HAV)
    pred0, err0 = h.predict(0, pc)
    pu, eu, b, c = h.predict_universal(0, pc)   # no trend: ck_predict's bits
    assert np.array_equal(pu, pred0) and np.array_equal(eu, err0) and b.size == 0
    for k in range(2):
        h.set_trend(k, design("linear", coords[k], coords[k]))
    pu1 = h.predict_universal(0, pc, design("linear", coords[0], pc))
    pred1, err1 = h.predict(0, pc)   # ck_predict after a universal call: its earlier bits
    assert np.array_equal(pred1, pred0) and np.array_equal(err1, err0)
    # site_order 0 and 1 agree
    h0 = handle(native, p, coords, values, HAV, site_order=0)
    for k in range(2):
        h0.set_trend(k, design("linear", coords[k], coords[k]))
    pu0 = h0.predict_universal(0, pc, design("linear", coords[0], pc))
    assert np.max(np.abs(pu0[0] - pu1[0])) < 1e-11 * max(1.0, np.max(np.abs(pu1[0])))
    assert np.max(np.abs(pu0[1] - pu1[1])) < 1e-11
    assert np.max(np.abs(pu0[2] - pu1[2])) < 1e-11 * max(1.0, np.max(np.abs(pu1[2])))
    h.close()
    h0.close()


def test_refusals_and_state(native):
    p, coords, values = make_data(11, BIV, HAV, n0=300, n1=280)
    pc = pred_sites(np.random.default_rng(3), HAV, 50)
    h = handle(native, p, coords, values, HAV, factor=False)
    n0 = len(coords[0])
    with pytest.raises(RuntimeError, match="at most 8"):
        h.set_trend(0, np.ones((n0, 9)))
    with pytest.raises(RuntimeError, match="data sites"):
        h.set_trend(0, np.ones((n0 - 1, 1)))
    bad = np.ones((n0, 2))
    bad[5, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        h.set_trend(0, bad)
    h.set_trend(0, np.ones((n0, 1)))
    with pytest.raises(RuntimeError, match="ck_factor"):
        h.predict_universal(0, pc, np.ones((50, 1)))
    assert h.factor() == 0
    h.set_trend(0, np.column_stack([np.ones(n0), np.ones(n0)]))   # a constant column twice on process 0
    with pytest.raises(RuntimeError, match="rank deficient.*process 0"):
        h.predict_universal(0, pc, np.ones((50, 2)))
    h.set_trend(0, np.ones((n0, 1)))
    h.predict(0, pc)
    assert h.verify_model() == 0
    h.predict_universal(0, pc, np.ones((50, 1)))
    with pytest.raises(RuntimeError, match="ck_predict_universal"):
        h.verify_model()
    buf = np.empty(64)
    with pytest.raises(RuntimeError, match="ck_predict_universal"):
        native._chk(native.lib().ck_aux_finish(h._h, native._p(buf), native._p(buf)))
    h.predict(0, pc)
    assert h.verify_model() == 0
    h.close()
    # n_k < p_k
    p1, c1, v1 = make_data(12, UNI, HAV, n0=3)
    h1 = handle(native, p1, c1, v1, HAV, factor=False)
    with pytest.raises(RuntimeError, match="3 data sites for 4 regressors"):
        h1.set_trend(0, np.ones((3, 4)))
    h1.close()
    # a partitioned handle
    hp = native.Handle(0, devices=[0, 0], rank=0)
    with pytest.raises(RuntimeError, match="single-process"):
        hp.predict_universal(0, pc)
    hp.close()


def _predictor(coords, values, params, **kw):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    mod = model.MultivariateMatern(len(coords), params=model.MaternParams(len(coords)).set_values(params))
    mf = fields.MultiField([fields.Field(c, v) for c, v in zip(coords, values)])
    return joint_prediction.Predictor(mod, mf, **kw)


def test_predictor_surface(native):
    p, coords, values = make_data(13, BIV, HAV)
    pc = pred_sites(np.random.default_rng(4), HAV, 400)
    P = _predictor(coords, values, BIV, trend="linear")
    pred, err = P.predict_arrays(1, pc)
    Fs = [design("linear", c, c) for c in coords]
    rp, rv, rb, rc = dense_universal(p, coords, values, pc, 1, HAV, Fs, design("linear", coords[1], pc))
    assert rel(pred, rp) < 1e-9 and np.max(np.abs(err ** 2 - rv)) < 1e-10
    assert rel(P.trend_coef, rb) < 1e-9 and rel(P.trend_cov, rc) < 1e-9
    # chunked: the same bits
    P.rhs_budget_bytes = 8 * 1024 * 1536
    pred_c, err_c = P.predict_arrays(1, np.vstack([pc] * 4))
    assert np.array_equal(pred_c[:400], pred) and np.array_equal(err_c[1200:], err)
    # a site with non-finite regressors gets NaN
    Q = _predictor(coords, values, BIV, trend=lambda k, c: np.column_stack([np.ones(len(c)), np.where(c[:, 0] > 52, np.nan,
                                                                                                       c[:, 0] / 10)]))
    pc = np.vstack([pc, [[55.0, -100.0], [53.0, -90.0]]])   # two sites beyond the covariate's coverage
    pq, eq = Q.predict_arrays(0, pc)
    nanrow = pc[:, 0] > 52
    assert nanrow.any() and np.all(np.isnan(pq[nanrow])) and np.all(np.isnan(eq[nanrow]))
    assert np.all(np.isfinite(pq[~nanrow]))
    # refusals
    with pytest.raises(NotImplementedError):
        P.predict_blocks(0, pc, np.zeros(len(pc), dtype=int))
    with pytest.raises(NotImplementedError):
        P.conditional_simulation(0, pc, 4)
    with pytest.raises(NotImplementedError):
        P.cross_validation(0)
    with pytest.raises(NotImplementedError):
        _predictor(coords, values, BIV, trend="constant", devices=[0, 0])
    P.close()
    Q.close()


def test_predictor_cv_ix_against_dense_loo(native):
    p, coords, values = make_data(15, BIV, HAV, n0=400, n1=380)
    P = _predictor(coords, values, BIV, trend="constant")
    ix = 17
    pred, err = P.predict_arrays(0, coords[0][ix], cv_ix=ix)
    c2 = [np.delete(coords[0], ix, axis=0), coords[1]]
    v2 = [np.delete(values[0], ix), values[1]]
    Fs = [np.ones((len(c), 1)) for c in c2]
    rp, rv, _, _ = dense_universal(p, c2, v2, coords[0][ix:ix + 1], 0, HAV, Fs, np.ones((1, 1)))
    assert abs(pred[0] - rp[0]) < 1e-9 * max(1.0, abs(rp[0])) and abs(err[0] ** 2 - rv[0]) < 1e-10
    P.close()


# ---- REML ---------------------------------------------------------------------------------------------------------------
def dense_reml(params, coords, values, metric, Fs):
    p = orc.Params.from_flat(params)
    S = orc.joint_cov(p, coords, metric)
    X = block_X(Fs)
    z = np.concatenate(values)
    cf = cho_factor(S, lower=True)
    A = X.T @ cho_solve(cf, X)
    b = X.T @ cho_solve(cf, z)
    _, ldS = np.linalg.slogdet(S)
    _, ldA = np.linalg.slogdet(A)
    quad = float(z @ cho_solve(cf, z) - b @ np.linalg.solve(A, b))
    N, q = X.shape
    return -0.5 * ((N - q) * np.log(2 * np.pi) + ldS + ldA + quad), ldS, ldA, quad


@pytest.mark.parametrize("params,metric,kind", [(BIV, HAV, "linear"), (BIV_EUC, EUC, "constant"), (UNI, HAV, "cov")])
def test_reml_value_and_gradient(native, params, metric, kind):
    p, coords, values = make_data(21, params, metric)
    Fs = [design(kind, c, c) for c in coords]
    h = handle(native, p, coords, values, metric, factor=False)
    for k in range(p.n_procs):
        h.set_trend(k, Fs[k])
    info, out4, g = h.loglik_reml(True)
    assert info == 0
    ref = dense_reml(params, coords, values, metric, Fs)
    for a, b in zip(out4, ref):
        assert abs(a - b) < 1e-8 * max(1.0, abs(b))
    info, out4v, _ = h.loglik_reml(False)
    assert abs(out4v[0] - out4[0]) < 1e-9 * abs(out4[0])
    x = np.asarray(params, dtype=float)
    nug = (3,) if x.size == 4 else (8, 9)
    for k in range(x.size):
        e = 1e-4 if k in nug else 1e-3 * max(abs(x[k]), 1.0)
        f = []
        for d in (-2, -1, 1, 2):
            y = x.copy()
            y[k] += d * e
            f.append(dense_reml(y, coords, values, metric, Fs)[0])
        fd = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * e)
        assert abs(g[k] - fd) < 1e-6 * max(1.0, abs(fd)), (k, g[k], fd)
    h.close()


def test_reml_without_trend_is_loglik(native):
    p, coords, values = make_data(23, BIV, HAV)
    h = handle(native, p, coords, values, HAV, factor=False)
    info, out3, g = h.loglik(True)
    h.assemble_joint()
    info2, out4, g2 = h.loglik_reml(True)
    assert info == info2 == 0
    assert out4[0] == out3[0] and out4[1] == out3[1] and out4[2] == 0.0 and out4[3] == out3[2]
    assert np.array_equal(g, g2)
    h.close()


def test_fit_likelihood_reml_univariate_matches_dense_scipy(native):
    from sif_xco2_cokriging_amd import fields, model
    truth = [1.1, 1.2, 380.0, 0.05]
    p, coords, values = make_data(17, truth, HAV, n0=400)
    mf = fields.MultiField([fields.Field(coords[0], values[0])])
    mod = model.MultivariateMatern(1)
    start = np.array([1.0, 1.5, 500.0, 0.02])
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params, trend="linear")
    assert mod.fit_result.method == "REML"
    bounds = mod.params.get_bounds()
    lo = np.array([b[0] for b in bounds])
    wd = np.array([b[1] - b[0] for b in bounds])
    Fs = [design("linear", coords[0], coords[0])]

    def cost(u):
        return -dense_reml(lo + wd * u, coords, values, HAV, Fs)[0]

    res = minimize(cost, (start - lo) / wd, method="L-BFGS-B", bounds=[(0.0, 1.0)] * 4,
                   options={"ftol": 1e-14, "gtol": 1e-9, "eps": 1e-9, "maxiter": 1000})
    assert mod.fit_result.loglik >= -res.fun - 1e-4
    assert abs(mod.fit_result.loglik - dense_reml(mod.params.get_values(), coords, values, HAV, Fs)[0]) < 1e-8 * abs(res.fun)


def test_fullsize_linear(native):
    """N = 40 000, "linear": equivariance and interpolation at sampled sites, and the no-trend bit check"""
    rng = np.random.default_rng(31)
    n = 20000
    pts = np.column_stack([rng.uniform(25, 50, n), rng.uniform(-120, -70, n)])
    coords = [pts, pts[rng.permutation(n)]]
    p = orc.Params.from_flat(BIV)
    values = [np.sin(coords[0][:, 0] / 3) + 0.01 * rng.standard_normal(n), np.cos(coords[1][:, 1] / 5)]
    h = handle(native, p, coords, values, HAV)
    pc = np.vstack([pred_sites(rng, HAV, 2000), coords[0][:200]])
    pred0, err0 = h.predict(0, pc)
    Fs = [design("linear", c, c) for c in coords]
    for k in range(2):
        h.set_trend(k, Fs[k])
    F0 = design("linear", coords[0], pc)
    pred, err, beta, _ = h.predict_universal(0, pc, F0)
    assert np.array_equal(h.predict(0, pc)[0], pred0)
    assert np.all(np.isfinite(pred)) and np.all(err ** 2 >= err0 ** 2 - 1e-12)
    gamma = np.array([1.0, -0.5, 0.25, 2.0, 0.1, -0.3])
    h2 = handle(native, p, coords, [values[0] + Fs[0] @ gamma[:3], values[1] + Fs[1] @ gamma[3:]], HAV)
    for k in range(2):
        h2.set_trend(k, Fs[k])
    pred2, err2, beta2, _ = h2.predict_universal(0, pc, F0)
    assert np.max(np.abs(pred2 - pred - F0 @ gamma[:3])) < 1e-7
    assert np.max(np.abs(beta2 - beta - gamma)) < 1e-7 and np.max(np.abs(err2 - err)) < 1e-9
    # data sites of process 0: c0 carries the nugget where h == 0, as Sigma does, so the predictor interpolates exactly
    # (lambda = e_j satisfies X^T lambda = x0 there): pred = z and pred_err = 0 to rounding
    assert np.max(np.abs(pred0[2000:] - values[0][:200])) < 1e-7
    assert np.max(np.abs(pred[2000:] - values[0][:200])) < 1e-7
    assert np.max(err[2000:]) < 1e-4
    h.close()
    h2.close()
