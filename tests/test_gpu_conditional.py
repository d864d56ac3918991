"""GPU tests of conditional simulation: include/cokrige.h ck_conditional_draws, native.Handle.conditional_draws and
joint_prediction.Predictor.conditional_simulation against a dense numpy chain (oracle covariances, the same deflation mask,
numpy.linalg.cholesky in the library's site order), the device's noise, and the state the call leaves on the handle."""
import os

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def make_data(rng, params, n_per=700):
    p = orc.Params.from_flat(params)
    pts = np.column_stack([rng.uniform(25, 50, 2 * n_per), rng.uniform(-120, -70, 2 * n_per)])
    coords = [pts[:n_per], pts[n_per // 2:n_per // 2 + n_per]]
    S = orc.joint_cov(p, coords, HAV)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
    return p, coords, [z[:n_per], z[n_per:]]


def handle(native, p, coords, values, metric, site_order=None):
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
    if site_order is not None:
        h.set_option("site_order", site_order)
    h.assemble_joint()
    assert h.factor() == 0
    return h


def posterior(p, coords, values, pc, i, metric):
    """pred and S = C_pp - c0^T Sigma^-1 c0 (src/joint_prediction.py:60-78 with the full m x m matrix)"""
    cf = cho_factor(orc.joint_cov(p, coords, metric), lower=True)
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    pred = c0.T @ cho_solve(cf, np.concatenate(values))
    return pred, orc.pred_cov(p, pc, i, metric) - c0.T @ cho_solve(cf, c0)


def internal_order(native, pc, site_order):
    return native.hilbert_order(pc) if site_order and len(pc) >= 256 else np.arange(len(pc))


def chain_factor(S, defl, perm, jitter_abs=0.0):
    """the Cholesky of S without the deflated sites, in the library's order: (kept sites in that order, L)"""
    kept = perm[~defl[perm]]
    return kept, np.linalg.cholesky(S[np.ix_(kept, kept)] + jitter_abs * np.eye(len(kept)))


def chain_draws(pred, S, defl, perm, eps, jitter_abs=0.0):
    kept, L = chain_factor(S, defl, perm, jitter_abs)
    x = np.zeros_like(eps)
    x[:, kept] = eps[:, kept] @ L.T
    return pred + x


def biv_case(native, rng, i, m=600):
    """m sites of process i: 20 on data of process i, 10 on data of the other process only, the rest random"""
    p, coords, values = make_data(rng, BIV)
    mine = coords[i][rng.choice(len(coords[i]), 20, replace=False)]
    other_only = np.array([c for c in coords[1 - i] if not (coords[i] == c).all(axis=1).any()])
    other = other_only[rng.choice(len(other_only), 10, replace=False)]
    pc = np.vstack([np.column_stack([rng.uniform(26, 49, m - 30), rng.uniform(-118, -72, m - 30)]), mine, other])
    perm = rng.permutation(m)
    pc = pc[perm]
    on_mine = np.zeros(m, dtype=bool)
    on_mine[np.argsort(perm)[m - 30:m - 10]] = True
    return p, coords, values, pc, on_mine


@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("i", [0, 1])
def test_given_noise_matches_the_dense_chain(native, i, site_order):
    rng = np.random.default_rng(100 + 10 * i + site_order)
    p, coords, values, pc, on_mine = biv_case(native, rng, i)
    m = len(pc)
    h = handle(native, p, coords, values, HAV, site_order)
    p0, e0 = h.predict(i, pc)
    eps = rng.standard_normal((7, m))
    draws, pred, err, defl, info = h.conditional_draws(i, pc, 7, noise=eps)
    assert info == 0
    assert np.array_equal(pred, p0) and np.array_equal(err, e0)
    assert np.array_equal(defl, on_mine)
    assert np.array_equal(draws[:, defl], np.broadcast_to(pred[defl], (7, int(defl.sum()))))
    rp, S = posterior(p, coords, values, pc, i, HAV)
    want = chain_draws(pred, S, defl, internal_order(native, pc, site_order), eps)
    assert rel(draws, want) < 1e-8
    t = h.draws_timings()
    assert t["n_deflated"] == 20 and t["n_chunks"] == 1 and t["product_ms"] > 0
    h.close()


def test_kat_simulation_experiment(native):
    """the reference's simulation experiment: nugget 0, process 1 on 2 601 grid sites, 100 of them data sites of process 1"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "kat_simulation_experiment.npz"))
    p = orc.Params.from_flat(g["params"])
    coords, values = [g["coords0"], g["coords1"]], [g["values0"], g["values1"]]
    pc = g["pcoords"]
    h = handle(native, p, coords, values, EUC)
    eps = np.random.default_rng(3).standard_normal((5, len(pc)))
    draws, pred, err, defl, info = h.conditional_draws(1, pc, 5, noise=eps)
    assert info == 0
    on_data = np.array([(coords[1] == c).all(axis=1).any() for c in pc])
    assert on_data.sum() == 100 and np.array_equal(defl, on_data)
    assert np.array_equal(draws[:, defl], np.broadcast_to(pred[defl], (5, 100)))
    z1 = {tuple(c): v for c, v in zip(coords[1], values[1])}
    assert np.max(np.abs(pred[defl] - np.array([z1[tuple(c)] for c in pc[defl]]))) < 1e-6
    rp, S = posterior(p, coords, values, pc, 1, EUC)
    want = chain_draws(rp, S, defl, internal_order(native, pc, 1), eps)
    assert rel(draws[:, ~defl], want[:, ~defl]) < 1e-6
    h.close()


def test_zero_noise_determinism_and_prefix(native):
    rng = np.random.default_rng(5)
    p, coords, values, pc, _ = biv_case(native, rng, 0, m=700)
    h = handle(native, p, coords, values, HAV)
    m = len(pc)
    d0, pred, _, h_defl, _ = h.conditional_draws(0, pc, 3, noise=np.zeros((3, m)))
    assert h_defl.sum() == 20
    assert np.array_equal(d0, np.broadcast_to(pred, (3, m)))
    a = h.conditional_draws(0, pc, 300, seed=77)[0]
    b = h.conditional_draws(0, pc, 300, seed=77)[0]
    assert np.array_equal(a, b)
    for chunk in (1, 100, 129, 256):
        h.set_option("draw_chunk", chunk)
        c = h.conditional_draws(0, pc, 300, seed=77)[0]
        assert np.array_equal(a, c), chunk
        assert h.draws_timings()["n_chunks"] == -(-300 // chunk)
    h.set_option("draw_chunk", 0)
    assert np.array_equal(h.conditional_draws(0, pc, 10, seed=77)[0], a[:10])
    assert not np.array_equal(h.conditional_draws(0, pc, 10, seed=78)[0], a[:10])
    h.close()
    # the device's normals are those of csrc/ck_rng.h on the host, keyed on the caller's site index whatever the library's
    # order (Hilbert here): draws from the host shim's noise through the dense chain
    import ctypes
    import subprocess
    so = os.path.join(ROOT, "tests", "_build", "libck_host_rng_gpu.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_rng_shim.cpp"), "-o", so], check=True)
    eps = np.empty((300, m))
    ctypes.CDLL(so).shim_normals(ctypes.c_uint64(77), ctypes.c_long(m), ctypes.c_long(300),
                                 eps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    defl = h_defl
    rp, S = posterior(p, coords, values, pc, 0, HAV)
    want = chain_draws(pred, S, defl, internal_order(native, pc, 1), np.where(defl, 0.0, eps))
    assert rel(a, want) < 1e-8


def test_device_noise_statistics(native):
    rng = np.random.default_rng(6)
    p, coords, values = make_data(rng, BIV, n_per=500)
    pc = np.column_stack([rng.uniform(26, 49, 300), rng.uniform(-118, -72, 300)])
    h = handle(native, p, coords, values, HAV)
    n = 20000
    draws, pred, err, defl, info = h.conditional_draws(1, pc, n, seed=2024)
    assert info == 0 and not defl.any()
    rp, S = posterior(p, coords, values, pc, 1, HAV)
    kept, L = chain_factor(S, defl, internal_order(native, pc, 1))
    w = solve_triangular(L, (draws - pred)[:, kept].T, lower=True).ravel()
    N = w.size
    assert abs(w.mean()) < 2.576 / np.sqrt(N)
    assert abs(w.var() - 1.0) < 2.576 * np.sqrt(2.0 / N) + 1e-6
    from scipy.stats import kstest
    assert kstest(w, "norm").statistic < 1.628 / np.sqrt(N)
    # the empirical covariance of 20 random block means against predict_blocks' A S A^T
    lab = rng.integers(0, 20, 300)
    wgt = rng.uniform(0.5, 1.5, 300)
    _, _, cov = h.predict_blocks(1, pc, lab.astype(np.int32), wgt, 20, want_cov=True)
    A = np.zeros((20, 300))
    A[lab, np.arange(300)] = wgt
    y = (draws - pred) @ A.T
    emp = y.T @ y / n
    # E |emp - C|_F^2 = ((tr C)^2 + |C|_F^2) / n for Gaussian draws: 3 sqrt(2 / n) relative when the blocks are strongly
    # correlated ((tr C)^2 ~ |C|_F^2), larger for 20 nearly independent blocks -- three standard deviations either way
    sd = np.sqrt((np.trace(cov) ** 2 + np.linalg.norm(cov) ** 2) / n) / np.linalg.norm(cov)
    assert np.linalg.norm(emp - cov) / np.linalg.norm(cov) <= max(3 * np.sqrt(2.0 / n), 3 * sd)
    h.close()


def test_state_duplicates_and_refusals(native):
    rng = np.random.default_rng(9)
    p, coords, values = make_data(rng, BIV, n_per=500)
    pc = np.column_stack([rng.uniform(26, 49, 300), rng.uniform(-118, -72, 300)])
    h = handle(native, p, coords, values, HAV)
    p0, e0 = h.predict(0, pc)
    v0 = h.verify_model()
    h.conditional_draws(0, pc, 50, seed=1)
    assert h.verify_model() == v0
    p1, e1 = h.predict(0, pc)
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1)
    # duplicates at the C level: info names one of the pair (the later in the library's order), draws are left untouched
    pcd = np.vstack([pc, pc[[17]]])
    draws, pred, err, defl, info = h.conditional_draws(0, pcd, 4, seed=1)
    assert info in (18, 301) and not draws.any()
    assert rel(pred[:300], p0) < 1e-12
    # refusals leave the handle usable
    for kw, msg in [({"tol": -1.0}, "tol"), ({"jitter": -1e-3}, "jitter")]:
        with pytest.raises(native.NativeError, match=msg):
            h.conditional_draws(0, pc, 2, **kw)
    with pytest.raises(native.NativeError, match="65 536"):
        h.conditional_draws(0, np.column_stack([np.linspace(26, 49, 65537), np.linspace(-118, -72, 65537)]), 1)
    with pytest.raises(native.NativeError, match="n_draws"):
        h.conditional_draws(0, pc, 0)
    p2, e2 = h.predict(0, pc)
    assert np.array_equal(p0, p2) and h.verify_model() == v0
    h.close()
    u = native.Handle(0)
    u.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    for k in range(2):
        u.set_data(k, coords[k], values[k])
    u.assemble_joint()
    with pytest.raises(native.NativeError, match="ck_factor"):
        u.conditional_draws(0, pc, 2)
    assert u.factor() == 0
    assert u.conditional_draws(0, pc, 2, seed=3)[4] == 0
    u.close()
    q = native.Handle(devices=[0, 0], rank=0)
    with pytest.raises(native.NativeError, match="partitioned"):
        q.conditional_draws(0, pc, 2)
    q.close()


class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


class _StubTrend:
    def predict(self, X):
        X = np.asarray(X, dtype=float)
        return 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.05


def test_predictor_surface(native):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    rng = np.random.default_rng(12)
    p, coords, values = make_data(rng, BIV, n_per=500)
    at = dict(scale_fact=1.7, spatial_mean=0.25, temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
              covariate_scales=[12.0, 6.0], spatial_model=_StubTrend())
    f0, f1 = fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])
    for f in (f0, f1):
        f.ds = _Attrs(at)
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    P = joint_prediction.Predictor(mod, fields.MultiField([f0, f1]))
    pc = np.vstack([np.column_stack([rng.uniform(26, 49, 300), rng.uniform(-118, -72, 300)]), coords[1][:5]])
    pcd = np.vstack([pc, pc[[3, 302]]])          # a duplicated site and a duplicated data site
    draws, pred, err, defl, seed = P.conditional_draws_arrays(1, pcd, 40, seed=11)
    assert seed == 11 and defl[300:305].all() and defl[306] and not defl[:300].any()
    assert np.array_equal(draws[:, 305], draws[:, 3]) and np.array_equal(draws[:, 306], draws[:, 302])
    pp, ee = P.predict_arrays(1, pc)
    assert rel(pred[:305], pp) < 1e-12
    raw = P.conditional_simulation(1, pc, 40, seed=11, postprocess=False)
    out = P.conditional_simulation(1, pc, 40, seed=11, postprocess=True)
    if joint_prediction.xr is None:
        (df_raw, d_raw), (df, d) = raw, out
        assert df.attrs == {"seed": 11, "n_deflated": 5, "jitter": 0.0}
        assert d.shape == (40, 305) and np.array_equal(d_raw, draws[:, :305])
        assert np.allclose(d - df["pred"].values, 1.7 * (d_raw - df_raw["pred"].values), rtol=0, atol=1e-12)
    else:
        assert out["draws"].dims[0] == "draw" and out.attrs["n_deflated"] == 5 and out.attrs["seed"] == 11
        dd = (out["draws"] - out["pred"]).values
        rr = (raw["draws"] - raw["pred"]).values
        assert np.allclose(dd, 1.7 * rr, rtol=0, atol=1e-12, equal_nan=True)
    P.close()
    Q = joint_prediction.Predictor(mod, fields.MultiField([f0, f1]), devices=[0])
    dq = Q.conditional_draws_arrays(1, pcd, 40, seed=11)[0]
    assert np.array_equal(dq, draws)
    Q.close()
