"""GPU tests of the Fisher information of the likelihood fit: include/cokrige.h ck_loglik_fisher, native.Handle.fisher and
model.MultivariateMatern.information / fit_likelihood(std_errors=True) against a dense numpy chain on the oracle's
covariances (tests/dense_chains.py: dense_fisher): D_k = dSigma/dtheta_k (nu and len by 4th-order central differences of
the block they enter, with the steps of tests/test_gpu_likelihood.py's fd_grad; sigma, rho, nugget and noise-scale derivatives
as exact block expressions) and I = 1/2 tr(S^-1 D_j S^-1 D_k) through cho_solve (REML: P formed densely).  One reference per
data set and module.  tests/test_gpu_newer_entry_edge_sizes.py runs the same reference over the size ladder."""
import warnings
from ctypes import byref, c_int64

import numpy as np
import pytest

from tests.dense_chains import dense_fisher as reference, normalised
from tests.test_gpu_likelihood import BIV, BIV_EUC, BIV_HALF, EUC, HAV, UNI, handle, make_data

pytestmark = pytest.mark.gpu

EXACT_BIV = [0, 1, 8, 9, 10, 11, 12]   # slots whose derivative is an exact block expression: sigma, nugget, rho, noise scales
EXACT_UNI = [0, 3, 11]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


_CASES = {}


def case(name, seed, params, metric, n0, n1):
    """data and ML reference of a named case, computed once"""
    if name not in _CASES:
        coords, values = make_data(seed, params, metric, n0=n0, n1=n1)
        _CASES[name] = (coords, values, reference(params, coords, metric))
    return _CASES[name]


def check_against(I, ref, exact):
    e = normalised(I, ref)
    print("largest normalised error", e.max(), "among exact derivatives", e[np.ix_(exact, exact)].max())
    assert e.max() <= 1e-6, e
    assert e[np.ix_(exact, exact)].max() <= 1e-9, e[np.ix_(exact, exact)]


SETS = {"BIV": (BIV, HAV), "BIV_EUC": (BIV_EUC, EUC), "UNI": (UNI, HAV), "BIV_HALF": (BIV_HALF, HAV)}
SIZES = [("BIV", 300, 333), ("BIV_EUC", 300, 333), ("UNI", 300, 333), ("BIV_HALF", 300, 333),
         ("BIV", 37, 50), ("BIV_EUC", 37, 50), ("UNI", 37, 50), ("BIV_HALF", 37, 50), ("BIV", 600, 570)]


@pytest.mark.parametrize("name,n0,n1", SIZES)
def test_against_reference(native, name, n0, n1):
    params, metric = SETS[name]
    coords, values, ref = case(f"{name}-{n0}-{n1}", 21, params, metric, n0, n1)
    h = handle(native, params, coords, values, metric)
    info, I = h.fisher()
    h.close()
    assert info == 0 and I.shape == (13, 13)
    check_against(I, ref, EXACT_UNI if len(params) == 4 else EXACT_BIV)
    dead = [k for k in range(13) if ref[k, k] == 0.0]   # slots that do not exist (and rho = 0: nu_12, len_12)
    assert np.all(I[dead] == 0.0) and np.all(I[:, dead] == 0.0)


def _trend_rows(kind, coords):
    from sif_xco2_cokriging_amd.trend import TrendDesign
    design = TrendDesign(kind, [np.asarray(c)[:, :2] for c in coords])
    F = [design.data(k, np.asarray(coords[k])[:, :2]) for k in range(len(coords))]
    p = sum(f.shape[1] for f in F)
    X = np.zeros((sum(len(c) for c in coords), p))
    r = c = 0
    for f in F:
        X[r:r + f.shape[0], c:c + f.shape[1]] = f
        r += f.shape[0]
        c += f.shape[1]
    return F, X


def test_scale_identity_ml_and_reml(native):
    """v = (sigma, 0 .., 2 nugget, 0): sum_k v_k D_k = 2 Sigma, so v^T I v = 2 N (ML) and 2 (N - p) (REML); no differencing"""
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    N = 633
    v = np.zeros(13)
    v[0], v[1], v[8], v[9] = BIV[0], BIV[1], 2 * BIV[8], 2 * BIV[9]
    h = handle(native, BIV, coords, values, HAV)
    info, I = h.fisher()
    assert info == 0
    print("ML  v^T I v / 2N - 1 =", v @ I @ v / (2 * N) - 1)
    assert abs(v @ I @ v - 2 * N) <= 1e-9 * 2 * N
    for kind in ("constant", "linear"):
        F, X = _trend_rows(kind, coords)
        for k in range(2):
            h.set_trend(k, F[k])
        info, I = h.fisher(reml=True)
        assert info == 0
        p = X.shape[1]
        print(kind, "REML v^T I v / 2(N - p) - 1 =", v @ I @ v / (2 * (N - p)) - 1)
        assert abs(v @ I @ v - 2 * (N - p)) <= 1e-9 * 2 * (N - p)
    h.close()


def test_reml_against_reference(native):
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    F, X = _trend_rows("linear", coords)
    ref = reference(BIV, coords, HAV, X=X)
    h = handle(native, BIV, coords, values, HAV)
    for k in range(2):
        h.set_trend(k, F[k])
    info, I = h.fisher(reml=True)
    h.close()
    assert info == 0
    check_against(I, ref, EXACT_BIV)


def test_structure(native):
    coords, values, ref = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    h = handle(native, BIV, coords, values, HAV)
    info, I = h.fisher()
    info2, I2 = h.fisher()
    h.close()
    assert info == 0 and info2 == 0
    assert np.array_equal(I, I.T)                       # symmetric to the bit
    assert np.array_equal(I, I2)                        # and reproducible
    live = np.flatnonzero(np.diag(I) > 0)
    assert list(live) == list(range(11))
    s = 1.0 / np.sqrt(np.diag(I)[live])
    w = np.linalg.eigvalsh(I[np.ix_(live, live)] * np.outer(s, s))
    print("smallest eigenvalue of the unit-diagonal scaling", w.min())
    assert w.min() >= -1e-12
    h0 = handle(native, BIV, coords, values, HAV, site_order=0)
    info0, I0 = h0.fisher()
    h0.close()
    assert info0 == 0
    d = np.sqrt(np.outer(np.diag(I), np.diag(I)))[np.ix_(live, live)]
    e = (np.abs(I - I0)[np.ix_(live, live)] / d).max()
    print("site orders differ by", e)
    assert e <= 1e-10


def test_mask(native):
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    h = handle(native, BIV, coords, values, HAV)
    info, I = h.fisher()
    free = np.zeros(13, dtype=bool)
    sub = [0, 3, 5, 8, 10]
    free[sub] = True
    info_m, Im = h.fisher(free=free)
    h.close()
    assert info == 0 and info_m == 0
    off = [k for k in range(13) if k not in sub]
    assert np.all(Im[off] == 0.0) and np.all(Im[:, off] == 0.0)
    d = np.sqrt(np.outer(np.diag(I), np.diag(I)))[np.ix_(sub, sub)]
    e = (np.abs(I - Im)[np.ix_(sub, sub)] / d).max()
    print("masked against full", e)
    assert e <= 1e-12


def test_product_groups(native):
    """too little room for all products: they are formed in groups, every pair still sums the same terms in the same order;
    not even two of them: refused with the amounts"""
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    h = handle(native, BIV, coords, values, HAV)
    info, I = h.fisher()
    assert info == 0 and h.fisher_timings()["groups"] == 1
    h.set_option("fisher_product_mb", 20)     # Npad = 1024: a cross product is 8 MiB, the others 3 and 6
    info, Ig = h.fisher()
    t = h.fisher_timings()
    assert info == 0 and t["groups"] > 2 and t["flop"] > 0
    assert np.array_equal(I, Ig)
    h.set_option("fisher_product_mb", 8)
    with pytest.raises(native.NativeError, match=r"needs \d+ bytes of device memory .* bytes are available"):
        h.fisher()
    h.close()


@pytest.mark.parametrize("which", [(0,), (0, 1)])
def test_noise_scales(native, which):
    coords, values, ref0 = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    rng = np.random.default_rng(5)
    noise = [rng.uniform(0.01, 0.1, len(coords[k])) if k in which else None for k in range(2)]
    scales = (1.7, 0.6)
    ref = reference(BIV, coords, HAV, noise=noise, scales=scales)
    h = handle(native, BIV, coords, values, HAV)
    info, I = h.fisher()
    assert info == 0 and np.all(I[11:] == 0.0) and np.all(I[:, 11:] == 0.0)   # without noise the s rows are 0
    for k in which:
        h.set_noise(k, noise[k], scales[k])
    h.assemble_joint()
    info, I = h.fisher()
    h.close()
    assert info == 0
    check_against(I, ref, EXACT_BIV)
    for k in range(2):
        assert (I[11 + k, 11 + k] > 0) == (k in which)


def test_rho_zero_not_identified(native):
    from sif_xco2_cokriging_amd import fields, model
    coords, values, ref = case("BIV_HALF-300-333", 21, BIV_HALF, HAV, 300, 333)
    h = handle(native, BIV_HALF, coords, values, HAV)
    info, I = h.fisher()
    h.close()
    assert info == 0
    for k in (3, 6):   # nu_12, len_12: their derivative is identically 0
        assert np.all(I[k] == 0.0) and np.all(I[:, k] == 0.0)
    mod = model.MultivariateMatern(2)
    mod.params.set_values(BIV_HALF)
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        inf = mod.information(mf)
    assert len(w) == 1 and "not identified" in str(w[0].message)
    assert inf.not_identified == ["nu_12", "len_scale_12"]
    assert np.isnan(inf.std_error["nu_12"]) and np.isnan(inf.std_error["len_scale_12"])
    keep = [k for k in range(11) if k not in (3, 6)]
    se_ref = np.sqrt(np.diag(np.linalg.inv(ref[np.ix_(keep, keep)])))
    se = inf.std_error.values[keep]
    print("standard errors against the reduced reference", np.max(np.abs(se / se_ref - 1)))
    assert np.max(np.abs(se / se_ref - 1)) <= 1e-5


def test_state_and_refusals(native):
    from tests.conftest import load_golden
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    grid = np.column_stack([np.linspace(26, 49, 120), np.linspace(-118, -72, 120)])
    h0 = handle(native, BIV, coords, values, HAV)
    assert h0.factor() == 0
    p0, e0 = h0.predict(1, grid)
    h0.close()
    h = handle(native, BIV, coords, values, HAV)
    r1 = h.loglik(True)
    info, I = h.fisher()
    assert info == 0
    with pytest.raises(native.NativeError, match="ck_loglik"):
        h.verify_model()                       # ck_loglik's state
    r2 = h.loglik(True)
    assert r1[1] == r2[1] and np.array_equal(r1[2], r2[2])
    info, I2 = h.fisher()
    assert np.array_equal(I, I2)
    p1, e1 = h.predict(1, grid)                # the factor stayed resident: the bits of a handle that never computed it
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1)
    out = np.empty((13, 13))
    inf = c_int64(0)
    with pytest.raises(native.NativeError, match="null argument"):
        native._chk(native.lib().ck_loglik_fisher(h._h, 0, None, None, byref(inf)))
    with pytest.raises(native.NativeError, match="null argument"):
        native._chk(native.lib().ck_loglik_fisher(h._h, 0, None, native._p(out), None))
    h.close()
    hu = native.Handle(0)                      # not assembled
    hu.set_model(2, BIV[0:2], BIV[2:5], BIV[5:8], BIV[8:10], BIV[10])
    hu.set_metric(HAV)
    for k in range(2):
        hu.set_data(k, coords[k], values[k])
    with pytest.raises(native.NativeError, match="ck_assemble_joint has not been called"):
        hu.fisher()
    hu.close()
    hp = native.Handle(devices=[0, 0], rank=0)   # partitioned
    with pytest.raises(native.NativeError, match="single-process form"):
        hp.fisher()
    hp.close()
    g = load_golden("joint_not_pd")
    hn = handle(native, list(g["params"]), [g["coords0"], g["coords1"]], [np.zeros(260), np.zeros(260)], HAV)
    info, In = hn.fisher()
    hn.close()
    assert info > 0 and np.all(np.isnan(In))


def test_fit_likelihood_std_errors(native):
    """the univariate case of test_fit_likelihood_univariate_matches_dense_scipy"""
    from sif_xco2_cokriging_amd import fields, model
    truth = [1.1, 1.2, 380.0, 0.05]
    coords, values = make_data(17, truth, HAV, n0=400)
    mf = fields.MultiField([fields.Field(coords[0], values[0])])
    start = np.array([1.0, 1.5, 500.0, 0.02])
    mod = model.MultivariateMatern(1)
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params)
    r = mod.fit_result
    assert r.information is None and r.std_error is None and r.at_bound is None and r.conf_int() is None
    mod.params.set_values(start)
    mod.fit_likelihood(mf, guess=mod.params, std_errors=True)
    r = mod.fit_result
    x = mod.params.get_values().astype(float)
    ref = reference(x, coords, HAV)[:4, :4]
    se_ref = np.sqrt(np.diag(np.linalg.inv(ref)))
    print("fitted", x, "standard errors", r.std_error.values, "reference", se_ref)
    assert r.at_bound == [] and list(r.std_error.index) == list(mod.params.get_names())
    assert np.max(np.abs(r.std_error.values / se_ref - 1)) <= 1e-5
    ci = r.conf_int(0.95)
    assert np.allclose(ci["lower"].values, x - 1.95996 * r.std_error.values, rtol=0, atol=1e-5 * np.abs(r.std_error.values))
    assert np.allclose(ci["upper"].values, x + 1.95996 * r.std_error.values, rtol=0, atol=1e-5 * np.abs(r.std_error.values))
    mod.params.set_values(start)
    mod.params.set_bounds(nugget=(0.1, 0.2))           # the nugget ends on its lower bound
    mod.params.set_values([1.0, 1.5, 500.0, 0.15])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mod.fit_likelihood(mf, guess=mod.params, std_errors=True)
    r = mod.fit_result
    assert r.at_bound == ["nugget_11"] and np.isnan(r.std_error["nugget_11"])
    assert sum("ended on a bound" in str(x.message) for x in w) == 1
    assert np.all(np.isfinite(r.std_error.values[:3]))
    x = mod.params.get_values().astype(float)
    ref3 = reference(x, coords, HAV)[:3, :3]
    assert np.max(np.abs(r.std_error.values[:3] / np.sqrt(np.diag(np.linalg.inv(ref3))) - 1)) <= 1e-5


def test_nothing_of_a_sweep_stays_on_the_handle(native):
    """Fisher REML -> loglik_reml with gradient -> Fisher ML -> loglik with gradient -> Fisher REML on ONE handle: every result
    (and loglik_noise_grad behind each gradient) has the bits of the same call on a fresh handle.  BIV-300-333 with a
    two-column trend: Npad = 1024, two panels, the process boundary off every tile edge; noise on process 0, so that the noise
    scores are not identically zero"""
    coords, values, _ = case("BIV-300-333", 21, BIV, HAV, 300, 333)
    F, X = _trend_rows("constant", coords)
    assert X.shape[1] == 2
    noise = np.random.default_rng(5).uniform(0.01, 0.1, len(coords[0]))

    def fresh():
        h = handle(native, BIV, coords, values, HAV)
        for k in range(2):
            h.set_trend(k, F[k])
        h.set_noise(0, noise, 1.7)
        h.assemble_joint()
        return h

    def grad_call(reml):
        def call(h):
            r = h.loglik_reml(True) if reml else h.loglik(True)
            return r[0], tuple(r[1]), r[2], h.loglik_noise_grad()
        return call

    steps = [("fisher reml", lambda h: h.fisher(reml=True)), ("loglik_reml grad", grad_call(True)),
             ("fisher ml", lambda h: h.fisher()), ("loglik grad", grad_call(False)), ("fisher reml again", lambda h: h.fisher(reml=True))]

    def flat(r):
        return np.concatenate([np.atleast_1d(np.asarray(x, dtype=float)).ravel() for x in r])

    h = fresh()
    for name, step in steps:
        got = flat(step(h))
        f = fresh()
        want = flat(step(f))
        f.close()
        assert np.all(np.isfinite(got)), name
        assert got.tobytes() == want.tobytes(), name
    h.close()
