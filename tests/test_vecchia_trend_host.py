"""The Vecchia likelihood with a GLS trend without a GPU: the numpy loop of tests/vecchia_trend_ref.py against dense GLS under
full conditioning, the envelope theorem and the invariance z -> z + X gamma; the row arithmetic of csrc/ck_vecchia_trend.h, the
fixed-order Gram matrix and the host GLS step compiled with g++ (tests/host_vecchia_trend_shim.cpp) against that loop; the
validation of Vecchia(trend=..., trend_likelihood=...) and the refusals of the Python layer, all before any device work; the same
host code in a stand-alone program under -fsanitize=address,undefined (tests/host_vecchia_trend_sanitize_main.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)

from tests import vecchia_ref as vr           # noqa: E402
from tests import vecchia_trend_ref as vtr    # noqa: E402

EUC = 1
GAMMA = np.array([0.7, -0.4, 0.25, -1.1, 0.3, 0.5])   # the known trend added to the values ("linear": p = 6)


@pytest.fixture(scope="module")
def problem():
    """150 + 110 sites of half_colocated_sites(150) on the unit square, SET_B_UNIT, a linear trend added to the values"""
    from sif_xco2_cokriging_amd import synth
    coords, values = vr.half_colocated_sites(150)
    coords, values = [coords[0], coords[1][:110]], [values[0], values[1][:110]]
    X, F = vtr.design("linear", coords)
    zt = np.concatenate(values) + X @ GAMMA
    return dict(coords=coords, values=[zt[:150], zt[150:]], plain=values, params=list(synth.SET_B_UNIT), X=X, F=F,
                ranks=np.random.default_rng(11).permutation(260))


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_equals_dense_gls_under_full_conditioning(problem):
    pb = problem
    ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], pb["X"], EUC, pb["ranks"], 10.0)
    dense = vtr.dense_gls(pb["params"], pb["coords"], pb["values"], pb["X"], EUC)
    assert ref["k_max"] == 259 and ref["n_empty"] == 1
    for key in ("out5", "out5_reml"):
        assert np.allclose(ref[key], dense[key], rtol=1e-11, atol=0), (key, ref[key], dense[key])
    assert np.allclose(ref["beta"], dense["beta"], rtol=1e-10, atol=1e-12)
    assert np.allclose(ref["cov"], dense["cov"], rtol=1e-10, atol=1e-14)
    assert np.allclose(ref["A"], dense["A"], rtol=1e-11) and np.allclose(ref["b"], dense["b"], rtol=1e-11, atol=1e-11)


def test_reference_invariance_and_envelope(problem):
    pb = problem
    caps = (8, 8)
    ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], pb["X"], EUC, pb["ranks"], 0.5, caps)
    plain = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["plain"], pb["X"], EUC, pb["ranks"], 0.5, caps)
    for k in (0, 1, 3):                                            # z -> z + X gamma: the value stays, beta moves by gamma
        assert abs(ref["out5"][k] - plain["out5"][k]) <= 1e-9 * abs(ref["out5"][k])
    assert np.allclose(ref["beta"] - plain["beta"], GAMMA, rtol=0, atol=1e-10)
    assert np.linalg.cond(ref["A"]) < 50
    zero_mean = vr.vecchia_reference(pb["params"], pb["coords"], pb["values"], EUC, pb["ranks"], 0.5, caps)
    assert ref["out5"][0] > zero_mean["out3"][0] + 10.0            # the trend is in the data: the zero-mean value is far below
    # the envelope theorem: d l_P / d theta = the derivative of the plain Vecchia value of the residual at fixed beta-hat
    resid = np.concatenate(pb["values"]) - pb["X"] @ ref["beta"]
    rv = [resid[:150], resid[150:]]
    x0 = np.array(pb["params"], dtype=float)
    for k in (0, 5, 8, 10):
        e = 1e-5 * max(abs(x0[k]), 1.0)
        d_prof, d_res = [], []
        for sgn in (1.0, -1.0):
            x = x0.copy()
            x[k] += sgn * e
            d_prof.append(vtr.profile_value(x, pb["coords"], pb["values"], pb["X"], EUC, ref["keep"]))
            d_res.append(vr.vecchia_reference(x, pb["coords"], rv, EUC, pb["ranks"], 0.5, caps,
                                              sets=(ref["keep"], ref["gap"], None))["out3"][0])
        g_prof, g_res = (d_prof[0] - d_prof[1]) / (2 * e), (d_res[0] - d_res[1]) / (2 * e)
        assert abs(g_prof - g_res) <= 1e-6 * max(abs(g_res), 1.0), (k, g_prof, g_res)


# ---------------------------------------------------------------------------------------------------------------------
# the header on the host
# ---------------------------------------------------------------------------------------------------------------------
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vecchia_trend") / "libck_vecchia_trend.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "tests", "host_vecchia_trend_shim.cpp"), os.path.join(CSRC, "ck_host.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.shim_vecchia_trend_row.argtypes = [ctypes.c_double] * 5 + [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp]
    lib.shim_vecchia_trend_row.restype = ctypes.c_int
    lib.shim_vecchia_trend_gram.argtypes = [ctypes.c_long, ctypes.c_int, _dp, _dp]
    lib.shim_vecchia_trend_gram.restype = None
    lib.shim_vecchia_trend_fit.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp,
                                           ctypes.c_double, _dp, _dp, _dp, _dp, _dp]
    lib.shim_vecchia_trend_fit.restype = ctypes.c_longlong
    return lib


def test_one_row(shim):
    x, g = np.array([1.0, 0.5, -2.0]), np.array([0.25, 0.125, 1.0])
    out4, row = np.zeros(4), np.zeros(4)
    rc = shim.shim_vecchia_trend_row(0.7, 0.2, 0.4, 1.02, 0.3, 5, 3, _d(x), _d(g), _d(out4), _d(row))
    s2 = (1.02 + 0.3) - 0.4
    assert rc == 0 and out4[0] == 0.2 and out4[1] == s2
    assert np.allclose(row, np.r_[0.5, x - g] / np.sqrt(s2), rtol=1e-15, atol=0)
    rc = shim.shim_vecchia_trend_row(0.7, np.nan, np.nan, 1.02, 0.0, 0, 3, _d(x), _d(np.full(3, np.nan)), _d(out4), _d(row))
    assert rc == 0 and np.allclose(row, np.r_[0.7, x] / np.sqrt(1.02), rtol=1e-15, atol=0)   # an empty set: (z, x) / s
    for mu, vv in ((0.2, 1.02), (0.2, 1.5), (np.nan, 0.1), (0.2, np.nan)):                   # no term: nothing for G
        row[:] = 7.0
        rc = shim.shim_vecchia_trend_row(0.7, mu, vv, 1.02, 0.0, 3, 3, _d(x), _d(g), _d(out4), _d(row))
        assert rc == 1 and np.all(row == 0.0) and np.isnan(out4[2])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 65537])
@pytest.mark.parametrize("p", [0, 2, 6, 16])
def test_fixed_order_gram_matrix_against_numpy(shim, n, p):
    rows = np.random.default_rng(n + p).standard_normal((n, p + 1))
    tri, again = np.full(156, np.nan), np.full(156, np.nan)
    shim.shim_vecchia_trend_gram(n, p, _d(rows), _d(tri))
    shim.shim_vecchia_trend_gram(n, p, _d(rows), _d(again))
    G = rows.T @ rows
    got = np.zeros_like(G)
    got[np.tril_indices(p + 1)] = tri[:(p + 1) * (p + 2) // 2]     # rows first: (0,0) (1,0) (1,1) (2,0) ..
    assert np.allclose(got, np.tril(G), rtol=1e-12, atol=1e-12 * n)
    assert np.all(tri[(p + 1) * (p + 2) // 2:] == 0.0) and np.array_equal(tri, again)


def host_fit(shim, ref, reml, tol=1e-10, X=None, mu=None, vv=None):
    """the host pipeline on the reference's per-datum solves (mu_t, v . v, g_t)"""
    N, p = len(ref["z"]), ref["p"]
    X = np.ascontiguousarray(ref["X"] if X is None else X)
    prior = np.ascontiguousarray(ref["prior"])
    mu = np.ascontiguousarray(ref["mean"] if mu is None else mu)
    vv = np.ascontiguousarray(prior - ref["var"] if vv is None else vv)
    cnt = np.ascontiguousarray(ref["count"], dtype=np.int32)
    g = np.ascontiguousarray(ref["g"])
    out5, beta, cov, mean, var = np.zeros(5), np.zeros(p), np.zeros((p, p)), np.zeros(N), np.zeros(N)
    rc = shim.shim_vecchia_trend_fit(N, p, int(reml), _d(ref["z"]), _d(mu), _d(vv), _d(prior), None, cnt.ctypes.data_as(_ip),
                                     _d(X), _d(g), tol, _d(out5), _d(beta), _d(cov), _d(mean), _d(var))
    return rc, out5, beta, cov, mean, var


@pytest.mark.parametrize("caps", [(8, 8), (32, 32)])
def test_host_pipeline_against_the_numpy_loop(shim, problem, caps):
    pb = problem
    ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], pb["X"], EUC, pb["ranks"], 0.5, caps)
    S = vtr.joint_cov(pb["params"], pb["coords"], EUC)
    ref["prior"] = np.diag(S).copy()
    for reml in (False, True):
        rc, out5, beta, cov, mean, var = host_fit(shim, ref, reml)
        want = ref["out5_reml" if reml else "out5"]
        assert rc == 0
        assert np.allclose(out5, want, rtol=1e-11, atol=1e-11), (out5, want)
        assert np.allclose(beta, ref["beta"], rtol=1e-9, atol=1e-11) and np.allclose(cov, ref["cov"], rtol=1e-9, atol=1e-13)
        assert np.allclose(mean, ref["mean_trend"], rtol=1e-10, atol=1e-11)
        assert np.allclose(var, ref["var"], rtol=1e-12, atol=0)
    assert out5[0] != host_fit(shim, ref, False)[1][0]             # REML is another number
    # a repeated column is refused, naming it (1-based, negated)
    Xd = pb["X"].copy()
    Xd[:, 4] = Xd[:, 3]
    rd = dict(ref, X=Xd, g=ref["g"].copy())
    rd["g"][:, 4] = rd["g"][:, 3]
    assert host_fit(shim, rd, False)[0] == -5
    # a datum without a term: NaN in out5, beta and cov, and it is named
    vv = ref["prior"] - ref["var"]
    vv[77] = ref["prior"][77] + 1.0
    rc, out5, beta, cov, _, _ = host_fit(shim, ref, False, vv=vv)
    assert rc == 78 and np.all(np.isnan(out5)) and np.all(np.isnan(beta)) and np.all(np.isnan(cov))


def test_host_pipeline_without_a_trend_is_the_plain_likelihood(shim, problem):
    pb = problem
    ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], np.zeros((260, 0)), EUC, pb["ranks"], 0.5, (8, 8))
    ref["prior"] = np.diag(vtr.joint_cov(pb["params"], pb["coords"], EUC)).copy()
    for reml in (False, True):
        rc, out5, *_ = host_fit(shim, ref, reml)
        assert rc == 0 and out5[2] == 0.0 and out5[3] == out5[4]
        assert np.allclose(out5[[0, 1, 3]], ref["out3"], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# the configuration and the Python layer's refusals: no device work
# ---------------------------------------------------------------------------------------------------------------------
def test_trend_configuration_is_validated_in_the_constructor():
    from sif_xco2_cokriging_amd import vecchia
    v = vecchia.Vecchia(0.5)
    assert v.trend is None and v.trend_likelihood == "profile" and not v.reml           # the defaults: as before
    assert not vecchia.Vecchia(0.5, trend_likelihood="reml").reml                       # no trend: nothing to restrict
    for t in ("constant", "linear", lambda k, c: np.ones((len(c), 1))):
        v = vecchia.Vecchia(0.5, trend=t)
        assert v.trend is t and not v.reml
        assert vecchia.Vecchia(0.5, trend=t, trend_likelihood="reml").reml
    for bad in ("quadratic", 1, 0.5, ["constant"], True):
        with pytest.raises(ValueError, match="trend must be None, 'constant', 'linear' or a callable"):
            vecchia.Vecchia(0.5, trend=bad)
    for bad in ("ml", "REML", None, 1, True):
        with pytest.raises(ValueError, match="trend_likelihood must be one of"):
            vecchia.Vecchia(0.5, trend="constant", trend_likelihood=bad)


def _model_and_fields():
    from sif_xco2_cokriging_amd import fields, model
    rng = np.random.default_rng(2)
    c = np.column_stack([rng.uniform(25, 50, 20), rng.uniform(-120, -70, 20)])
    mf = fields.MultiField([fields.Field(c, rng.standard_normal(20)) for _ in range(2)])
    return model.MultivariateMatern(2), mf


def test_python_refusals_need_no_device():
    from sif_xco2_cokriging_amd import vecchia
    mod, mf = _model_and_fields()
    v = vecchia.Vecchia(300.0, max_neighbours=8)                    # the default configuration refuses as before
    for call in (mod.log_likelihood, mod.fit_likelihood, mod.information):
        with pytest.raises(ValueError, match=r"REML.*Vecchia\(trend="):
            call(mf, vecchia=v, trend="constant")
    with pytest.raises(NotImplementedError, match="no analytic gradient yet"):
        mod.log_likelihood(mf, vecchia=v, gradient=True)
    with pytest.raises(NotImplementedError, match="Fisher information"):
        mod.fit_likelihood(mf, vecchia=v, std_errors=True)
    vt = vecchia.Vecchia(300.0, max_neighbours=8, trend="constant")
    with pytest.raises(ValueError, match=r"REML.*Vecchia\(trend="):
        mod.log_likelihood(mf, vecchia=vt, trend="constant")       # the keyword stays refused next to vecchia=
    with pytest.raises(NotImplementedError, match="no analytic gradient yet"):
        mod.log_likelihood(mf, vecchia=vt, gradient=True)          # gradient="numeric": the fit differences the value
    with pytest.raises(NotImplementedError, match="Fisher information"):
        mod.fit_likelihood(mf, vecchia=vt, std_errors=True)        # information="none"
    vr_ = vecchia.Vecchia(300.0, max_neighbours=8, trend="constant", trend_likelihood="reml", gradient="analytic",
                          information="expected")
    with pytest.raises(NotImplementedError, match=r"REML.*numeric route"):
        mod.log_likelihood(mf, vecchia=vr_, gradient=True)
    with pytest.raises(NotImplementedError, match=r"REML.*profile"):
        mod.information(mf, vecchia=vr_)
    with pytest.raises(NotImplementedError, match=r"REML.*profile"):
        mod.fit_likelihood(mf, vecchia=vr_, std_errors=True)
    assert mod._lik is None                                         # no handle was made


def test_abi_declares_the_trend_entry_points():
    from sif_xco2_cokriging_amd import native
    header = open(os.path.join(ROOT, "include", "cokrige.h")).read()
    for name in ("ck_loglik_vecchia_trend", "ck_loglik_vecchia_trend_grad", "ck_debug_vecchia_trend"):
        assert name in native.exported_names() and f"int {name}(" in header


def test_host_code_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_vecchia_trend_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "host_vecchia_trend_sanitize_main.cpp"), os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
