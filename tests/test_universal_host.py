"""Host side of universal cokriging, without a GPU: the trend designs of Predictor(trend=...) / log_likelihood(trend=...)
(sif_xco2_cokriging_amd/trend.py) and the p x p GLS step of the library (csrc/ck_host.cpp: ck_host_gls) compiled for the
host with g++ (tests/host_gls_shim.cpp) and checked against numpy."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gls") / "libck_host_gls.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_gls_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.shim_gls.argtypes = [ctypes.c_int, dp, dp, ctypes.c_double, dp, dp, dp, dp, dp]
    lib.shim_gls.restype = ctypes.c_int
    return lib


def gls(lib, A, b, tol=1e-10):
    p = len(b)
    A, b = np.ascontiguousarray(A, dtype=float), np.ascontiguousarray(b, dtype=float)
    R, beta, Ai = np.zeros((p, p)), np.zeros(p), np.zeros((p, p))
    ld, q = ctypes.c_double(), ctypes.c_double()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.shim_gls(p, A.ctypes.data_as(dp), b.ctypes.data_as(dp), tol, R.ctypes.data_as(dp), beta.ctypes.data_as(dp),
                      Ai.ctypes.data_as(dp), ctypes.byref(ld), ctypes.byref(q))
    return rc, R, beta, Ai, ld.value, q.value


@pytest.mark.parametrize("p", [1, 2, 6, 16])
def test_gls_against_numpy(shim, p):
    rng = np.random.default_rng(p)
    X = rng.standard_normal((50, p))
    A = X.T @ X + 0.1 * np.eye(p)
    b = rng.standard_normal(p)
    rc, R, beta, Ai, ld, q = gls(shim, A, b)
    assert rc == 0
    assert np.allclose(R @ R.T, A, rtol=1e-13, atol=1e-12) and np.allclose(np.triu(R, 1), 0)
    assert np.allclose(beta, np.linalg.solve(A, b), rtol=1e-11)
    assert np.allclose(Ai, np.linalg.inv(A), rtol=1e-11, atol=1e-13) and np.array_equal(Ai, Ai.T)
    assert abs(ld - np.linalg.slogdet(A)[1]) < 1e-12 * max(1, abs(ld))
    assert abs(q - b @ np.linalg.solve(A, b)) < 1e-12 * max(1, abs(q))


def test_gls_refuses_rank_deficient(shim):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 3))
    X = np.column_stack([X, X[:, 1]])             # column 3 repeats column 1
    rc = gls(shim, X.T @ X, np.ones(4))[0]
    assert rc == 4
    X = np.column_stack([np.ones(30), np.ones(30)])   # a constant column twice
    assert gls(shim, X.T @ X, np.ones(2))[0] == 2
    assert gls(shim, np.zeros((1, 1)), np.ones(1))[0] == 1


def test_designs():
    from sif_xco2_cokriging_amd.trend import TrendDesign, check_trend
    rng = np.random.default_rng(1)
    c0 = np.column_stack([rng.uniform(25, 50, 100), rng.uniform(-120, -70, 100)])
    c1 = np.column_stack([rng.uniform(30, 40, 80), rng.uniform(-100, -90, 80)])
    d = TrendDesign("constant", [c0, c1])
    assert d.p == [1, 1] and np.array_equal(d(0, c0[:5]), np.ones((5, 1)))
    d = TrendDesign("linear", [c0, c1])
    assert d.p == [3, 3]
    F1 = d.data(1, c1)
    assert np.allclose(F1[:, 1:].mean(0), 0, atol=1e-12) and np.allclose(F1[:, 1:].std(0), 1)
    pc = np.array([[35.0, -95.0]])
    assert np.allclose(d(1, pc)[0, 1:], (pc[0] - c1.mean(0)) / c1.std(0))   # prediction sites: the data sites' scaling
    d = TrendDesign(lambda k, c: np.column_stack([np.ones(len(c)), c[:, 0] ** 2]), [c0])
    assert d.p == [2] and d(0, c0).shape == (100, 2)
    for bad in ("quadratic", 3, [1, 2]):
        with pytest.raises(ValueError):
            check_trend(bad)
    with pytest.raises(ValueError, match="at most 8"):
        TrendDesign(lambda k, c: np.ones((len(c), 9)), [c0])(0, c0)
    with pytest.raises(ValueError, match="shape"):
        TrendDesign(lambda k, c: np.ones((len(c) + 1, 1)), [c0])
    nanF = TrendDesign(lambda k, c: np.where(c[:, :1] > 49, np.nan, 1.0), [c0])
    with pytest.raises(ValueError, match="not finite at data site"):
        nanF.data(0, c0)
    with pytest.raises(ValueError, match="3 data sites for 4 regressors"):
        TrendDesign(lambda k, c: np.ones((len(c), 4)), [c0[:3]]).data(0, c0[:3])


def test_predictor_refusals_before_device_work():
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    rng = np.random.default_rng(2)
    c = np.column_stack([rng.uniform(25, 50, 20), rng.uniform(-120, -70, 20)])
    mf = fields.MultiField([fields.Field(c, rng.standard_normal(20)), fields.Field(c, rng.standard_normal(20))])
    mod = model.MultivariateMatern(2)
    with pytest.raises(ValueError):
        joint_prediction.Predictor(mod, mf, trend="cubic")
    with pytest.raises(NotImplementedError, match="one device"):
        joint_prediction.Predictor(mod, mf, trend="linear", devices=[0, 1])
    P = joint_prediction.Predictor(mod, mf, trend="constant")
    for call in (lambda: P.predict_blocks(0, c, np.zeros(20, dtype=int)), lambda: P.cross_validation(0),
                 lambda: P.conditional_draws_arrays(0, c, 4)):
        with pytest.raises(NotImplementedError, match="simple cokriging only"):
            call()
