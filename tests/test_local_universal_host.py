"""Host side of universal cokriging in the moving neighbourhood, without a GPU: the per-neighbourhood GLS step the local
kernels run on the device (csrc/ck_local_gls.h) compiled for the host with g++ (tests/local_gls_shim.cpp) and checked against
numpy, and the refusals of point_prediction.Predictor(trend=...) that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)

OK, RANK_DEF = 0, 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lgls") / "libck_local_gls.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + CSRC, os.path.join(ROOT, "tests", "local_gls_shim.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.shim_local_gls.argtypes = [ctypes.c_int] * 5 + [dp, dp, dp, ctypes.c_double, dp, dp]
    lib.shim_local_gls.restype = ctypes.c_int
    return lib


def gls(lib, p0, p1, n0, n1, i, A, b, r, tol=1e-10):
    dp = ctypes.POINTER(ctypes.c_double)
    A, b, r = (np.ascontiguousarray(x, dtype=float) for x in (A, b, r))
    beta, out2 = np.zeros(p0 + p1), np.zeros(2)
    rc = lib.shim_local_gls(p0, p1, n0, n1, i, A.ctypes.data_as(dp), b.ctypes.data_as(dp), r.ctypes.data_as(dp), tol,
                            beta.ctypes.data_as(dp), out2.ctypes.data_as(dp))
    return rc, beta, out2[0], out2[1]


def system(rng, n0, n1, p0, p1):
    """U = L^-1 X_loc for a block-diagonal X_loc, y, v and x0 of a random neighbourhood"""
    k, p = n0 + n1, p0 + p1
    X = np.zeros((k, p))
    X[:n0, :p0] = rng.standard_normal((n0, p0))
    X[n0:, p0:] = rng.standard_normal((n1, p1))
    M = rng.standard_normal((k, k))
    L = np.linalg.cholesky(M @ M.T + k * np.eye(k))
    U = np.linalg.solve(L, X)
    y, v = rng.standard_normal(k), rng.standard_normal(k)
    return U, y, v


@pytest.mark.parametrize("p0,p1,i", [(1, 0, 0), (1, 1, 0), (1, 1, 1), (3, 3, 0), (3, 3, 1), (8, 8, 0), (8, 8, 1)])   # p = 1, 2, 6, 16
def test_local_gls_against_numpy(shim, p0, p1, i):
    rng = np.random.default_rng(10 * (p0 + p1) + i)
    p = p0 + p1
    U, y, v = system(rng, 30, 25 if p1 else 0, p0, p1)
    A, b = U.T @ U, U.T @ y
    x0 = np.zeros(p)
    x0[(0 if i == 0 else p0):(p0 if i == 0 else p)] = rng.standard_normal(p0 if i == 0 else p1)
    r = x0 - U.T @ v
    rc, beta, rb, rar = gls(shim, p0, p1, 30, 25 if p1 else 0, i, A, b, r)
    assert rc == OK
    ref = np.linalg.solve(A, b)
    assert np.allclose(beta, ref, rtol=1e-11, atol=0)                 # every column kept
    assert np.isclose(rar, r @ np.linalg.solve(A, r), rtol=1e-11, atol=0)
    assert np.isclose(rb, r @ ref, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("p0,p1", [(1, 1), (3, 3), (8, 8), (2, 5)])
@pytest.mark.parametrize("i", [0, 1])
def test_zero_columns_of_the_other_process_are_dropped(shim, p0, p1, i):
    """the other process has no neighbour: its columns of U are zero and leave the system"""
    rng = np.random.default_rng(100 + p0 + p1 + i)
    p = p0 + p1
    n = [28, 0] if i == 0 else [0, 28]
    U, y, v = system(rng, n[0], n[1], p0, p1)
    keep = np.arange(0, p0) if i == 0 else np.arange(p0, p)
    gone = np.setdiff1d(np.arange(p), keep)
    assert np.all(U[:, gone] == 0)
    x0 = np.zeros(p)
    x0[keep] = rng.standard_normal(len(keep))
    A, b, r = U.T @ U, U.T @ y, x0 - U.T @ v
    rc, beta, rb, rar = gls(shim, p0, p1, n[0], n[1], i, A, b, r)
    assert rc == OK
    Ak, bk, rk = A[np.ix_(keep, keep)], b[keep], r[keep]
    ref = np.linalg.solve(Ak, bk)
    assert np.all(np.isnan(beta[gone])) and np.allclose(beta[keep], ref, rtol=1e-11, atol=0)
    assert np.isclose(rar, rk @ np.linalg.solve(Ak, rk), rtol=1e-11, atol=0)
    assert np.isclose(rb, rk @ ref, rtol=1e-11, atol=1e-13)
    # with p_i = 0 and the other process gone nothing is left: simple cokriging
    Z = np.zeros((p, p))
    if i == 0:
        rc, beta, rb, rar = gls(shim, 0, p1, 5, 0, 0, Z[:p1, :p1], np.zeros(p1), np.zeros(p1))
        assert rc == OK and rb == 0.0 and rar == 0.0 and np.all(np.isnan(beta))


@pytest.mark.parametrize("i", [0, 1])
def test_zero_columns_of_the_predicted_process_are_rank_deficient(shim, i):
    rng = np.random.default_rng(7 + i)
    n = [0, 20] if i == 0 else [20, 0]
    U, y, v = system(rng, n[0], n[1], 3, 3)
    x0 = np.zeros(6)
    x0[3 * i:3 * i + 3] = 1.0
    rc, beta, rb, rar = gls(shim, 3, 3, n[0], n[1], i, U.T @ U, U.T @ y, x0 - U.T @ v)
    assert rc == RANK_DEF and np.all(np.isnan(beta)) and np.isnan(rb) and np.isnan(rar)


def test_rank_deficient_designs(shim):
    rng = np.random.default_rng(3)
    # a repeated column
    U, y, v = system(rng, 30, 20, 3, 2)
    U[:, 2] = U[:, 1]
    rc, beta = gls(shim, 3, 2, 30, 20, 0, U.T @ U, U.T @ y, -U.T @ v)[:2]
    assert rc == RANK_DEF and np.all(np.isnan(beta))
    # fewer rows than columns: two neighbours of process 1 for its three regressors
    U, y, v = system(rng, 30, 2, 3, 3)
    for i in (0, 1):
        assert gls(shim, 3, 3, 30, 2, i, U.T @ U, U.T @ y, -U.T @ v)[0] == RANK_DEF
    # a column that is zero although its process has neighbours (a covariate that vanishes in this neighbourhood)
    U, y, v = system(rng, 30, 20, 2, 1)
    U[:, 1] = 0.0
    assert gls(shim, 2, 1, 30, 20, 0, U.T @ U, U.T @ y, -U.T @ v)[0] == RANK_DEF
    # a non-finite entry never passes
    A = np.eye(2)
    A[1, 1] = np.nan
    assert gls(shim, 1, 1, 4, 4, 0, A, np.ones(2), np.ones(2))[0] == RANK_DEF


def test_predictor_refusals_before_device_work():
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    rng = np.random.default_rng(2)
    c = np.column_stack([rng.uniform(25, 50, 20), rng.uniform(-120, -70, 20)])
    mf = fields.MultiField([fields.Field(c, rng.standard_normal(20)), fields.Field(c, rng.standard_normal(20))])
    mod = model.MultivariateMatern(2)
    with pytest.raises(ValueError):
        point_prediction.Predictor(mod, mf, trend="quadratic")
    with pytest.raises(NotImplementedError, match="one device"):
        point_prediction.Predictor(mod, mf, trend="constant", devices=[0, 1])
    P = point_prediction.Predictor(mod, mf, trend="linear")   # no device state yet
    assert P.trend == "linear" and P.trend_coef is None and P._h is None
