"""The Matern derivatives of the log-likelihood gradient (csrc/ck_math.h: ck_matern_dlen_scaled, ck_matern_grad) compiled
for the host with g++ (tests/host_matern_grad_shim.cpp) and checked against scipy, without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.special as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = ctypes.POINTER(ctypes.c_double)
NUS = [0.2, 0.5, 0.7, 1.5, 2.5, 3.5]


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "tests", "_build", "libck_host_matern_grad.so")
    csrc = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + csrc, os.path.join(ROOT, "tests", "host_matern_grad_shim.cpp"),
                    os.path.join(csrc, "ck_model.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def _dlen(shim, nu, s):
    s = np.ascontiguousarray(s, dtype=np.float64)
    out = np.empty_like(s)
    shim.shim_dlen_scaled(ctypes.c_double(nu), s.ctypes.data_as(dp), ctypes.c_long(s.size), out.ctypes.data_as(dp))
    return out


def _grad(shim, nu, ell, h):
    h = np.ascontiguousarray(h, dtype=np.float64)
    out = np.empty((h.size, 3))
    shim.shim_grad(ctypes.c_double(nu), ctypes.c_double(ell), h.ctypes.data_as(dp), ctypes.c_long(h.size),
                   out.ctypes.data_as(dp))
    return out


def matern(nu, ell, h):
    """scipy's Matern correlation, as the reference evaluates it (log-domain prefactor; 1 at h == 0)"""
    h = np.asarray(h, dtype=np.float64)
    x = np.sqrt(2 * nu) * h / ell
    with np.errstate(all="ignore"):
        r = np.exp((1 - nu) * np.log(2) - sps.gammaln(nu) + nu * np.log(x)) * sps.kv(nu, x)
    return np.where(h == 0, 1.0, r)


def lags(nu, ell):
    """scaled lags from 1e-8 to the underflow tail of the correlation"""
    x = np.concatenate([np.geomspace(1e-8, 2.0, 80), np.linspace(2.0, 40.0, 60)[1:], np.geomspace(40.0, 700.0, 40)[1:]])
    return x, x * ell / np.sqrt(2 * nu)


@pytest.mark.parametrize("nu", NUS)
def test_dlen_against_kv_closed_form(shim, nu):
    ell = 350.0
    x, h = lags(nu, ell)
    with np.errstate(all="ignore"):
        D = np.exp((1 - nu) * np.log(2) - sps.gammaln(nu) + nu * np.log(x)) * sps.kv(nu - 1, x)
    ref = x / ell * D
    got = _grad(shim, nu, ell, h)[:, 2]
    ok = (ref > 1e-290) & np.isfinite(ref)
    assert ok.sum() > 150
    assert np.max(np.abs(got[ok] / ref[ok] - 1)) < 2e-12, nu
    # beyond the underflow of M the derivative is 0, as the value is
    M = _grad(shim, nu, ell, h)[:, 0]
    assert np.all(got[M == 0.0] == 0.0)
    # the scaled form alone (no 1 / ell)
    assert np.max(np.abs(_dlen(shim, nu, x[ok]) / D[ok] - 1)) < 2e-12


@pytest.mark.parametrize("nu", NUS)
def test_dnu_against_finite_differences_of_scipy(shim, nu):
    ell = 300.0
    x, h = lags(nu, ell)
    sel = x < 600.0
    h = h[sel]
    # sixth-order central differences of scipy's Matern in nu (lag h fixed); near h = 0 both sides are rounding noise of a
    # value ~1 (the derivative itself vanishes like x^2 there), hence the floor of the scale at 1 % of its largest value
    e = 3e-3 * nu
    f = lambda d: matern(nu + d * e, ell, h)   # noqa: E731
    ref = (-f(-3) + 9 * f(-2) - 45 * f(-1) + 45 * f(1) - 9 * f(2) + f(3)) / (60 * e)
    got = _grad(shim, nu, ell, h)[:, 1]
    scale = np.maximum(np.abs(ref), 1e-2 * np.max(np.abs(ref)))
    assert np.max(np.abs(got - ref) / scale) < 1e-7, nu


@pytest.mark.parametrize("nu", NUS)
def test_values_at_h_zero_and_in_the_tail(shim, nu):
    g = _grad(shim, nu, 500.0, np.array([0.0, 1e9]))
    assert g[0].tolist() == [1.0, 0.0, 0.0]     # h == 0: M = 1, constant in nu and ell
    assert g[1].tolist() == [0.0, 0.0, 0.0]     # underflow: M = 0 and so are its derivatives
    # M itself is the library's evaluator
    x, h = lags(nu, 500.0)
    M = _grad(shim, nu, 500.0, h)[:, 0]
    ref = matern(nu, 500.0, h)
    ok = ref > 1e-280
    assert np.max(np.abs(M[ok] - ref[ok]) / np.maximum(ref[ok], 1e-12)) < 1e-11
