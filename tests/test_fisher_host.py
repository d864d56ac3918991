"""Host side of the Fisher information, without a GPU: the numpy summary of model.py (summarize_information: inversion on
the unit-diagonal scaling, zero rows, a remainder that is not positive definite, the mask, names, conf_int), and the host
functions of the library (csrc/ck_host.cpp: ck_host_fisher_coef / _combine / _reml) compiled with g++
(tests/host_fisher_shim.cpp) against numpy, plus the same functions in a stand-alone program under
-fsanitize=address,undefined (tests/host_fisher_sanitize_main.cpp)."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)

NO = NP = 13
BIV_NAMES = ["sigma_11", "sigma_22", "nu_11", "nu_12", "nu_22", "len_scale_11", "len_scale_12", "len_scale_22", "nugget_11",
             "nugget_22", "rho_12"]


def spd(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, n)) * np.logspace(-3, 3, n)   # scales six orders apart, as the parameters' are
    return X.T @ X


def inv_ref(A):
    """the inverse through the known column scales (numpy's inverse of the unscaled matrix loses digits to them)"""
    s = np.logspace(-3, 3, A.shape[0])
    return np.linalg.inv(A / np.outer(s, s)) / np.outer(s, s)


def full13(block, slots):
    F = np.zeros((13, 13))
    F[np.ix_(slots, slots)] = block
    return F


# ---- the numpy summary ----------------------------------------------------------------------------------------------
def test_names_and_inverse_bivariate():
    from sif_xco2_cokriging_amd.model import information_slot_names, summarize_information
    assert information_slot_names(2) == BIV_NAMES + ["noise_scale_0", "noise_scale_1"]
    slots = list(range(11)) + [12]
    A = spd(12, 1)
    est = np.arange(13, dtype=float)
    live = np.zeros(13, dtype=bool)
    live[slots] = True
    inf = summarize_information(full13(A, slots), 2, live, est)
    assert inf.names == BIV_NAMES + ["noise_scale_1"] and inf.not_identified == [] and inf.positive_definite
    Ai = inv_ref(A)
    assert np.allclose(inf.cov, Ai, rtol=1e-8, atol=0) and np.array_equal(inf.fisher, A)
    assert np.allclose(inf.std_error.values, np.sqrt(np.diag(Ai)), rtol=1e-9)
    assert list(inf.std_error.index) == inf.names
    sd = np.sqrt(np.diag(Ai))
    assert np.allclose(inf.correlation, Ai / np.outer(sd, sd), rtol=1e-8) and np.allclose(np.diag(inf.correlation), 1.0)
    ci = inf.conf_int(0.95)
    assert np.allclose(ci["upper"].values - est[slots], 1.959963984540054 * inf.std_error.values, rtol=1e-12)
    assert np.allclose(est[slots] - ci["lower"].values, 1.959963984540054 * inf.std_error.values, rtol=1e-12)
    assert np.allclose((inf.conf_int(0.5)["upper"].values - est[slots]) / inf.std_error.values, 0.6744897501960817)
    with pytest.raises(ValueError):
        inf.conf_int(1.0)


def test_names_univariate_and_default_mask():
    from sif_xco2_cokriging_amd.model import information_slot_names, summarize_information
    names = information_slot_names(1)
    assert names[:4] == ["sigma_11", "nu_11", "len_scale_11", "nugget_11"] and names[11] == "noise_scale_0"
    assert all(n == "" for n in names[4:11]) and names[12] == ""
    slots = [0, 1, 2, 3, 11]
    A = spd(5, 2)
    live = np.zeros(13, dtype=bool)
    live[slots] = True
    inf = summarize_information(full13(A, slots), 1, live)
    assert inf.names == ["sigma_11", "nu_11", "len_scale_11", "nugget_11", "noise_scale_0"]
    assert np.allclose(inf.cov, inv_ref(A), rtol=1e-8)
    with pytest.raises(ValueError):
        inf.conf_int()                     # no estimates given
    live[11] = False                       # the mask: without the noise scale the others are conditional on it
    inf = summarize_information(full13(A, slots), 1, live)
    s4 = np.outer(np.logspace(-3, 3, 5)[:4], np.logspace(-3, 3, 5)[:4])
    assert inf.names == names[:4] and np.allclose(inf.cov, np.linalg.inv(A[:4, :4] / s4) / s4, rtol=1e-8)
    with pytest.raises(ValueError):
        summarize_information(np.zeros((11, 11)), 2)


def test_zero_rows_are_not_identified():
    from sif_xco2_cokriging_amd.model import summarize_information
    keep = [0, 1, 2, 4, 5, 7, 8, 9, 10]    # rho = 0: nu_12 and len_12 carry no information
    A = spd(9, 3)
    live = np.zeros(13, dtype=bool)
    live[:11] = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        inf = summarize_information(full13(A, keep), 2, live, np.ones(13))
    assert len(w) == 1 and "nu_12, len_scale_12" in str(w[0].message)
    assert inf.not_identified == ["nu_12", "len_scale_12"] and inf.positive_definite
    assert np.all(np.isnan(inf.cov[3])) and np.all(np.isnan(inf.cov[:, 6])) and np.all(np.isnan(inf.correlation[6]))
    assert np.isnan(inf.std_error["nu_12"]) and np.isnan(inf.std_error["len_scale_12"])
    assert np.allclose(inf.cov[np.ix_(keep, keep)], inv_ref(A), rtol=1e-8)
    assert np.all(np.isnan(inf.conf_int().loc["nu_12"].values))


def test_remainder_not_positive_definite():
    from sif_xco2_cokriging_amd.model import summarize_information
    A = spd(4, 4)
    A[0, 1] = A[1, 0] = 2.0 * np.sqrt(A[0, 0] * A[1, 1])   # a "correlation" of 2
    live = np.zeros(13, dtype=bool)
    live[:4] = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        inf = summarize_information(full13(A, [0, 1, 2, 3]), 1, live)
    assert len(w) == 1 and "not positive definite" in str(w[0].message)
    assert not inf.positive_definite and np.all(np.isnan(inf.std_error.values)) and np.all(np.isnan(inf.cov))


def test_at_bound_is_conditioned_on():
    from sif_xco2_cokriging_amd.model import summarize_information
    A = spd(3, 5)
    live = np.zeros(13, dtype=bool)
    live[:4] = True
    bound = np.zeros(13, dtype=bool)
    bound[3] = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        inf = summarize_information(full13(A, [0, 1, 2]), 1, live, None, at_bound=bound)
    assert len(w) == 0 and inf.at_bound == ["nugget_11"] and inf.not_identified == []
    assert np.isnan(inf.std_error["nugget_11"]) and np.allclose(inf.cov[:3, :3], inv_ref(A), rtol=1e-8)


# ---- the library's host functions ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fisher") / "libck_host_fisher.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_fisher_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.shim_fisher_coef.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, dp]
    lib.shim_fisher_coef.restype = None
    lib.shim_fisher_combine.argtypes = [dp, dp, ctypes.POINTER(ctypes.c_ubyte), dp]
    lib.shim_fisher_combine.restype = None
    lib.shim_fisher_reml.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, ctypes.c_int64, dp, dp]
    lib.shim_fisher_reml.restype = ctypes.c_int
    return lib


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _operands(n0, n1, s1, s2, rho, rng):
    """thirteen random symmetric operands with the block structure of ck_internal.h and the derivatives they make up"""
    N = n0 + n1

    def blk(i, j):
        M = np.zeros((N, N))
        r = slice(0, n0) if i == 0 else slice(n0, N)
        c = slice(0, n0) if j == 0 else slice(n0, N)
        B = rng.standard_normal((r.stop - r.start, c.stop - c.start))
        if i == j:
            M[r, c] = B + B.T
        else:
            M[r, c] = B
            M[c, r] = B.T
        return M
    ops = [blk(0, 0) for _ in range(4)] + [blk(1, 1) for _ in range(4)] + [blk(0, 1) for _ in range(3)]
    d = rng.uniform(0.1, 1.0, N)
    ops += [np.diag(np.where(np.arange(N) < n0, d, 0.0)), np.diag(np.where(np.arange(N) >= n0, d, 0.0))]
    D = [2 * s1 * ops[0] + rho * s2 * ops[8], 2 * s2 * ops[4] + rho * s1 * ops[8], ops[1], ops[9], ops[5], ops[2], ops[10], ops[6],
         ops[3], ops[7], s1 * s2 * ops[8], ops[11], ops[12]]
    return ops, D


def test_coefficients_and_combination(shim):
    rng = np.random.default_rng(6)
    s1, s2, rho = 1.1, 0.8, -0.3
    ops, D = _operands(7, 9, s1, s2, rho, rng)
    S = np.linalg.inv(spd(16, 7) / 1e3 + np.eye(16))
    T = np.array([[0.5 * np.trace(S @ a @ S @ b) for b in ops] for a in ops])
    ref = np.array([[0.5 * np.trace(S @ a @ S @ b) for b in D] for a in D])
    C = np.zeros((NP, NO))
    shim.shim_fisher_coef(2, s1, s2, rho, _dp(C))
    live = np.ones(13, dtype=np.uint8)
    live[[4, 12]] = 0
    I = np.zeros((13, 13))
    shim.shim_fisher_combine(_dp(C), _dp(np.ascontiguousarray(np.triu(T))), live.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), _dp(I))
    on = np.flatnonzero(live)
    assert np.array_equal(I, I.T) and np.all(I[4] == 0) and np.all(I[:, 12] == 0)
    assert np.allclose(I[np.ix_(on, on)], ref[np.ix_(on, on)], rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    shim.shim_fisher_coef(1, s1, 0.0, 0.0, _dp(C))
    assert np.count_nonzero(C) == 5 and C[0, 0] == 2 * s1 and C[1, 1] == C[2, 2] == C[3, 3] == C[11, 11] == 1.0


@pytest.mark.parametrize("p", [1, 2, 6, 16])
def test_reml_correction_against_numpy(shim, p):
    rng = np.random.default_rng(p)
    n0, n1 = 11, 14
    N = n0 + n1
    ops, _ = _operands(n0, n1, 1.0, 1.0, 0.5, rng)
    Sig = spd(N, 8) / 1e3 + np.eye(N)
    S = np.linalg.inv(Sig)
    X = rng.standard_normal((N, p))
    H = S @ X
    A = X.T @ H
    P = S - H @ np.linalg.solve(A, H.T)
    ref = np.array([[0.5 * np.trace(P @ a @ P @ b) for b in ops] for a in ops])
    T = np.array([[0.5 * np.trace(S @ a @ S @ b) for b in ops] for a in ops])
    Y = np.column_stack([a @ H for a in ops])            # N x (13 p): Y_a = D_a H
    K = np.ascontiguousarray(Y.T @ S @ Y)
    Gm = np.ascontiguousarray(Y.T @ H)
    Tin = np.ascontiguousarray(np.triu(T))               # the upper triangle is read
    rc = shim.shim_fisher_reml(p, NO, _dp(np.ascontiguousarray(A)), _dp(K), NO * p, _dp(Gm), _dp(Tin))
    assert rc == 0 and np.array_equal(Tin, Tin.T)
    assert np.allclose(Tin, ref, rtol=1e-9, atol=1e-10 * np.abs(ref).max())
    X2 = np.column_stack([X[:, :1], X[:, :1]]) if p == 2 else None
    if X2 is not None:                                   # a repeated column: reported
        assert shim.shim_fisher_reml(2, NO, _dp(np.ascontiguousarray(X2.T @ S @ X2)), _dp(K), NO * p, _dp(Gm), _dp(Tin)) == 2


def test_host_functions_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_fisher_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_fisher_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
