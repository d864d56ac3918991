"""The Vecchia likelihood without a GPU: the numpy reference of tests/vecchia_ref.py against the dense log-density under full
conditioning; vecchia.ordering_ranks and the validation of vecchia.Vecchia; the term arithmetic of csrc/ck_vecchia.h and the
fixed-order sums of k_vecchia_terms / k_vecchia_sum compiled for the host (tests/host_vecchia_shim.cpp) against numpy; the same
in a stand-alone program under -fsanitize=address,undefined (tests/host_vecchia_sanitize_main.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)

from tests import vecchia_ref as vr   # noqa: E402

EUC = 1


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    from sif_xco2_cokriging_amd import synth
    coords, values = vr.half_colocated_sites(150)
    assert np.array_equal(coords[0][:75], coords[1][:75])          # half of process 1 co-located with process 0
    return dict(coords=coords, values=values, params=list(synth.SET_B_UNIT))


@pytest.mark.parametrize("ordering", ["random", "identity"])
def test_reference_equals_the_dense_logpdf_under_full_conditioning(problem, ordering):
    n = 300
    ranks = np.random.default_rng(3).permutation(n) if ordering == "random" else np.arange(n)
    ref = vr.vecchia_reference(problem["params"], problem["coords"], problem["values"], EUC, ranks, 10.0)
    dense = vr.dense_logpdf(problem["params"], problem["coords"], problem["values"], EUC)
    assert ref["info"] == 0 and ref["n_empty"] == 1 and ref["k_max"] == n - 1 and ref["n_capped"] == 0
    assert ref["count"].sum(axis=1)[np.argmin(ranks)] == 0
    for k in range(3):                                             # l, log|Sigma| and the quadratic form separately
        assert abs(ref["out3"][k] - dense[k]) <= 1e-12 * abs(dense[k]), (k, ref["out3"][k], dense[k])


def test_reference_cut_keeps_ties_and_counts_capped_data(problem):
    ranks = np.random.default_rng(3).permutation(300)
    D, proc = vr.stacked_distances(problem["coords"], EUC)
    keep, gap, capped = vr.conditioning_sets(D, proc, ranks, 0.5, (4, 4))
    assert gap.min() > 1e-9
    for t in (int(np.argmax(ranks)), 17):
        for q in range(2):
            cand = (proc == q) & (ranks < ranks[t]) & (D[t] <= 0.5)
            k = np.count_nonzero(keep[t] & (proc == q))
            assert k == min(4, np.count_nonzero(cand))
            if k:
                assert D[t, keep[t] & (proc == q)].max() <= np.sort(D[t, cand])[k - 1]
    # ties at the cut are all kept: four equidistant earlier sites, cap 2
    c = [np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])]
    D, proc = vr.stacked_distances(c, EUC)
    keep, gap, capped = vr.conditioning_sets(D, proc, np.array([4, 0, 1, 2, 3]), 2.0, (2,))
    assert keep[0].sum() == 4 and capped[0] and not keep[1].any()


# ---------------------------------------------------------------------------------------------------------------------
# orderings and the configuration
# ---------------------------------------------------------------------------------------------------------------------
def test_ordering_ranks(problem):
    from sif_xco2_cokriging_amd import native, vecchia
    coords = problem["coords"]
    n = 300
    r = vecchia.ordering_ranks(coords, "random", 5)
    assert r.dtype == np.int64 and np.array_equal(np.sort(r), np.arange(n))
    assert np.array_equal(r, vecchia.ordering_ranks(coords, "random", 5))
    assert not np.array_equal(r, vecchia.ordering_ranks(coords, "random", 6))
    assert np.array_equal(vecchia.ordering_ranks(coords), vecchia.ordering_ranks(coords, "random", 0))   # the defaults
    hr = vecchia.ordering_ranks(coords, "hilbert")
    perm = native.hilbert_order(np.vstack(coords))
    assert hr.dtype == np.int64 and np.array_equal(np.sort(hr), np.arange(n))
    assert np.array_equal(np.argsort(hr), perm)                    # the datum of rank k is the k-th along the curve
    explicit = np.arange(n)[::-1] * 3 - 7
    assert np.array_equal(vecchia.ordering_ranks(coords, explicit), explicit)
    for bad in (np.zeros(n, dtype=int), np.r_[np.arange(n - 1), 0], np.arange(n - 1), np.arange(n, dtype=float), "maxmin",
                np.arange(n).reshape(2, -1)):
        with pytest.raises(ValueError):
            vecchia.ordering_ranks(coords, bad)
    for bad in (-1, 1.5, True, "0"):
        with pytest.raises(ValueError):
            vecchia.ordering_ranks(coords, "random", bad)


def test_vecchia_configuration_is_validated_before_device_work():
    from sif_xco2_cokriging_amd import vecchia
    v = vecchia.Vecchia(0.5)
    assert v.max_dist == 0.5 and v.caps(2) == (0, 0) and v.ordering == "random" and v.seed == 0
    assert vecchia.Vecchia(250, max_neighbours=16).caps(2) == (16, 16)
    assert vecchia.Vecchia(250, max_neighbours=(8, 5), ordering="hilbert", seed=3).caps(2) == (8, 5)
    assert vecchia.Vecchia(1.0, max_neighbours=7).caps(1) == (7, 0)
    for bad in (-1.0, np.inf, np.nan, "1", None, True):
        with pytest.raises(ValueError):
            vecchia.Vecchia(bad)
    for bad in (-1, (8, -5), 2.5, (8, 5.0), "8", True, (8, 5, 3), ()):
        with pytest.raises(ValueError):
            vecchia.Vecchia(0.5, max_neighbours=bad)
    with pytest.raises(ValueError):
        vecchia.Vecchia(0.5, max_neighbours=(8, 5)).caps(1)        # one process, two caps
    for bad in ("maxmin", np.array([0, 0, 1]), np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            vecchia.Vecchia(0.5, ordering=bad)
    with pytest.raises(ValueError):
        vecchia.Vecchia(0.5, seed=-3)


def _model_and_fields():
    from sif_xco2_cokriging_amd import fields, model
    rng = np.random.default_rng(2)
    c = np.column_stack([rng.uniform(25, 50, 20), rng.uniform(-120, -70, 20)])
    mf = fields.MultiField([fields.Field(c, rng.standard_normal(20)) for _ in range(2)])
    return model.MultivariateMatern(2), mf


def test_python_refusals_need_no_device():
    from sif_xco2_cokriging_amd import vecchia
    mod, mf = _model_and_fields()
    v = vecchia.Vecchia(300.0, max_neighbours=8)
    with pytest.raises(ValueError, match="REML"):
        mod.log_likelihood(mf, vecchia=v, trend="constant")
    with pytest.raises(NotImplementedError, match="no analytic gradient yet"):
        mod.log_likelihood(mf, vecchia=v, gradient=True)
    with pytest.raises(ValueError, match="REML"):
        mod.fit_likelihood(mf, vecchia=v, trend="constant")
    with pytest.raises(NotImplementedError, match="Fisher information"):
        mod.fit_likelihood(mf, vecchia=v, std_errors=True)
    for bad in (0.0, -1e-4, 0.5, 1, "1e-4"):
        with pytest.raises(ValueError, match="fd_step"):
            mod.fit_likelihood(mf, vecchia=v, fd_step=bad)
    assert mod._lik is None                                         # no handle was made


# ---------------------------------------------------------------------------------------------------------------------
# the term header on the host
# ---------------------------------------------------------------------------------------------------------------------
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vecchia") / "libck_vecchia.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + CSRC, os.path.join(ROOT, "tests", "host_vecchia_shim.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.shim_vecchia_term.argtypes = [ctypes.c_double] * 5 + [ctypes.c_int, _dp]
    lib.shim_vecchia_term.restype = ctypes.c_int
    lib.shim_vecchia_terms.argtypes = [ctypes.c_long, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp]
    lib.shim_vecchia_terms.restype = ctypes.c_longlong
    return lib


def term(lib, z, mu, vv, prior, noise, k):
    out = np.zeros(4)
    rc = lib.shim_vecchia_term(z, mu, vv, prior, noise, k, out.ctypes.data_as(_dp))
    return rc, out


def test_one_term(shim):
    rc, (m, s2, lv, q) = term(shim, 0.7, 0.2, 0.4, 1.02, 0.0, 5)
    assert rc == 0 and m == 0.2 and s2 == 1.02 - 0.4 and lv == pytest.approx(np.log(0.62), rel=1e-15)
    assert q == pytest.approx(0.25 / 0.62, rel=1e-15)
    rc, (m, s2, lv, q) = term(shim, 0.7, 0.2, 0.4, 1.02, 0.3, 5)   # the datum's own noise
    assert rc == 0 and s2 == (1.02 + 0.3) - 0.4
    rc, (m, s2, lv, q) = term(shim, 0.7, np.nan, np.nan, 1.02, 0.3, 0)   # empty set: the prior density, counted
    assert rc == 0 and m == 0.0 and s2 == 1.02 + 0.3 and q == pytest.approx(0.49 / 1.32, rel=1e-15)
    for vv in (1.02, 1.5, np.nan, np.inf):                         # s^2 = 0, < 0, not a number
        rc, (m, s2, lv, q) = term(shim, 0.7, 0.2, vv, 1.02, 0.0, 3)
        assert rc == 1 and np.isnan(lv) and np.isnan(q) and not s2 > 0
    rc, (m, s2, lv, q) = term(shim, 0.7, np.nan, 0.1, 1.02, 0.0, 3)     # the local system was not positive definite
    assert rc == 1 and np.isnan(lv) and np.isnan(q)


def run_terms(lib, z, mu, vv, prior, noise, cnt):
    n = len(z)
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (z, mu, vv, prior)]
    nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float64)
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    mean, var, out3 = np.zeros(n), np.zeros(n), np.zeros(3)
    info = lib.shim_vecchia_terms(n, *[x.ctypes.data_as(_dp) for x in a], None if nz is None else nz.ctypes.data_as(_dp),
                                  cnt.ctypes.data_as(_ip), mean.ctypes.data_as(_dp), var.ctypes.data_as(_dp),
                                  out3.ctypes.data_as(_dp))
    return info, mean, var, out3


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 65537])
@pytest.mark.parametrize("with_noise", [False, True])
def test_terms_and_fixed_order_sums_against_numpy(shim, n, with_noise):
    rng = np.random.default_rng(n)
    z, mu, vv = rng.standard_normal(n), rng.standard_normal(n), 0.99 * rng.random(n)
    prior = np.where(np.arange(n) % 2 == 0, 1.02, 1.52)
    noise = 0.5 * rng.random(n) if with_noise else None
    cnt = np.column_stack([1 + np.arange(n) % 5, np.arange(n) % 3])
    empty = np.arange(n) % 4 == 1
    cnt[empty] = 0
    info, mean, var, out3 = run_terms(shim, z, mu, vv, prior, noise, cnt)
    rm = np.where(empty, 0.0, mu)
    rv = (prior + (noise if with_noise else 0.0)) - np.where(empty, 0.0, vv)
    assert info == 0 and np.array_equal(mean, rm) and np.array_equal(var, rv)
    s1, s2 = np.log(rv).sum(), ((z - rm) ** 2 / rv).sum()
    assert out3[1] == pytest.approx(s1, rel=1e-12, abs=1e-12 * n) and out3[2] == pytest.approx(s2, rel=1e-12)
    assert out3[0] == pytest.approx(-0.5 * (n * np.log(2 * np.pi) + s1 + s2), rel=1e-12)
    assert np.array_equal(out3, run_terms(shim, z, mu, vv, prior, noise, cnt)[3])


def test_first_datum_without_a_term_is_reported(shim):
    n = 1000
    rng = np.random.default_rng(1)
    z, mu, vv, prior = rng.standard_normal(n), rng.standard_normal(n), 0.5 * rng.random(n), np.full(n, 1.02)
    cnt = np.ones((n, 2), dtype=np.int32)
    vv[[700, 301, 999]] = 1.02
    info, mean, var, out3 = run_terms(shim, z, mu, vv, prior, None, cnt)
    assert info == 302 and np.all(np.isnan(out3))
    ok = np.ones(n, dtype=bool)
    ok[[700, 301, 999]] = False
    assert np.array_equal(var[ok], (1.02 - vv)[ok]) and np.array_equal(mean, mu)


def test_terms_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_vecchia_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_vecchia_sanitize_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
