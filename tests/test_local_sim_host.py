"""The host side of the local conditional simulation without a GPU: the level planner (csrc/ck_host.cpp: ck_host_sim_levels)
compiled for the host with g++ (tests/host_sim_levels_shim.cpp) against the levels of tests/local_sim_ref.py on the four rows of
the issue's table, on a chain and on sites without site-neighbours; the same function in a stand-alone program under
-fsanitize=address,undefined (tests/host_sim_levels_sanitize_main.cpp); and tests/local_sim_ref.py itself against the dense
posterior under full conditioning."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import local_sim_ref as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
LD = 64
_cache = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sim_levels") / "libck_host_sim_levels.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_sim_levels_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.shim_sim_levels.restype = ctypes.c_longlong
    return lib


def plan(lib, pos, nbr_pos):
    """-> (n_levels, level, order, off); nbr_pos[t]: the positions site t conditions on"""
    m = len(pos)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    ns = np.array([len(r) for r in nbr_pos], dtype=np.int32)
    nbr = np.full((m, LD), -1, dtype=np.int32)
    for t, r in enumerate(nbr_pos):
        nbr[t, :len(r)] = r
    level, order, off = np.full(m, -7, np.int32), np.full(m, -7, np.int32), np.full(m + 1, -7, np.int64)
    ip = ctypes.POINTER(ctypes.c_int)
    n = lib.shim_sim_levels(ctypes.c_longlong(m), LD, pos.ctypes.data_as(ip), ns.ctypes.data_as(ip), nbr.ctypes.data_as(ip),
                            level.ctypes.data_as(ip), order.ctypes.data_as(ip), off.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    return n, level, order, off


def check_plan(n, level, order, off, pos, want_level):
    assert n == want_level.max()
    assert np.array_equal(level, want_level)
    assert off[0] == 0 and off[n] == len(pos) and np.all(np.diff(off[:n + 1]) > 0)
    assert np.array_equal(np.sort(order), np.arange(len(pos)))
    for l in range(1, n + 1):
        grp = order[off[l - 1]:off[l]]
        assert np.all(level[grp] == l) and np.all(np.diff(pos[grp]) > 0)   # a level's sites in ascending position


def row_reference(row):
    if row not in _cache:
        pb = ls.row_inputs(row)
        _cache[row] = (pb, ls.local_sim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, pb["sites"], pb["ranks"],
                                                  pb["max_dist"], pb["caps"]))
    return _cache[row]


@pytest.mark.parametrize("row", [1, 2, 3, 4])
def test_levels_of_the_table_rows(shim, row):
    pb, ref = row_reference(row)
    want = ls.ROWS[row]
    assert (ref["n_empty"], ref["k_max"], ref["ns_max"], ref["n_levels"]) == (want["n_empty"], want["k_max"], want["ns_max"],
                                                                                want["n_levels"])
    assert ref["gap"] > 1e-9 and ref["info"] == 0
    pos = ref["pos"]
    n, level, order, off = plan(shim, pos, [pos[u] for u in ref["nbr_sites"]])
    check_plan(n, level, order, off, pos, ref["level"])
    assert n == want["n_levels"]


def test_a_chain_has_m_levels_and_no_neighbours_one(shim):
    rng = np.random.default_rng(3)
    for m in (1, 2, 65, 300):
        pos = rng.permutation(m)
        n, level, order, off = plan(shim, pos, [[q - 1] if q > 0 else [] for q in pos])
        check_plan(n, level, order, off, pos, pos + 1)
        assert n == m
        n, level, order, off = plan(shim, pos, [[] for _ in pos])
        check_plan(n, level, order, off, pos, np.ones(m, dtype=np.int64))
        assert n == 1 and np.array_equal(order, np.argsort(pos))


def test_a_neighbour_that_is_not_earlier_is_refused(shim):
    pos = np.array([2, 0, 1])
    n, _, _, off = plan(shim, pos, [[1], [], [1]])      # site 2 (position 1) names its own position
    assert n == -1 and off[0] == 2 and off[1] == 1
    n, _, _, off = plan(shim, np.array([0, 0, 1]), [[], [], []])
    assert n == -1 and off[0] == 1


def test_reference_is_the_dense_posterior_under_full_conditioning():
    """Row 4: every datum and every earlier site in every set.  The recursion of tests/local_sim_ref.py then is pred + L_S eps
    with L_S the factor of the dense posterior covariance in rank order; measured max |difference| 2.1e-15."""
    pb, ref = row_reference(4)
    eps = np.random.default_rng(1).standard_normal((6, len(pb["sites"])))
    pred, L, order = ls.dense_chain(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, pb["sites"], pb["ranks"])
    got, want = ref["draws"](eps), ls.dense_draws(pred, L, order, eps)
    err = np.max(np.abs(got - want))
    print(f"reference against the dense chain: max |d| {err:.2e}")
    # 63 conditioning members, condition numbers ~1e4 of the local systems: a few hundred ulp of values of order 1
    assert err < 1e-12
    # the diagonal of L_S is the recursion's s_t in rank order
    np.testing.assert_allclose(np.sqrt(ref["var"][order]), np.diag(L), rtol=1e-10)


def test_planner_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_sim_levels_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_sim_levels_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
