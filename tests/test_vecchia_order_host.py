"""The index work of the Vecchia ordering without a GPU (csrc/ck_host.cpp: ck_host_vecchia_order): ranks -> positions of the
data, of the sites in the internal order and every datum's own internal index, compiled for the host with g++
(tests/host_vecchia_order_shim.cpp) and checked against a restatement in numpy; the same function in a stand-alone program
under -fsanitize=address,undefined (tests/host_vecchia_order_sanitize_main.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vecchia_order") / "libck_host_vecchia_order.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_vecchia_order_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def order(lib, rank, n, n0p, npad, perms):
    """-> (status, pos, rs, gself, dup); n: data per process (one entry: one process), perms: internal position -> caller's index"""
    rank = np.ascontiguousarray(rank, dtype=np.int64)
    N = int(sum(n))
    assert rank.size == N
    perms = [np.ascontiguousarray(p, dtype=np.int64) for p in perms]
    ll, ip = ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)
    pos, rs, gself, dup = np.full(N, -7, np.int32), np.full(npad, -7, np.int32), np.full(N, -7, np.int32), np.zeros(2, np.int64)
    rc = lib.shim_vecchia_order(rank.ctypes.data_as(ll), len(n), ctypes.c_longlong(n[0]), ctypes.c_longlong(n[1] if len(n) == 2 else 0),
                                ctypes.c_longlong(n0p), ctypes.c_longlong(npad), perms[0].ctypes.data_as(ll),
                                perms[1].ctypes.data_as(ll) if len(n) == 2 else None, pos.ctypes.data_as(ip), rs.ctypes.data_as(ip),
                                gself.ctypes.data_as(ip), dup.ctypes.data_as(ll))
    return rc, pos, rs, gself, dup


def restated(rank, n, n0p, npad, perms):
    rank = np.asarray(rank, dtype=np.int64)
    N = int(sum(n))
    pos = np.empty(N, dtype=np.int64)
    pos[np.argsort(rank, kind="stable")] = np.arange(N)
    rs, gself = np.full(npad, INT32_MAX, dtype=np.int64), np.empty(N, dtype=np.int64)
    for k in range(len(n)):
        off, soff = (0, 0) if k == 0 else (n0p, n[0])
        j = np.arange(n[k])
        rs[off + j] = pos[soff + np.asarray(perms[k], dtype=np.int64)]
        gself[soff + np.asarray(perms[k], dtype=np.int64)] = off + j
    return pos, rs, gself


def check(lib, rank, n, n0p, npad, perms):
    rc, pos, rs, gself, _ = order(lib, rank, n, n0p, npad, perms)
    want = restated(rank, n, n0p, npad, perms)
    assert rc == 0
    for got, ref in zip((pos, rs, gself), want):
        assert np.array_equal(got, ref)
    N = int(sum(n))
    assert np.array_equal(np.sort(pos), np.arange(N))                    # a permutation ...
    assert np.array_equal(np.argsort(pos), np.argsort(rank, kind="stable"))   # ... in the order of the ranks
    assert np.array_equal(np.sort(rs[rs != INT32_MAX]), np.arange(N)) and np.count_nonzero(rs == INT32_MAX) == npad - N
    assert np.array_equal(rs[gself], pos)                                # a datum's site carries the datum's position


def layout(rng, n0, n1, two=True, pad=64):
    """sizes as ck_set_data lays them out: process 1 starts at a multiple of 64 when it has data; random site orders"""
    n = [n0, n1] if two else [n0]
    n0p = -(-n0 // pad) * pad if two and n1 > 0 else n0
    npad = -(-(n0p + (n1 if two else 0)) // 128) * 128
    return n, n0p, npad, [rng.permutation(k) for k in n]


def test_ranks_that_are_a_permutation(shim):
    rng = np.random.default_rng(1)
    n, n0p, npad, perms = layout(rng, 70, 33)
    check(shim, rng.permutation(103), n, n0p, npad, perms)
    check(shim, np.arange(103), n, n0p, npad, perms)
    check(shim, np.arange(103)[::-1], n, n0p, npad, perms)


def test_distinct_ranks_that_are_no_permutation(shim):
    rng = np.random.default_rng(2)
    n, n0p, npad, perms = layout(rng, 70, 33)
    r = rng.permutation(103)
    check(shim, r * 5 - 3, n, n0p, npad, perms)                          # negative ones
    check(shim, r + 1, n, n0p, npad, perms)                              # one rank equal to N
    wide = rng.permutation(np.unique(rng.integers(-10 ** 12, 10 ** 12, 200))[:103])
    assert len(wide) == 103
    check(shim, wide, n, n0p, npad, perms)
    big = r.copy()
    big[r == 102] = 2 ** 62                                              # a permutation but for its last entry
    check(shim, big, n, n0p, npad, perms)


@pytest.mark.parametrize("route", ["permutation", "sort"])
def test_two_equal_ranks_name_the_pair(shim, route):
    rng = np.random.default_rng(3)
    n, n0p, npad, perms = layout(rng, 70, 33)
    r = rng.permutation(103) if route == "permutation" else rng.permutation(103) * 7 - 100
    for a, b in ((17, 90), (0, 102), (5, 6)):
        dup = r.copy()
        dup[b] = dup[a]
        rc, _, _, _, pair = order(shim, dup, n, n0p, npad, perms)
        assert rc == -1 and pair.tolist() == [a, b], (route, a, b, pair)
    three = r.copy()
    three[[40, 8, 77]] = three[40]                                       # three of a kind: the two earliest data
    lo = np.setdiff1d(np.flatnonzero(r < r[40]), [8, 77])                # ... and of two pairs the one of the smaller rank
    assert len(lo) >= 2
    three[lo[1]] = three[lo[0]]
    rc, _, _, _, pair = order(shim, three, n, n0p, npad, perms)
    assert rc == -1 and pair.tolist() == sorted([lo[0], lo[1]])
    three[lo[1]] = r[lo[1]]
    rc, _, _, _, pair = order(shim, three, n, n0p, npad, perms)
    assert rc == -1 and pair.tolist() == [8, 40]


def test_second_process_without_data(shim):
    rng = np.random.default_rng(4)
    n, n0p, npad, perms = layout(rng, 50, 0)
    assert n0p == 50
    check(shim, rng.permutation(50), n, n0p, npad, perms)
    check(shim, rng.permutation(50) - 9, n, n0p, npad, perms)


def test_one_process(shim):
    rng = np.random.default_rng(5)
    n, n0p, npad, perms = layout(rng, 50, 0, two=False)
    check(shim, rng.permutation(50), n, n0p, npad, perms)
    check(shim, rng.permutation(50) * 2, n, n0p, npad, perms)


def test_padding_between_the_processes_is_never_earlier(shim):
    rng = np.random.default_rng(6)
    n, n0p, npad, perms = layout(rng, 70, 33)
    assert n0p == 128 and npad == 256
    for rank in (rng.permutation(103), rng.permutation(103) * 3 - 50):
        rc, pos, rs, gself, _ = order(shim, rank, n, n0p, npad, perms)
        assert rc == 0 and np.all(rs[70:128] == INT32_MAX) and np.all(rs[128 + 33:] == INT32_MAX)
        assert np.all(rs[:70] < 103) and np.all(rs[128:128 + 33] < 103)
        assert np.all(gself[:70] < 70) and np.all(gself[70:] >= 128)
        check(shim, rank, n, n0p, npad, perms)


def test_one_datum(shim):
    for rank in ([0], [-5], [41]):
        rc, pos, rs, gself, _ = order(shim, rank, [1], 1, 128, [[0]])
        assert rc == 0 and pos.tolist() == [0] and gself.tolist() == [0] and rs[0] == 0 and np.all(rs[1:] == INT32_MAX)
        check(shim, rank, [1, 0], 1, 128, [[0], []])


def test_order_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_vecchia_order_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_vecchia_order_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
