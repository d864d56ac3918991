"""The plan of the local predictor without a GPU (csrc/ck_host.cpp: ck_host_local_needs, ck_host_local_plan): size classes,
slab offsets, batches under the budget and the tiled systems, compiled for the host with g++ (tests/host_local_plan_shim.cpp)
and checked against a restatement in numpy; the same functions in a stand-alone program under -fsanitize=address,undefined
(tests/host_local_plan_sanitize_main.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
LDS = 100   # the LDS limit is a parameter of the plan


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("local_plan") / "libck_host_local_plan.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_local_plan_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def plan(lib, cnt, k_hi, trend, budget, lds=LDS):
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    m = len(cnt)
    ll = ctypes.POINTER(ctypes.c_longlong)
    sc, need, tiled, off = (np.zeros(n, np.int64) for n in (7, m, m, m))
    batches, sys_, tbatches = np.zeros((m, 2), np.int64), np.zeros((m, 5), np.int64), np.zeros((m, 2), np.int64)
    lib.shim_local_plan(cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.c_longlong(m), lds, k_hi, trend,
                        ctypes.c_longlong(budget), *(a.ctypes.data_as(ll) for a in (sc, need, tiled, off, batches, sys_, tbatches)))
    return dict(k_max=sc[0], n_empty=sc[1], need_max=sc[2], slab=sc[3], need=need, tiled=tiled[:sc[4]], off=off,
                batches=batches[:sc[5]], sys=sys_[:sc[4]], tbatches=tbatches[:sc[6]])


def tiled_doubles(k, p):
    """the scratch of one tiled system: (kq + 128) rows of ld = kq + 128 doubles, 8 inverses of 64 x 64, k ints; kept even"""
    kq = (k + 2 + p + 63) // 64 * 64
    return ((kq + 128) * (kq + 128) + 8 * 64 * 64 + (k + 1) // 2 + 1) & ~1


def check_batches(bt, need, off, budget, cap):
    """in-order partition; offsets = prefix sums inside a batch, even; sums within cap; a batch ends only where the next
    element would not fit the budget.  -> the largest batch sum"""
    assert bt[0, 0] == 0 and bt[-1, 1] == len(need) and np.array_equal(bt[1:, 0], bt[:-1, 1]) and np.all(bt[:, 1] > bt[:, 0])
    assert np.all(off % 2 == 0)
    sums = []
    for b, e in bt:
        assert np.array_equal(off[b:e], np.cumsum(need[b:e]) - need[b:e])
        sums.append(int(need[b:e].sum()))
        assert sums[-1] <= cap
        if e < len(need):
            assert sums[-1] + need[e] > budget
    return max(sums)


def check(lib, cnt, k_hi, trend, budget):
    cnt = np.asarray(cnt, dtype=np.int64)
    P = plan(lib, cnt, k_hi, trend, budget)
    slab_class = (cnt > LDS) & (cnt <= k_hi)
    need = np.where(slab_class, ((cnt + 2) * cnt + (cnt + 1) // 2 + 3) & ~1, 0)
    tneed = tiled_doubles(cnt, trend)
    assert np.array_equal(P["need"], need)
    assert P["k_max"] == cnt.max() and P["n_empty"] == np.sum(cnt == 0)
    assert P["need_max"] == max(need.max(), np.where(cnt > k_hi, tneed, 0).max())
    idx = np.flatnonzero(cnt > k_hi)
    tiled = idx[np.lexsort((idx, -cnt[idx]))]     # count descending, then index ascending
    assert np.array_equal(P["tiled"], tiled)
    cap = max(budget, int(P["need_max"]))
    largest = check_batches(P["batches"], need, P["off"], budget, cap)
    if len(tiled):
        s = P["sys"]
        kq = (cnt[tiled] + 2 + trend + 63) // 64 * 64
        assert np.array_equal(s[:, 1], cnt[tiled]) and np.array_equal(s[:, 2], kq) and np.array_equal(s[:, 3], kq + 128)
        assert np.array_equal(s[:, 4], tiled)
        largest = max(largest, check_batches(P["tbatches"], tneed[tiled], s[:, 0], budget, cap))
    else:
        assert len(P["tbatches"]) == 0
    assert P["slab"] == largest
    return P


@pytest.mark.parametrize("trend", [0, 3])
@pytest.mark.parametrize("k_hi", [60, LDS, 140])   # below the LDS limit (the universal form), at it, above it
def test_plan_edges(shim, k_hi, trend):
    P = check(shim, [0] * 9, k_hi, trend, 4096)
    assert P["slab"] == 0 and len(P["batches"]) == 1 and P["n_empty"] == 9
    check(shim, [LDS, LDS + 1, k_hi, k_hi + 1, 0, LDS - 1], k_hi, trend, 4096)     # exactly at and one above both limits
    P = check(shim, [137], k_hi, trend, 0)                                             # one point
    assert len(P["batches"]) == 1 and len(P["tiled"]) == (137 > k_hi)
    cnt = [120, 130, 110, 125, 135, 300, 300, 200, 170]
    P = check(shim, cnt, k_hi, trend, 1)                 # below every single need: every batch still holds one element
    assert len(P["tbatches"]) == len(P["tiled"]) and all(np.count_nonzero(P["need"][b:e]) <= 1 for b, e in P["batches"])
    # a budget equal to a running sum fits (the cut is at >, not >=); one double less does not
    for need in (P["need"], np.array([tiled_doubles(cnt[t], trend) for t in P["tiled"]])):
        for run in np.cumsum(need)[need > 0]:
            check(shim, cnt, k_hi, trend, int(run))
            check(shim, cnt, k_hi, trend, int(run) - 1)


def test_plan_random_counts(shim):
    rng = np.random.default_rng(3)
    cnt = np.where(rng.random(4000) < 0.2, 0, rng.integers(0, 400, 4000))
    for k_hi, trend, budget in ((60, 3, 700000), (LDS, 0, 0), (180, 0, 300000), (250, 3, 2000000), (10 ** 6, 0, 50000)):
        check(shim, cnt, k_hi, trend, budget)


def test_plan_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_local_plan_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_local_plan_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
