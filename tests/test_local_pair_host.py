"""CPU tests of both processes in the moving neighbourhood: the new host planning (csrc/ck_host.cpp: ck_host_sim_order,
ck_host_sim_ext, ck_host_local_pair_needs) compiled for the host with g++ (tests/host_local_pair_shim.cpp) against numpy, the
same functions in a stand-alone program under -fsanitize=address,undefined (tests/host_local_pair_sanitize_main.cpp), and the
numpy reference itself (tests/local_pair_ref.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import local_pair_ref as lp
from tests import local_sim_ref as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
LL = ctypes.c_longlong
LLP, IP = ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("local_pair") / "libck_host_local_pair.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_local_pair_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.shim_pair_classes.restype = None
    return lib


def _ll(a):
    return a.ctypes.data_as(LLP)


def _ip(a):
    return a.ctypes.data_as(IP)


@pytest.mark.parametrize("m0,m1", [(1, 0), (0, 1), (1, 1), (3, 5), (257, 2)])
@pytest.mark.parametrize("direct", [True, False])
def test_stacked_ordering_and_ext_map(shim, m0, m1, direct):
    rng = np.random.default_rng(100 * m0 + m1)
    m = m0 + m1
    rank = rng.permutation(m).astype(np.int64)
    if not direct:
        rank = 5 * rank - 17          # distinct, no permutation of 0 .. m - 1: the sorting path
    pos, dup = np.full(m, -1, dtype=np.int32), np.zeros(2, dtype=np.int64)
    assert shim.shim_sim_order(_ll(rank), LL(m0), LL(m1), _ip(pos), _ll(dup)) == 0
    assert np.array_equal(pos, lp.stacked_order(rank, m0, m1))
    # the augmented set: n = (11, 70) data, the sites behind them, shuffled internal orders, process 1 behind padding
    n = (11, 70)
    N = sum(n)
    nc = (n[0] + m0, n[1] + m1)
    n0p = -(-nc[0] // 64) * 64
    npad = n0p + -(-nc[1] // 64) * 64
    perm = [rng.permutation(c).astype(np.int64) for c in nc]
    ext, rs, rp = (np.full(npad, -7, dtype=np.int32), np.full(npad, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32))
    assert shim.shim_sim_ext(_ll(rank), 2, LL(n[0]), LL(n[1]), LL(m0), LL(m1), LL(n0p), LL(npad), _ll(perm[0]), _ll(perm[1]), _ip(ext),
                             _ip(rs), _ip(rp)) == 0
    aug = lp.augmented_ext(n, (m0, m1))            # the augmented caller order (process q: data, then sites) -> stacked index
    want_ext = np.full(npad, -1, dtype=np.int64)
    want_ext[:nc[0]] = aug[:nc[0]][perm[0]]
    want_ext[n0p:n0p + nc[1]] = aug[nc[0]:][perm[1]]
    assert np.array_equal(ext, want_ext)
    want_rs = np.where(want_ext < 0, np.iinfo(np.int32).max, want_ext)
    site = want_ext >= N
    want_rs[site] = N + pos[want_ext[site] - N]
    assert np.array_equal(rs, want_rs)
    assert np.array_equal(rp, N + pos)
    assert np.all(rs[~site & (want_ext >= 0)] < rp.min())     # every datum precedes every site


def test_duplicate_ranks_name_both_stacked_sites(shim):
    m0, m1 = 3, 5
    rank = np.array([4, 9, 2, 7, 1, 9, 0, 3], dtype=np.int64)   # stacked sites 1 (process 0) and 5 (site 2 of process 1)
    pos, dup = np.zeros(8, dtype=np.int32), np.zeros(2, dtype=np.int64)
    assert shim.shim_sim_order(_ll(rank), LL(m0), LL(m1), _ip(pos), _ll(dup)) == -1
    assert dup.tolist() == [1, 5]
    rank = np.array([4, 4], dtype=np.int64)
    assert shim.shim_sim_order(_ll(rank), LL(1), LL(1), _ip(pos), _ll(dup)) == -1 and dup.tolist() == [0, 1]


@pytest.mark.parametrize("tile_min", [64, 0, 10 ** 6])
def test_three_extra_row_size_classes(shim, tile_min):
    cnt = np.array([0, 1, 61, 62, 63, 64, 65, 125, 126, 127, 128, 189, 190], dtype=np.int32)
    m = len(cnt)
    cls, kq, ld = (np.zeros(m, dtype=np.int32) for _ in range(3))
    off, out3 = np.zeros(m, dtype=np.int64), np.zeros(3, dtype=np.int64)
    shim.shim_pair_classes(_ip(cnt), LL(m), 64, tile_min, LL(1 << 40), _ip(cls), _ip(kq), _ip(ld), _ll(off), _ll(out3))
    k_hi = min(tile_min, 64)                        # the pair form has no slab class: everything above the LDS bound is tiled
    want_cls = np.where(cnt == 0, 0, np.where(cnt > k_hi, 2, 1))
    assert np.array_equal(cls, want_cls)
    tiled = want_cls == 2
    want_kq = -(-(cnt + 3) // 64) * 64
    assert np.array_equal(kq[tiled], want_kq[tiled]) and np.array_equal(ld[tiled], want_kq[tiled] + 128)
    assert not kq[~tiled].any()
    by_k = dict(zip(cnt.tolist(), kq.tolist()))
    if tile_min != 0:
        assert [by_k[k] for k in (65, 125, 126, 127, 128, 189, 190)] == [128, 128, 192, 192, 192, 192, 256]
    else:
        assert [by_k[k] for k in (1, 61, 62, 63, 64, 65)] == [64, 64, 128, 128, 128, 128]
    # one batch under a large budget: the offsets are the prefix sums of the systems, largest first, three rows counted
    doubles = (want_kq + 128) * (want_kq + 128) + 8 * 64 * 64 + (cnt + 1) // 2 + 1 & ~1
    order = [p for p in np.argsort(-cnt, kind="stable") if tiled[p]]
    at = 0
    for p in order:
        assert off[p] == at
        at += int(doubles[p])
    assert out3[0] == at and out3[1] == (1 if order else 0) and out3[2] == (max(int(doubles[p]) for p in order) if order else 0)
    # the smallest budget (the call raises it to the largest single system): batches are cut greedily in that order
    shim.shim_pair_classes(_ip(cnt), LL(m), 64, tile_min, LL(1), _ip(cls), _ip(kq), _ip(ld), _ll(off), _ll(out3))
    budget = max((int(doubles[p]) for p in order), default=0)
    n_batches, acc, largest = (1 if order else 0), 0, 0
    for j, p in enumerate(order):
        if acc + int(doubles[p]) > budget and acc > 0:
            n_batches, acc = n_batches + 1, 0
        assert off[p] == acc
        acc += int(doubles[p])
        largest = max(largest, acc)
    assert out3[1] == n_batches and out3[0] == largest and (n_batches >= 6 or not order)


def test_host_planning_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_local_pair_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_local_pair_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [1, 2, 3])
def test_reference_posterior_matrices_are_positive_semidefinite(row):
    pb = ls.row_inputs(row)
    ref = lp.local_pair_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["sites"][:60], pb["max_dist"], pb["caps"])
    assert ref["gap"] > 1e-9
    solved = ref["k"] > 0
    assert solved.any() and ref["n_not_pd"] == 0
    ev = np.linalg.eigvalsh(ref["post"][solved])
    assert np.all(ev[:, 0] >= -1e-12 * ev[:, 1])
    e0, e1, cov = ref["err0"][solved], ref["err1"][solved], ref["cov"][solved]
    assert np.all(np.abs(cov) <= e0 * e1 * (1 + 1e-12))
    assert np.all(np.isnan(ref["cov"][~solved])) and np.all(np.isnan(ref["pred0"][~solved]))
    # either process alone is the oracle's local predictor
    from oracle import cokrige_oracle as orc
    p = orc.Params.from_flat(pb["params"])
    if pb["caps"] == (0, 0):
        for q in range(2):
            pred, err = orc.local_predict(p, pb["coords"], pb["values"], pb["sites"][:60], q, pb["metric"], max_dist=pb["max_dist"])[:2]
            np.testing.assert_allclose(ref[f"pred{q}"], pred, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(ref[f"err{q}"], err, rtol=1e-9, atol=1e-12)


def test_reference_uncorrelated_processes_and_a_neighbourhood_of_one_process():
    """rho_12 = 0 and only process-0 data in range: process 1's prediction is its prior, the covariance of the errors 0"""
    pb = ls.row_inputs(2)
    pv = list(pb["params"])
    pv[10] = 0.0
    coords = [pb["coords"][0], pb["coords"][1] + 50.0]      # process 1's data far out of every site's reach
    ref = lp.local_pair_reference(pv, coords, pb["values"], pb["metric"], pb["sites"], pb["max_dist"], pb["caps"])
    solved = ref["k"] > 0
    assert solved.sum() > 40 and not ref["count"][:, 1].any()
    assert np.all(ref["cov"][solved] == 0.0) and np.all(ref["pred1"][solved] == 0.0) and np.any(ref["pred0"][solved] != 0.0)
    assert np.allclose(ref["err1"][solved], np.sqrt(pv[1] ** 2 + pv[9]), rtol=1e-15)


def test_cosim_reference_with_one_site_set_is_the_single_reference():
    pb = ls.row_inputs(2)
    a = ls.local_sim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], 1, pb["sites"], pb["ranks"], pb["max_dist"],
                               pb["caps"])
    b = lp.local_cosim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], np.zeros((0, 2)), pb["sites"], pb["ranks"],
                                 pb["max_dist"], pb["caps"])
    assert all(np.array_equal(x, y) for x, y in zip(a["members"], b["members"]))
    assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["var"], b["var"])
    assert np.array_equal(a["count"][:, 2], b["count"][:, 3]) and not b["count"][:, 2].any()
    eps = np.random.default_rng(1).standard_normal((3, 50))
    assert np.array_equal(a["draws"](eps), b["draws"](eps))
