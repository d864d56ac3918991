"""Host side of leave-group-out cross-validation, without a GPU: the validation and label handling of
Predictor.cross_validation(folds=...) (sif_xco2_cokriging_amd/joint_prediction.py: fold_codes), and the fold layout of the
library (csrc/ck_host.cpp: ck_host_fold_plan) compiled for the host with g++ (tests/host_folds_shim.cpp), plus the same
function in a stand-alone program under -fsanitize=address,undefined (tests/host_folds_sanitize_main.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)
CK_FOLD_MAX = 4096


def test_header_and_host_agree_on_the_cap():
    import re
    hdr = open(os.path.join(ROOT, "include", "cokrige.h")).read()
    assert int(re.search(r"#define CK_FOLD_MAX (\d+)", hdr).group(1)) == CK_FOLD_MAX
    from sif_xco2_cokriging_amd import joint_prediction
    assert joint_prediction.CK_FOLD_MAX == CK_FOLD_MAX


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("folds") / "libck_host_folds.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_folds_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def plan(lib, i, n, n0p, perm, folds, n_folds, fold_max=CK_FOLD_MAX):
    """-> dict of the plan's arrays, or the error text"""
    ll, ip = ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)
    n_procs = len(n)
    pm = [np.ascontiguousarray(p, dtype=np.int64) for p in perm] + [None] * (2 - n_procs)
    fd = [None if f is None else np.ascontiguousarray(f, dtype=np.int32) for f in folds] + [None] * (2 - len(folds))
    as_ll = lambda a: None if a is None else a.ctypes.data_as(ll)
    as_ip = lambda a: None if a is None else a.ctypes.data_as(ip)
    counts, pmm, bufd = np.zeros(6, dtype=np.int64), np.zeros(2, dtype=np.int64), ctypes.c_longlong(0)
    err = ctypes.create_string_buffer(512)

    def call(*arrays):
        return lib.shim_fold_plan(i, n_procs, ctypes.c_longlong(n[0]), ctypes.c_longlong(n[1] if n_procs == 2 else 0),
                                  ctypes.c_longlong(n0p), as_ll(pm[0]), as_ll(pm[1]), as_ip(fd[0]), as_ip(fd[1]), n_folds, fold_max,
                                  as_ll(counts), as_ll(pmm), *arrays, ctypes.byref(bufd), err, 512)
    if call(None, None, None, None, None, None, None) != 0:
        return err.value.decode()
    out = dict(off=np.zeros(n_folds + 1, np.int32), pos=np.zeros(counts[0], np.int32), cidx=np.zeros(counts[0], np.int32),
               gbase=np.zeros(n_folds, np.int32), gpos=np.zeros(counts[1], np.int32), tiles=np.zeros((counts[2], 5), np.int64),
               big=np.zeros((counts[4], 6), np.int64))
    assert call(as_ip(out["off"]), as_ip(out["pos"]), as_ip(out["cidx"]), as_ip(out["gbase"]), as_ip(out["gpos"]),
                as_ll(out["tiles"]), as_ll(out["big"])) == 0
    out.update(pmin=int(pmm[0]), pmax=int(pmm[1]), n_small=int(counts[3]), n_small_tiles=int(counts[5]), buffer=bufd.value)
    return out


def test_plan_permuted_sites_both_processes(shim):
    rng = np.random.default_rng(0)
    n, n0p = (200, 150), 256
    perm = [rng.permutation(200), rng.permutation(150)]
    f0 = rng.integers(-1, 6, 200).astype(np.int32)
    f1 = rng.integers(-1, 6, 150).astype(np.int32)
    f0[:6] = np.arange(6)                       # every fold holds a datum of process 0
    f0[f0 == 5] = -1
    f0[7:107] = 5                               # one fold above 64 members
    P = plan(shim, 0, n, n0p, perm, [f0, f1], 6)
    assert isinstance(P, dict), P
    inv = [np.argsort(perm[0]), np.argsort(perm[1])]   # internal position of the caller's datum
    for f in range(6):
        want = np.sort(np.concatenate([inv[0][f0 == f], n0p + inv[1][f1 == f]]))
        got = P["pos"][P["off"][f]:P["off"][f + 1]]
        assert np.array_equal(got, want)
        cidx = P["cidx"][P["off"][f]:P["off"][f + 1]]
        assert np.array_equal(cidx[got < n0p], perm[0][got[got < n0p]]) and np.all(cidx[got >= n0p] == -1)
        assert np.array_equal(P["gpos"][P["gbase"][f]:P["gbase"][f] + len(got)], got)
        if len(got) <= 64:
            assert P["gbase"][f] // 128 == (P["gbase"][f] + len(got) - 1) // 128      # no small fold across a tile edge
    withheld = np.concatenate([inv[0][f0 >= 0], n0p + inv[1][f1 >= 0]])
    assert P["pmin"] == withheld.min() and P["pmax"] == withheld.max()
    assert len(P["big"]) == 1 and P["big"][0][5] == 5 and P["n_small"] == 5
    s = int(P["big"][0][1])
    assert P["big"][0][2] == (2 * s + 1 + 63) // 64 * 64 and P["big"][0][3] == P["big"][0][2] + 128
    t = P["tiles"]
    assert np.all(np.diff(t[:, 4]) >= 0) and len(t) == P["n_small_tiles"] + sum(range(1, (s + 127) // 128 + 1))
    for c_off, a0, b0, ld, pos0 in t:
        assert pos0 == min(P["gpos"][a0:a0 + 128].min(), P["gpos"][a0]) and b0 <= a0
        assert c_off + 127 * ld + 128 <= P["buffer"]
    # the predicted process may be the second one; the other array may be absent
    P1 = plan(shim, 1, n, n0p, perm, [None, np.where(f1 < 0, 0, f1)], 6)
    assert isinstance(P1, dict) and np.all(P1["pos"] >= n0p) and np.all(P1["cidx"] >= 0)


def test_plan_refusals(shim):
    perm = [np.arange(10)]
    f = np.zeros(10, dtype=np.int32)
    assert "fold 1 is empty" in plan(shim, 0, (10,), 64, perm, [f], 2)
    f[3] = 2
    msg = plan(shim, 0, (10,), 64, perm, [f], 2)
    assert "label 2 of datum 3 of process 0" in msg and "[-1, n_folds = 2)" in msg
    f[3] = -2
    assert "label -2" in plan(shim, 0, (10,), 64, perm, [f], 2)
    # a fold of the other process's data only is empty for the predicted process
    msg = plan(shim, 0, (10, 10), 64, [np.arange(10), np.arange(10)], [np.zeros(10, np.int32), np.ones(10, np.int32)], 2)
    assert "fold 1 is empty" in msg and "10 of the other process" in msg


def test_plan_fold_of_exactly_the_cap_and_one_more(shim):
    n = CK_FOLD_MAX + 1
    perm = [np.random.default_rng(1).permutation(n)]
    f = np.zeros(n, dtype=np.int32)
    f[0] = -1
    P = plan(shim, 0, (n,), 4160, perm, [f], 1)
    assert isinstance(P, dict) and P["big"][0][1] == CK_FOLD_MAX and len(P["tiles"]) == 32 * 33 // 2
    f[0] = 0
    msg = plan(shim, 0, (n,), 4160, perm, [f], 1)
    assert f"fold 0 holds {CK_FOLD_MAX + 1} data" in msg and f"CK_FOLD_MAX = {CK_FOLD_MAX}" in msg


def test_fold_layout_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_folds_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_folds_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- Python: labels and validation, no device touched -------------------------------------------------------------------
def test_label_factorisation():
    from sif_xco2_cokriging_amd.joint_prediction import fold_codes
    codes, other, labels = fold_codes(["t7", "t2", None, "t7", float("nan"), -1, ("a", 1)], [("a", 1), None, "t7"], 7, 3)
    assert labels == ["t7", "t2", ("a", 1)]
    assert codes.dtype == np.int32 and codes.tolist() == [0, 1, -1, 0, -1, -1, 2] and other.tolist() == [2, -1, 0]
    codes, other, labels = fold_codes(np.array([3.0, np.nan, 3.0, 1.0]), None, 4, None)
    assert labels == [3.0, 1.0] and codes.tolist() == [0, -1, 0, 1] and other is None


def test_random_kfold_is_reproducible_from_seed():
    from sif_xco2_cokriging_amd.joint_prediction import fold_codes
    a = fold_codes(10, None, 1003, None, seed=5)[0]
    b = fold_codes(10, None, 1003, None, seed=5)[0]
    c = fold_codes(10, None, 1003, None, seed=6)[0]
    d = fold_codes(10, None, 1003, None)[0]
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.array_equal(d, fold_codes(10, None, 1003, None, seed=0)[0])
    assert sorted(np.bincount(a).tolist()) == [100] * 7 + [101] * 3 and fold_codes(10, None, 1003, None)[2] == list(range(10))


def _predictor(n0=30, n1=20, **kw):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    rng = np.random.default_rng(2)
    c0 = np.column_stack([rng.uniform(25, 50, n0), rng.uniform(-120, -70, n0)])
    c1 = np.column_stack([rng.uniform(25, 50, n1), rng.uniform(-120, -70, n1)])
    mf = fields.MultiField([fields.Field(c0, rng.standard_normal(n0)), fields.Field(c1, rng.standard_normal(n1))])
    return joint_prediction.Predictor(model.MultivariateMatern(2), mf, **kw)


def test_validation_before_device_work():
    """every refusal is a ValueError raised on the host (without a GPU anything that reached the device would raise
    native.NativeError instead)"""
    P = _predictor()
    lab = ["a"] * 15 + ["b"] * 15
    with pytest.raises(ValueError, match="folds has 29 labels, the predicted process has 30"):
        P.cross_validation(0, folds=lab[:29])
    with pytest.raises(ValueError, match="also_withhold has 30 labels, the other process has 20"):
        P.cross_validation(0, folds=lab, also_withhold=lab)
    with pytest.raises(ValueError, match="also_withhold label 'c' .datum 3. is no label of folds"):
        P.cross_validation(0, folds=lab, also_withhold=["a", "b", None, "c"] + [None] * 16)
    with pytest.raises(ValueError, match="withholds nothing"):
        P.cross_validation(0, folds=[None] * 30)
    with pytest.raises(ValueError, match="K-fold"):
        P.cross_validation(0, folds=31)
    with pytest.raises(ValueError, match="also_withhold needs folds"):
        P.cross_validation(0, also_withhold=["a"] * 20)
    with pytest.raises(ValueError, match="single device"):
        _predictor(devices=[0, 1]).cross_validation(0, folds=lab)
    big = _predictor(n0=CK_FOLD_MAX + 1, n1=3)
    with pytest.raises(ValueError, match=f"fold 'x' withholds {CK_FOLD_MAX + 1} data; the cap is CK_FOLD_MAX = {CK_FOLD_MAX}"):
        big.cross_validation(0, folds=["x"] * (CK_FOLD_MAX + 1))
    with pytest.raises(ValueError, match=f"fold 'x' withholds {CK_FOLD_MAX + 1} data"):
        big.cross_validation(0, folds=["x"] * CK_FOLD_MAX + [None], also_withhold=["x", None, None])


def test_trend_predictor_still_refuses():
    P = _predictor(trend="constant")
    for kw in ({"folds": ["a"] * 30}, {"folds": 5, "seed": 1}, {"folds": ["a"] * 30, "also_withhold": ["a"] * 20, "refactor_each": True}):
        with pytest.raises(NotImplementedError, match="simple cokriging only"):
            P.cross_validation(0, **kw)
