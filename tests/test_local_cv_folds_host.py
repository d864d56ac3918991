"""Cross-validation by folds and buffers in the moving neighbourhood, without a GPU: the plan of ck_cv_local_folds
(csrc/ck_host.cpp: ck_host_local_cv_plan) compiled for the host with g++ (tests/host_local_cv_shim.cpp) against a few lines of
numpy; the same function in a stand-alone program under -fsanitize=address,undefined (tests/host_local_cv_sanitize_main.cpp);
fold_codes with the fold-size cap lifted; the argument validation of point_prediction.Predictor.cross_validation(folds=...,
also_withhold=..., buffer=...), all of which happens before any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("local_cv") / "libck_host_local_cv.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_local_cv_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def plan(lib, i, n, perm, fold, n_folds, buffer_i=False, n_procs=2):
    """-> dict of the plan's arrays, or the refusal's text"""
    ip, lp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    n_i, N = n[i] if i < 2 else 0, n[0] + (n[1] if n_procs == 2 else 0)
    perm = [np.ascontiguousarray(p, dtype=np.int64) for p in perm]
    fold = [None if f is None else np.ascontiguousarray(f, dtype=np.int32) for f in fold]
    plist, fp, idx, gself = (np.full(max(k, 1), -7, np.int32) for k in (n_i, n_i, n_i, N))
    off, size, sc = np.full(max(n_folds, 1) + 1, -7, np.int64), np.full(max(n_folds, 1), -7, np.int64), np.zeros(3, np.int64)
    msg = ctypes.create_string_buffer(512)
    n0p = (n[0] + 63) // 64 * 64
    rc = lib.shim_local_cv_plan(i, n_procs, ctypes.c_longlong(n[0]), ctypes.c_longlong(n[1]), ctypes.c_longlong(n0p),
                                perm[0].ctypes.data_as(lp), perm[1].ctypes.data_as(lp),
                                None if fold[0] is None else fold[0].ctypes.data_as(ip),
                                None if fold[1] is None else fold[1].ctypes.data_as(ip), n_folds, int(buffer_i), sc.ctypes.data_as(lp),
                                plist.ctypes.data_as(ip), fp.ctypes.data_as(ip), idx.ctypes.data_as(ip), off.ctypes.data_as(lp),
                                size.ctypes.data_as(lp), gself.ctypes.data_as(ip), msg, 512)
    if rc:
        return msg.value.decode()
    m = int(sc[0])
    return dict(plist=plist[:m], fp=fp[:m], idx=idx[:m], n_groups=int(sc[1]), off=off[:sc[2]], size=size[:max(n_folds, 0)], gself=gself[:N],
                n0p=n0p)


def check(P, i, n, perm, fold, n_folds):
    """the plan against numpy: predicted data in the caller's order, stable groups, fold sizes over both processes, gself"""
    assert isinstance(P, dict), P
    fi, fo = fold[i], fold[1 - i]
    pl = np.arange(n[i]) if fi is None else np.flatnonzero(np.asarray(fi) >= 0)
    assert np.array_equal(P["plist"], pl)
    assert np.array_equal(P["fp"], np.full(len(pl), -1) if fi is None else np.asarray(fi)[pl])
    if fi is None:
        assert P["n_groups"] == (1 if n[i] else 0) and np.array_equal(P["idx"], np.arange(n[i]))
        assert np.array_equal(P["off"], [0, n[i]] if n[i] else [0])
    else:
        assert P["n_groups"] == n_folds
        order = np.argsort(P["fp"], kind="stable")               # by fold, ascending position inside a fold
        assert np.array_equal(P["idx"], order)
        assert np.array_equal(P["off"], np.concatenate([[0], np.cumsum(np.bincount(P["fp"], minlength=n_folds))]))
    size = np.zeros(n_folds, np.int64)
    for f in (fi, fo):
        if f is not None:
            f = np.asarray(f)
            size += np.bincount(f[f >= 0], minlength=n_folds)
    assert np.array_equal(P["size"], size)
    g = np.empty(n[0] + n[1], np.int64)
    g[np.asarray(perm[0])] = np.arange(n[0])
    g[n[0] + np.asarray(perm[1])] = P["n0p"] + np.arange(n[1])
    assert np.array_equal(P["gself"], g)


@pytest.mark.parametrize("n_i", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("i", [0, 1])
def test_plan_against_numpy_at_ragged_sizes(shim, n_i, i):
    rng = np.random.default_rng(100 * n_i + i)
    n = [0, 0]
    n[i], n[1 - i] = n_i, n_i // 2 + 3
    perm = [rng.permutation(n[0]), rng.permutation(n[1])]
    K = min(5, n_i)
    fold = [rng.integers(-1, K, n[k]) for k in range(2)]
    fold[i][rng.permutation(n_i)[:K]] = np.arange(K)              # every fold holds a datum of process i
    check(plan(shim, i, n, perm, fold, K), i, n, perm, fold, K)
    one_sided = list(fold)
    one_sided[1 - i] = None                                         # nothing of the other process is withheld
    check(plan(shim, i, n, perm, one_sided, K), i, n, perm, one_sided, K)
    single = [np.arange(n[0]), None] if i == 0 else [None, np.arange(n[1])]          # singleton folds
    check(plan(shim, i, n, perm, single, n_i), i, n, perm, single, n_i)
    check(plan(shim, i, n, perm, [None, None], 0, buffer_i=True), i, n, perm, [None, None], 0)     # the buffer-only call
    all_minus = [np.full(n[0], -1), np.full(n[1], -1)]                              # labels given, nobody withheld
    P = plan(shim, i, n, perm, all_minus, 0)
    check(P, i, n, perm, all_minus, 0)
    assert len(P["plist"]) == 0


def test_plan_labels_with_gaps_and_one_process(shim):
    """a label set whose codes are used unevenly; the univariate form ignores the second array"""
    n, perm = [9, 4], [np.arange(9)[::-1], np.arange(4)]
    fold = [np.array([2, -1, 0, 2, 2, -1, 1, 0, -1]), np.array([-1, 2, 2, -1])]
    P = plan(shim, 0, n, perm, fold, 3)
    check(P, 0, n, perm, fold, 3)
    assert P["idx"].tolist() == [1, 5, 4, 0, 2, 3] and P["size"].tolist() == [2, 1, 5]
    P = plan(shim, 0, [9, 0], [perm[0], np.arange(0)], [fold[0], np.array([77])], 3, n_procs=1)
    assert isinstance(P, dict) and P["size"].tolist() == [2, 1, 3]


def test_plan_refusals_name_the_datum(shim):
    n, perm = [6, 5], [np.arange(6), np.arange(5)]
    ok = np.array([0, 1, 0, 1, -1, 0])
    msg = plan(shim, 0, n, perm, [ok, np.array([0, 1, 2, -1, 0])], 2)
    assert "label 2 of datum 2 of process 1 is outside [-1, n_folds = 2)" in msg
    msg = plan(shim, 0, n, perm, [np.array([0, 1, 0, 1, -2, 0]), None], 2)
    assert "label -2 of datum 4 of process 0" in msg
    msg = plan(shim, 0, n, perm, [np.array([0, -1, 0, -1, -1, 0]), np.array([1, 1, -1, -1, 1])], 2)      # fold 1 wholly in process 1
    assert "fold 1 is empty: it holds no datum of process 0 (and 3 of the other process)" in msg
    msg = plan(shim, 1, n, perm, [ok, None], 2)                      # no labels for the predicted process, no buffer either
    assert "fold labels of the predicted process 1 are null" in msg and "buffer2[1]" in msg
    msg = plan(shim, 1, n, perm, [ok, None], 2, buffer_i=True)       # ... and with the buffer: folds no datum of process 1 is in
    assert "fold 0 is empty" in msg
    assert "n_folds = -3 is negative" in plan(shim, 0, n, perm, [ok, None], -3)
    assert "process index out of range" in plan(shim, 2, n, perm, [ok, None], 2)


def test_plan_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_local_cv_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_local_cv_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_fold_codes_with_the_cap_lifted():
    from sif_xco2_cokriging_amd.joint_prediction import CK_FOLD_MAX, fold_codes
    n = CK_FOLD_MAX + 5
    with pytest.raises(ValueError, match=f"fold 'x' withholds {n} data; the cap is CK_FOLD_MAX = {CK_FOLD_MAX}"):
        fold_codes(["x"] * n, None, n, None)                                         # the default is unchanged
    codes, other, labels = fold_codes(["x"] * n, ["x", None], n, 2, fold_max=None)
    assert labels == ["x"] and np.all(codes == 0) and other.tolist() == [0, -1]
    with pytest.raises(ValueError, match="the cap is CK_FOLD_MAX = 3"):
        fold_codes(["a"] * 4, None, 4, None, fold_max=3)
    a, b = fold_codes(2, None, 3 * CK_FOLD_MAX, None, seed=3, fold_max=None)[0], fold_codes(2, None, 3 * CK_FOLD_MAX, None, seed=3, fold_max=None)[0]
    assert np.array_equal(a, b) and np.bincount(a).tolist() == [3 * CK_FOLD_MAX // 2] * 2


def _predictor(n0=30, n1=20, **kw):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    rng = np.random.default_rng(2)
    c0 = np.column_stack([rng.uniform(25, 50, n0), rng.uniform(-120, -70, n0)])
    c1 = np.column_stack([rng.uniform(25, 50, n1), rng.uniform(-120, -70, n1)])
    mf = fields.MultiField([fields.Field(c0, rng.standard_normal(n0)), fields.Field(c1, rng.standard_normal(n1))])
    return point_prediction.Predictor(model.MultivariateMatern(2), mf, **kw)


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
    with pytest.raises(ValueError, match="also_withhold needs folds"):
        P.cross_validation(0, also_withhold=["a"] * 20, buffer=1.0)
    with pytest.raises(ValueError, match="single device"):
        _predictor(devices=[0, 1]).cross_validation(0, folds=lab)
    with pytest.raises(ValueError, match="single device"):
        _predictor(devices=[0, 1]).cross_validation(0, buffer=5.0)
    with pytest.raises(ValueError, match="process index 2 out of range"):
        P.cross_validation(2, folds=lab)
    with pytest.raises(ValueError, match="max_dist must be finite"):
        P.cross_validation(0, folds=lab, max_dist=float("nan"))
    with pytest.raises(ValueError, match="max_dist must be finite"):
        P.cross_validation(0, buffer=1.0, max_dist=-1.0)
    for bad in (-1.0, float("inf"), float("nan"), (1.0, -2.0), True):
        with pytest.raises(ValueError, match="a buffer radius must be None .off. or finite and >= 0"):
            P.cross_validation(0, folds=lab, buffer=bad)
    with pytest.raises(ValueError, match="one entry per process"):
        P.cross_validation(0, folds=lab, buffer=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="buffer alone predicts every datum of process 1 and needs a radius for that process"):
        P.cross_validation(1, buffer=(3.0, None))
    P.close()
