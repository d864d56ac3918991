"""Host side of the joint prediction of both processes, without a GPU: csrc/ck_host.cpp's ck_host_pair_plan and
ck_host_pair_coincident compiled for the host with g++ (tests/host_pair_shim.cpp) against numpy restatements of the layout
include/cokrige.h pins, the same functions in a stand-alone program under -fsanitize=address,undefined
(tests/host_pair_sanitize_main.cpp), and the argument checks of Predictor.predict_pair and of the tuple form of
Predictor.conditional_simulation, which must raise before any device work.  The device half is tests/test_gpu_pair.py."""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from sif_xco2_cokriging_amd import joint_prediction, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pair") / "libck_host_pair.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_pair_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.shim_pair_plan.restype = None
    lib.shim_pair_coincident.restype = LL
    return lib


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _pc(m, seed=0):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])


def plan(lib, pc0, pc1, site_order):
    m0, m1 = len(pc0), len(pc1)
    rows = -(-m0 // 64) * 64 + m1
    out4 = np.zeros(4, np.int64)
    cmap, row_of, xy = np.full(rows, -7, np.int32), np.full(m0 + m1, -7, np.int64), np.full((rows, 2), np.nan)
    lib.shim_pair_plan(_dp(pc0), LL(m0), _dp(pc1), LL(m1), int(site_order), out4.ctypes.data_as(ctypes.POINTER(LL)),
                       cmap.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), row_of.ctypes.data_as(ctypes.POINTER(LL)), _dp(xy))
    return out4, cmap, row_of, xy


@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("size", [(0, 0), (1, 1), (63, 65), (64, 64), (65, 63), (0, 40), (40, 0), (255, 256), (256, 255), (300, 277),
                                  (512, 130)])
def test_layout_gap_rows_and_cmap(shim, size, site_order):
    m0, m1 = size
    pc0, pc1 = np.ascontiguousarray(_pc(m0, 1)), np.ascontiguousarray(_pc(m1, 2))
    out4, cmap, row_of, xy = plan(shim, pc0, pc1, site_order)
    m0p = -(-m0 // 64) * 64
    assert out4[0] == m0p and out4[1] == m0p + m1
    # each set along its own Hilbert curve from 256 sites on when site_order is on, else the caller's order
    order = [native.hilbert_order(pc) if site_order and len(pc) >= 256 else np.arange(len(pc)) for pc in (pc0, pc1)]
    assert [bool(out4[2]), bool(out4[3])] == [bool(site_order) and m0 >= 256, bool(site_order) and m1 >= 256]
    want = np.full(m0p + m1, -1)
    want[:m0] = order[0]
    want[m0p:] = m0 + order[1]
    assert np.array_equal(cmap, want)
    assert np.array_equal(row_of[want[want >= 0]], np.flatnonzero(want >= 0))
    stacked = np.vstack([pc0, pc1])
    assert np.array_equal(xy[want >= 0], stacked[want[want >= 0]])
    assert not xy[m0:m0p].any()   # the gap rows: zeros, finite


def test_coincidence_counts_inside_a_process_only(shim):
    m0, m1 = 70, 300
    pc0, pc1 = _pc(m0, 3), _pc(m1, 4)
    pc1[17] = pc0[3]   # the two processes at one location: two random variables
    rows = 128 + m1

    def stop(mask_rows=()):
        _, _, row_of, _ = plan(shim, pc0, pc1, 1)
        mask = np.zeros(rows, np.uint8)
        mask[m0:128] = 2
        for c in mask_rows:
            mask[row_of[c]] = 1
        return int(shim.shim_pair_coincident(_dp(pc0), LL(m0), _dp(pc1), LL(m1), 1, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))), row_of

    assert stop()[0] == -1
    pc1[200] = pc1[17]
    s, row_of = stop()
    assert s == max(row_of[m0 + 17], row_of[m0 + 200])   # the later of the two in the internal (Hilbert) order
    assert stop(mask_rows=[m0 + 200])[0] == -1           # one of them deflated: nothing stops
    pc0[60] = pc0[3]
    assert stop()[0] == 60                               # process 0's rows come first


def test_pair_planner_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_pair_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_pair_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- the Python layer's argument checks -----------------------------------------------------------------------------------
class _NoDevice(joint_prediction.Predictor):
    """the checks must raise before the resident factor is asked for"""

    def _factored_handle(self):
        raise AssertionError("device touched before the input was validated")


class _Field:
    def __init__(self, n):
        self.coords_main = np.zeros((n, 2))
        self.values_main = np.zeros(n)
        self.timestamp = "2020-07-01"


class _MF:
    def __init__(self, fields):
        self.fields = fields
        self.n_procs = len(fields)


def _mod(n):
    return type("Mod", (), {"n_procs": n})()


@pytest.fixture
def pred():
    return _NoDevice(_mod(2), _MF([_Field(5), _Field(5)]))


@pytest.mark.parametrize("pairs", [[0, 1], [[0, 1, 2]], [[0.0, 1.0]], [[10, 0]], [[0, 7]], [[-1, 0]]])
def test_predict_pair_bad_pairs(pred, pairs):
    with pytest.raises(ValueError, match="pairs"):
        pred.predict_pair(_pc(10), _pc(7, 1), pairs=np.array(pairs), postprocess=False)


def test_predict_pair_bad_sites_and_models(pred):
    with pytest.raises(ValueError, match="pcoords"):
        pred.predict_pair(np.zeros((0, 2)), postprocess=False)
    with pytest.raises(ValueError, match="pcoords1"):
        pred.predict_pair_arrays(_pc(4), np.zeros((0, 2)))
    with pytest.raises(ValueError, match="pcoords"):
        pred.predict_pair(np.zeros((4, 1)), postprocess=False)
    one = _NoDevice(_mod(1), _MF([_Field(5)]))
    with pytest.raises(ValueError, match="two processes"):
        one.predict_pair(_pc(4), postprocess=False)
    with pytest.raises(ValueError, match="two processes"):
        one.conditional_simulation((0, 1), _pc(4), 3)
    tr = _NoDevice(_mod(2), _MF([_Field(5), _Field(5)]), trend="constant")
    with pytest.raises(NotImplementedError, match="joint prediction of both processes is simple cokriging only"):
        tr.predict_pair(_pc(4))
    with pytest.raises(NotImplementedError, match="simple cokriging only"):
        tr.conditional_simulation((0, 1), _pc(4), 3)


@pytest.mark.parametrize("i", [(1, 0), (0, 0), (0, 1, 1), (0,), (False, True)])
def test_joint_simulation_wants_the_pair_0_1(pred, i):
    with pytest.raises(ValueError, match="process index"):
        pred.conditional_simulation(i, _pc(6), 3)


def test_joint_simulation_argument_checks(pred):
    with pytest.raises(ValueError, match="n_draws"):
        pred.conditional_simulation((0, 1), _pc(6), 0)
    with pytest.raises(ValueError, match="tol and jitter"):
        pred.conditional_simulation((0, 1), _pc(6), 3, jitter=-1.0)
    with pytest.raises(ValueError, match=r"noise has shape \(3, 6\), expected \(n_draws, m\) = \(3, 10\)"):
        pred.conditional_simulation((0, 1), _pc(6), 3, noise=np.zeros((3, 6)), pcoords1=_pc(4, 1))
    with pytest.raises(ValueError, match="seed"):
        pred.conditional_simulation((0, 1), _pc(6), 3, seed=-1)
    with pytest.raises(ValueError, match="pcoords1 belongs to the joint form"):
        pred.conditional_simulation(0, _pc(6), 3, pcoords1=_pc(4))
    # the limit counts the distinct sites of both processes
    lat, lon = np.meshgrid(np.arange(129) * 0.01, np.arange(256) * 0.01, indexing="ij")
    pc = np.column_stack([lat.ravel(), lon.ravel()])   # 33 024 sites each
    with pytest.raises(ValueError, match="33024 \\+ 33024 distinct prediction sites"):
        pred.conditional_draws_arrays((0, 1), pc, 1)


class _FakeHandle:
    """records what reaches the device layer"""

    def __init__(self, n_pad):
        self.n_pad, self.calls = n_pad, []

    def num_panels(self):
        return 1, 512, self.n_pad

    def predict_pair(self, pc0, pc1, pairs=None):
        self.calls.append((len(pc0), len(pc1), None if pairs is None else np.array(pairs)))
        cov = None if pairs is None else pc0[pairs[:, 0], 0] * pc1[pairs[:, 1], 1]
        return pc0[:, 0].copy(), np.ones(len(pc0)), pc1[:, 1].copy(), np.full(len(pc1), 2.0), cov

    def pair_timings(self):
        return {}


def test_predict_pair_chunks_both_sets_at_the_same_indices():
    P = joint_prediction.Predictor(_mod(2), _MF([_Field(5), _Field(5)]))
    h = _FakeHandle(n_pad=512)
    P._factored_handle = lambda: h
    pc = _pc(3000, 9)
    p0, e0, p1, e1, cov = P.predict_pair_arrays(pc)
    assert len(h.calls) == 1 and np.array_equal(h.calls[0][2], np.column_stack([np.arange(3000)] * 2))
    P.rhs_budget_bytes = 1    # the floor: 1024 rows a sweep -> 479 sites of each process
    h.calls.clear()
    q0, f0, q1, f1, cov2 = P.predict_pair_arrays(pc)
    assert [c[:2] for c in h.calls] == [(479, 479)] * 6 + [(126, 126)]
    assert all(np.array_equal(c[2], np.column_stack([np.arange(c[0])] * 2)) for c in h.calls)
    assert np.array_equal(p0, q0) and np.array_equal(p1, q1) and np.array_equal(cov, cov2)
    # sets of different sizes: the shorter one runs out first
    h.calls.clear()
    r = P.predict_pair_arrays(pc[:1000], pc[:100])
    assert [c[:2] for c in h.calls] == [(479, 100), (479, 0), (42, 0)] and r[4] is None
    assert np.array_equal(r[0], pc[:1000, 0]) and np.array_equal(r[2], pc[:100, 1])
    with pytest.raises(ValueError, match="rhs_budget_bytes = 1"):
        P.predict_pair_arrays(pc[:1000], pc[:100], pairs=np.array([[0, 0]]))


def test_predict_pair_frame_and_postprocess():
    at = [dict(scale_fact=2.0, spatial_mean=1.0, temporal_trend=0.5, covariate_means=[0.0, 0.0], covariate_scales=[1.0, 1.0]),
          dict(scale_fact=3.0, spatial_mean=-1.0, temporal_trend=0.25, covariate_means=[0.0, 0.0], covariate_scales=[1.0, 1.0])]

    class _Zero:
        def predict(self, X):
            return np.zeros(len(X))

    fields = [_Field(5), _Field(5)]
    for f, a in zip(fields, at):
        a["spatial_model"] = _Zero()
        f.ds = type("DS", (), {"attrs": a})()
    P = joint_prediction.Predictor(_mod(2), _MF(fields))
    h = _FakeHandle(n_pad=512)
    P._factored_handle = lambda: h
    pc = _pc(6, 2)
    raw = P.predict_pair(pc, postprocess=False)
    out = P.predict_pair(pc, postprocess=True)
    if joint_prediction.xr is not None:
        raw, out = raw.to_dataframe(), out.to_dataframe().reset_index().set_index(["lon", "lat"]).loc[list(zip(pc[:, 1], pc[:, 0]))]
    assert list(raw.columns) == ["pred_0", "pred_err_0", "pred_1", "pred_err_1", "pred_cov", "pred_corr"]
    assert np.array_equal(raw["pred_cov"].values, pc[:, 0] * pc[:, 1])
    assert np.allclose(raw["pred_corr"].values, pc[:, 0] * pc[:, 1] / 2.0, rtol=1e-15)
    assert np.allclose(out["pred_0"].values, 2.0 * pc[:, 0] + 1.5) and np.allclose(out["pred_1"].values, 3.0 * pc[:, 1] - 0.75)
    assert np.allclose(out["pred_err_0"].values, 2.0) and np.allclose(out["pred_err_1"].values, 6.0)
    assert np.allclose(out["pred_cov"].values, 6.0 * raw["pred_cov"].values)
    assert np.allclose(out["pred_corr"].values, raw["pred_corr"].values)
    # explicit pairs: the covariances come back beside the frame, scaled the same way
    res, cov = P.predict_pair(pc, pairs=np.array([[0, 5], [3, 3]]), postprocess=True)
    assert np.allclose(cov, 6.0 * np.array([pc[0, 0] * pc[5, 1], pc[3, 0] * pc[3, 1]]))
    # two site sets: one output per process
    a, b = P.predict_pair(pc, pc[:4], postprocess=False)
    if joint_prediction.xr is None:
        assert isinstance(a, pd.DataFrame) and list(a.columns) == ["pred", "pred_err"] and len(a) == 6 and len(b) == 4
