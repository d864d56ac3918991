"""The gradient of the Vecchia likelihood without a GPU: the numpy reference of tests/vecchia_grad_ref.py against fourth-order
differences of tests/vecchia_ref.py's value with the sets held fixed; the score header csrc/ck_vecchia_grad.h driven serially
(tests/host_vecchia_grad.h) through a g++ shim against numpy, and in a stand-alone program under
-fsanitize=address,undefined (tests/host_vecchia_grad_sanitize_main.cpp); the validation of Vecchia(gradient=...) and the
refusals that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
sys.path.insert(0, ROOT)

from oracle import cokrige_oracle as orc   # noqa: E402
from tests import dense_chains as dc   # noqa: E402
from tests import vecchia_grad_ref as vgr   # noqa: E402
from tests import vecchia_ref as vr   # noqa: E402

EUC = 1
TOL = 1e-6   # the project's gradient measure |g - ref| / max(|ref|, 1)


def parameter_sets():
    from sif_xco2_cokriging_amd import synth
    gen = list(synth.SET_A)
    gen[5:8] = [0.2, 0.2, 0.2]                                     # generic nu on the unit square
    return {"SET_B_UNIT": list(synth.SET_B_UNIT), "GEN": gen}


# ---------------------------------------------------------------------------------------------------------------------
# (a) the reference against differences of the reference's value
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
def test_reference_gradient_equals_differences_of_the_value_with_fixed_sets(name):
    params = parameter_sets()[name]
    coords, values = vr.half_colocated_sites(30)
    ranks = np.random.default_rng(11).permutation(60)
    ref = vr.vecchia_reference(params, coords, values, EUC, ranks, 0.5, (4, 4))
    sets = (ref["keep"], ref["gap"], np.zeros(60, dtype=bool))
    assert ref["info"] == 0 and ref["n_empty"] >= 1 and ref["k_max"] == 8
    got = vgr.vecchia_grad_reference(params, coords, values, EUC, ref)
    fd = dc.fd_of(lambda y: vr.vecchia_reference(y, coords, values, EUC, ranks, 0.5, (4, 4), sets=sets)["out3"][0], params)
    err = vgr.measure(got["grad13"][:11], fd)
    print(name, "max measure", err.max())
    assert err.max() < TOL, (err, got["grad13"], fd)
    assert np.all(got["grad13"][11:] == 0.0)
    # the same through G_V and dense_chains.grad_trace
    gt = dc.grad_trace(params, coords, EUC, got["G_V"])
    assert vgr.measure(gt, got["grad13"][:11]).max() < 1e-12
    empty = np.flatnonzero(ref["count"].sum(axis=1) == 0)
    for t in empty:                                                 # an empty set: sigma_i and nugget_i only
        q = int(t >= 30)
        live = {q, 8 + q}
        assert all((got["score"][t, k] != 0.0) == (k in live) for k in range(13)), got["score"][t]


def test_reference_under_full_conditioning_is_the_dense_gradient():
    params = parameter_sets()["GEN"]
    coords, values = vr.half_colocated_sites(30)
    ranks = np.random.default_rng(11).permutation(60)
    ref = vr.vecchia_reference(params, coords, values, EUC, ranks, 10.0)
    got = vgr.vecchia_grad_reference(params, coords, values, EUC, ref)
    dense = dc.dense_ll_grad(params, coords, values, EUC)
    assert vgr.measure(got["grad13"][:11], dense).max() < 1e-10


# ---------------------------------------------------------------------------------------------------------------------
# (b) the score header on the host
# ---------------------------------------------------------------------------------------------------------------------
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vecchia_grad") / "libck_vecchia_grad.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, os.path.join(ROOT, "tests", "host_vecchia_grad_shim.cpp"),
                    os.path.join(CSRC, "ck_model.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.shim_vecchia_weights.argtypes = [ctypes.c_double] * 5 + [ctypes.c_int, _dp]
    lib.shim_vecchia_weights.restype = ctypes.c_int
    lib.shim_vecchia_score.argtypes = [ctypes.c_int, _dp, ctypes.c_uint, ctypes.c_int, _dp, _ip, _dp, _dp, _dp, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, _dp, _dp, _dp]
    lib.shim_vecchia_score.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def score_of(lib, params, coords, values, t, c, noise_d=None, scales=(1.0, 1.0), live=0x1fff):
    """the shim's score of datum t conditioned on the stacked indices c"""
    n0 = len(coords[0])
    allc = np.vstack(coords)
    z = np.concatenate(values)
    proc = (np.arange(len(z)) >= n0).astype(np.int32)
    S0 = orc.joint_cov(orc.Params.from_flat(params), coords, EUC)
    dvec = None if noise_d is None else np.concatenate(noise_d)
    S = S0 if dvec is None else S0 + np.diag(dvec * np.asarray(scales)[proc])
    ix = np.r_[c, t].astype(int)
    k = len(c)
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (allc[ix], S[np.ix_(c, c)] if k else np.zeros(1), S[c, t] if k else
                                                                np.zeros(1), z[c] if k else np.zeros(1))]
    out2, score = np.zeros(2), np.zeros(13)
    par = np.ascontiguousarray(params, dtype=np.float64)
    own = 0.0 if dvec is None else float(dvec[t] * scales[proc[t]])
    dv = None if dvec is None else np.ascontiguousarray(dvec[ix])
    rc = lib.shim_vecchia_score(2, _p(par), live, k, _p(args[0]), _p(np.ascontiguousarray(proc[ix])), _p(args[1]), _p(args[2]),
                                _p(args[3]), float(z[t]), float(S0[t, t]), own, _p(dv), _p(out2), _p(score))
    return rc, out2, score


def single_datum_reference(params, coords, values, t, c, noise_d=None, scales=(1.0, 1.0)):
    N = sum(len(x) for x in coords)
    keep = np.zeros((N, N), dtype=bool)
    keep[t, c] = True
    noise = None if noise_d is None else [scales[q] * noise_d[q] for q in range(2)]
    ref = vr.vecchia_reference(params, coords, values, EUC, np.arange(N), 0.0, noise=noise,
                               sets=(keep, np.full(N, np.inf), np.zeros(N, dtype=bool)))
    got = vgr.vecchia_grad_reference(params, coords, values, EUC, ref, noise_d=noise_d, scales=scales)
    return ref, got["score"][t]


@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("k", [0, 1, 64])
def test_score_header_against_numpy(shim, name, with_noise, k):
    params = parameter_sets()[name]
    coords, values = vr.half_colocated_sites(40)
    rng = np.random.default_rng(k)
    noise_d = [rng.uniform(0.01, 0.05, 40) for _ in range(2)] if with_noise else None
    scales = (0.7, 1.3)
    t = 45                                                          # a datum of process 1
    c = np.r_[5, rng.permutation(np.delete(np.arange(80), [5, 45]))[:k - 1]] if k else np.zeros(0, dtype=int)   # 5 is co-located with 45
    assert k == 0 or np.array_equal(coords[0][5], coords[1][5])
    c = np.sort(c)
    ref, want = single_datum_reference(params, coords, values, t, c, noise_d, scales)
    rc, out2, score = score_of(shim, params, coords, values, t, c, noise_d, scales)
    assert rc == 0
    if k:
        assert out2[0] == pytest.approx(ref["mean"][t], rel=1e-9, abs=1e-11)
        assert ref["var"][t] > 0.01
    err = vgr.measure(score, want)
    print(name, with_noise, k, "max measure", err.max())
    assert err.max() < TOL, (score, want)
    if not with_noise:
        assert score[11] == 0.0 and score[12] == 0.0
    if k == 0:
        live = {1, 9} | ({12} if with_noise else set())
        assert all((score[s] != 0.0) == (s in live) for s in range(13)), score
    mask = 0x1fff & ~(1 << 2 | 1 << 3 | 1 << 4 | 1 << 12)
    rc, _, masked = score_of(shim, params, coords, values, t, c, noise_d, scales, live=mask)
    assert rc == 0 and all(masked[s] == (score[s] if mask >> s & 1 else 0.0) for s in range(13))


def test_score_header_variance_not_positive(shim):
    params = parameter_sets()["SET_B_UNIT"]
    params[8] = params[9] = 0.0
    coords, values = vr.half_colocated_sites(40)
    coords = [coords[0].copy(), coords[1]]
    coords[0][3] = coords[0][10]                                    # a duplicate within process 0, no nugget: s^2 = 0
    rc, out2, score = score_of(shim, params, coords, values, 3, np.array([10]), live=0x7ff)
    assert rc == 1 and np.all(np.isnan(score[:11])) and np.all(score[11:] == 0.0)
    out = np.zeros(2)
    assert shim.shim_vecchia_weights(0.7, 0.2, 0.4, 1.02, 0.3, 5, _p(out)) == 0
    e, s2 = 0.5, 1.32 - 0.4
    assert out[0] == pytest.approx(e * e / s2 ** 2 - 1 / s2, rel=1e-14) and out[1] == pytest.approx(e / s2, rel=1e-14)
    assert shim.shim_vecchia_weights(0.7, np.nan, np.nan, 1.02, 0.3, 0, _p(out)) == 0      # the empty set
    assert out[1] == pytest.approx(0.7 / 1.32, rel=1e-14)
    assert shim.shim_vecchia_weights(0.7, np.nan, 0.1, 1.02, 0.0, 3, _p(out)) == 1 and np.all(np.isnan(out))


# ---------------------------------------------------------------------------------------------------------------------
# (c) the same driver under the sanitizers, in a program of its own
# ---------------------------------------------------------------------------------------------------------------------
def test_score_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_vecchia_grad_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_vecchia_grad_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_model.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------
# (d) the configuration and the refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def _model_and_fields():
    from sif_xco2_cokriging_amd import fields, model
    rng = np.random.default_rng(2)
    c = np.column_stack([rng.uniform(25, 50, 20), rng.uniform(-120, -70, 20)])
    mf = fields.MultiField([fields.Field(c, rng.standard_normal(20)) for _ in range(2)])
    return model.MultivariateMatern(2), mf


def test_gradient_option_is_validated_and_refusals_need_no_device():
    from sif_xco2_cokriging_amd import vecchia
    assert vecchia.Vecchia(0.5).gradient == "numeric"
    assert vecchia.Vecchia(0.5, max_neighbours=8, gradient="analytic").gradient == "analytic"
    for bad in ("exact", "", None, True, 1, ("analytic",)):
        with pytest.raises(ValueError, match="gradient must be one of"):
            vecchia.Vecchia(0.5, gradient=bad)
    mod, mf = _model_and_fields()
    v = vecchia.Vecchia(300.0, max_neighbours=8, gradient="analytic")
    with pytest.raises(ValueError, match="REML"):
        mod.log_likelihood(mf, vecchia=v, gradient=True, trend="constant")
    with pytest.raises(ValueError, match="REML"):
        mod.fit_likelihood(mf, vecchia=v, trend="constant")
    with pytest.raises(NotImplementedError, match="Fisher information"):
        mod.fit_likelihood(mf, vecchia=v, std_errors=True)
    for bad in (0.0, 0.5, "1e-4"):
        with pytest.raises(ValueError, match="fd_step"):
            mod.fit_likelihood(mf, vecchia=v, fd_step=bad)
    with pytest.raises(NotImplementedError, match="no analytic gradient yet"):   # the default configuration: as before
        mod.log_likelihood(mf, vecchia=vecchia.Vecchia(300.0, max_neighbours=8), gradient=True)
    assert mod._lik is None                                         # no handle was made
