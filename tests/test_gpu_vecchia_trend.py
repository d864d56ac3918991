"""GPU tests of the Vecchia likelihood with a GLS trend: include/cokrige.h ck_loglik_vecchia_trend / _trend_grad /
ck_debug_vecchia_trend, native.Handle.loglik_vecchia_trend*, vecchia.Vecchia(trend=..., trend_likelihood=...) and
MultivariateMatern.log_likelihood / vecchia_terms / information / fit_likelihood(vecchia=...).

The problem is that of tests/test_gpu_vecchia.py -- vecchia_ref.half_colocated_sites(150), SET_B_UNIT, Euclidean distance, ranks
default_rng(11).permutation(300) -- with a known X gamma ("linear" design, p = 6) added to the values.
A. capped sets (4,4), (16,16), (32,32) at max_dist 0.5, "constant" and "linear", against the numpy loop of
   tests/vecchia_trend_ref.py;  B. exactness under full conditioning on 40 + 25 = 65 data: ck_loglik_reml / ck_predict_universal
   on a second handle and numpy dense GLS, two orderings;  C. invariance under z -> z + X gamma;  D. the gradient;  E. one process,
   haversine, measurement-error variances;  F. repeatability and state;  G. refusals;  H. the Python layer and the fits.
Per datum mu_t, s_t^2 and the p dots g_tj are held to the local path's own tolerances (tests/test_gpu_local.py): rtol 1e-8,
atol 1e-10.  Every sum is held to the bound those per-datum tolerances propagate to it from the reference's own terms
(vecchia_trend_ref.bounds, the method of vecchia_ref.totals_bound); beta to |A^-1| (|db| + |dA| |beta|).  b and A are not outputs
of the call: they are recovered as A = Cov(beta)^-1, b = A beta (cond(A) is below 50: the recovery costs 1e-14, the bounds are
1e-7 and more)."""
import ctypes

import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import vecchia_grad_ref as vgr
from tests import vecchia_ref as vr
from tests import vecchia_trend_ref as vtr

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10
TOL_GRAD = 1e-6   # tests/test_gpu_vecchia_grad.py
GAMMA = np.array([0.7, -0.4, 0.25, -1.1, 0.3, 0.5])
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_handle(native, params, metric, coords, values, F=None):
    h = native.Handle(0)
    pv = list(params)
    if len(coords) == 2:
        h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    else:
        h.set_model(1, pv[0:1], pv[1:2], pv[2:3], pv[3:4])
    h.set_metric(metric)
    for k in range(len(coords)):
        h.set_data(k, coords[k], values[k])
        if F is not None:
            h.set_trend(k, F[k])
    return h


def with_trend(coords, values):
    """the values with the known linear trend added; (values, X_linear)"""
    X, _ = vtr.design("linear", coords)
    z = np.concatenate(values) + X @ GAMMA[:X.shape[1]]
    n0 = len(values[0])
    return ([z[:n0], z[n0:]] if len(values) == 2 else [z]), X


def problem():
    if "pb" not in _cache:
        from sif_xco2_cokriging_amd import synth
        coords, plain = vr.half_colocated_sites(150)
        values, _ = with_trend(coords, plain)
        _cache["pb"] = dict(coords=coords, values=values, plain=plain, params=list(synth.SET_B_UNIT), metric=EUC,
                            ranks=np.random.default_rng(11).permutation(300).astype(np.int64))
    return _cache["pb"]


def small_problem():
    """40 + 25 = 65 data: under full conditioning the last datum's set has 64"""
    if "small" not in _cache:
        from sif_xco2_cokriging_amd import synth
        coords, plain = vr.half_colocated_sites(150)
        coords, plain = [coords[0][:40], coords[1][:25]], [plain[0][:40], plain[1][:25]]
        values, _ = with_trend(coords, plain)
        _cache["small"] = dict(coords=coords, values=values, plain=plain, params=list(synth.SET_B_UNIT), metric=EUC)
    return _cache["small"]


def reference(pb, trend, max_dist, caps, ranks=None, noise=None, key=None):
    """computed once per case and left unchanged"""
    k = ("ref", id(pb), trend if isinstance(trend, str) else id(trend), max_dist, caps, key)
    if k not in _cache:
        X, F = vtr.design(trend, pb["coords"])
        ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], X, pb["metric"],
                                          pb["ranks"] if ranks is None else ranks, max_dist, caps, noise=noise)
        assert ref["gap"].min() > 1e-9, (caps, ref["gap"].min())   # numpy and the device agree on every set
        ref["F"] = F
        ref["prior"] = np.diag(vtr.joint_cov(pb["params"], pb["coords"], pb["metric"])).copy()
        ref["own"] = np.zeros(len(ref["z"])) if noise is None else np.concatenate(
            [np.zeros(len(c)) if d is None else d for c, d in zip(pb["coords"], noise)])
        _cache[k] = ref
    return _cache[k]


def check_case(h, pb, ref, max_dist, label, ranks=None):
    """the per-datum solves, then the value call in both forms against the reference within the propagated bounds"""
    ranks = pb["ranks"] if ranks is None else ranks
    mu, vv, g = h.debug_vecchia_trend(ranks, max_dist)
    solved = ref["count"].sum(axis=1) > 0
    assert np.all(mu[~solved] == 0.0) and np.all(vv[~solved] == 0.0) and np.all(g[~solved] == 0.0)
    s2 = (ref["prior"] + ref["own"]) - vv
    print(f"{label}: max |dmu| {np.max(np.abs(mu - ref['mean'])):.2e}, max rel ds2 {np.max(np.abs(s2 - ref['var']) / ref['var']):.2e}, "
          f"max |dg| {np.max(np.abs(g - ref['g'])):.2e}")
    np.testing.assert_allclose(mu, ref["mean"], rtol=RTOL, atol=ATOL, err_msg=label)
    np.testing.assert_allclose(s2, ref["var"], rtol=RTOL, atol=ATOL, err_msg=label)
    np.testing.assert_allclose(g, ref["g"], rtol=RTOL, atol=ATOL, err_msg=label)
    B = vtr.bounds(ref, RTOL, ATOL)
    out5, beta, cov, info, st = h.loglik_vecchia_trend(ranks, max_dist, terms=True)
    assert info == 0 and np.array_equal(st["count"], ref["count"]), label
    assert np.array_equal(st["var"], s2), label                      # the terms see the solve's v . v
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"]), label
    A = np.linalg.inv(cov)
    b = A @ beta
    print(f"{label}: out5 - ref {out5 - ref['out5']}, bounds l {B['l']:.2e} s1 {B['s1']:.2e} Q {B['Q']:.2e} yy {B['yy']:.2e}; "
          f"|dbeta| {np.linalg.norm(beta - ref['beta']):.2e} bound {B['beta']:.2e}; cond(A) {np.linalg.cond(ref['A']):.1f}")
    for k, key in enumerate(("l", "s1", "logdetA", "Q", "yy")):
        assert abs(out5[k] - ref["out5"][k]) <= B[key], (label, key, out5[k], ref["out5"][k], B[key])
    assert np.all(np.abs(b - ref["b"]) <= B["b"] + 1e-12 * np.abs(ref["b"])), (label, b, ref["b"], B["b"])
    assert np.all(np.abs(A - ref["A"]) <= B["A"] + 1e-12 * np.abs(ref["A"])), (label, A - ref["A"], B["A"])
    assert np.linalg.norm(beta - ref["beta"]) <= B["beta"], (label, beta, ref["beta"], B["beta"])
    assert np.array_equal(cov, cov.T) and np.linalg.norm(cov - ref["cov"]) <= B["cov"], (label, cov, ref["cov"], B["cov"])
    # the conditional mean under the fitted trend: mu_t + f_t . beta
    tm = ATOL + RTOL * np.abs(ref["mean"]) + (ATOL + RTOL * np.abs(ref["g"])) @ np.abs(ref["beta"]) + np.abs(ref["f"]).sum(axis=1) * B["beta"]
    assert np.all(np.abs(st["mean"] - ref["mean_trend"]) <= tm), label
    # the restricted form: the same sums, another total
    out5r, betar, covr, infor, _ = h.loglik_vecchia_trend(ranks, max_dist, reml=True)
    assert infor == 0 and np.array_equal(out5r[1:], out5[1:]) and np.array_equal(betar, beta) and np.array_equal(covr, cov)
    assert abs(out5r[0] - ref["out5_reml"][0]) <= B["l_reml"], (label, out5r[0], ref["out5_reml"][0], B["l_reml"])
    assert out5r[0] != out5[0]
    return out5, beta, cov, st


# ---------------------------------------------------------------------------------------------------------------------
# A. capped sets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(native):
    pb = problem()
    hs = {"none": make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])}
    for trend in ("constant", "linear"):
        hs[trend] = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], vtr.design(trend, pb["coords"])[1])
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("trend", ["constant", "linear"])
@pytest.mark.parametrize("caps", [(4, 4), (16, 16), (32, 32)])
def test_capped_sets(handles, trend, caps):
    pb = problem()
    ref = reference(pb, trend, 0.5, caps)
    assert ref["k_max"] == {4: 8, 16: 32, 32: 64}[caps[0]] and ref["n_empty"] == 3 and ref["p"] == {"constant": 2, "linear": 6}[trend]
    h = handles[trend]
    h.set_local_neighbours(*caps)
    out5, beta, cov, st = check_case(h, pb, ref, 0.5, f"{trend} caps {caps}")
    handles["none"].set_local_neighbours(*caps)
    out3, info, plain = handles["none"].loglik_vecchia(pb["ranks"], 0.5, terms=True)
    assert info == 0
    assert np.array_equal(st["count"], plain["count"]) and np.array_equal(st["var"], plain["var"])   # bit for bit
    assert out5[1] == out3[1]                                        # and so is the sum of the log variances
    t = h.vecchia_trend_timings()
    assert t["n_data"] == 300 and t["p"] == ref["p"] and t["grad_ms"] == 0.0
    assert t["select_ms"] > 0 and t["solve_ms"] > 0 and t["terms_gram_ms"] > 0 and t["total_ms"] > 0
    tv = h.vecchia_timings()
    assert tv["n_lds"] == 300 and tv["n_tiled"] == 0 and tv["select_ms"] == t["select_ms"]


# ---------------------------------------------------------------------------------------------------------------------
# B. exactness under full conditioning
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trend", ["constant", "linear"])
def test_full_conditioning_is_dense_gls(native, trend):
    from sif_xco2_cokriging_amd import vecchia
    pb = small_problem()
    X, F = vtr.design(trend, pb["coords"])
    dense = vtr.dense_gls(pb["params"], pb["coords"], pb["values"], X, EUC)
    h2 = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], F)
    h2.assemble_joint()
    assert h2.factor() == 0
    _, _, beta2, cov2 = h2.predict_universal(0, pb["coords"][0][:3], F[0][:3])
    h2.assemble_joint()
    info2, out4, _ = h2.loglik_reml(False)
    assert info2 == 0
    h2.close()
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], F)
    h.set_local_neighbours(0, 0)
    for ordering in ("random", "hilbert"):
        ranks = vecchia.ordering_ranks(pb["coords"], ordering, 1)
        ref = reference(pb, trend, 2.0, (0, 0), ranks=ranks, key=ordering)   # 2.0: above the domain's diameter
        assert ref["k_max"] == 64 and ref["n_empty"] == 1
        out5, beta, cov, _ = check_case(h, pb, ref, 2.0, f"full conditioning {trend} {ordering}", ranks=ranks)
        out5r = h.loglik_vecchia_trend(ranks, 2.0, reml=True)[0]
        B = vtr.bounds(ref, RTOL, ATOL)
        for k, key in enumerate(("l", "s1", "logdetA", "Q", "yy")):   # numpy dense GLS
            assert abs(out5[k] - dense["out5"][k]) <= B[key], (ordering, key, out5[k], dense["out5"][k], B[key])
        assert abs(out5r[0] - dense["out5_reml"][0]) <= B["l_reml"]
        for k, key in enumerate(("l_reml", "s1", "logdetA", "Q")):    # ck_loglik_reml on the second handle
            assert abs(out5r[k] - out4[k]) <= B[key], (ordering, key, out5r[k], out4[k], B[key])
        for want in (dense["beta"], beta2):                           # ck_predict_universal's beta and its covariance
            assert np.linalg.norm(beta - want) <= B["beta"], (ordering, beta, want, B["beta"])
        for want in (dense["cov"], cov2):
            assert np.linalg.norm(cov - want) <= B["cov"], (ordering, cov, want, B["cov"])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. invariance
# ---------------------------------------------------------------------------------------------------------------------
def test_adding_a_trend_to_the_data_moves_beta_only(native, handles):
    pb = problem()
    caps = (16, 16)
    ref = reference(pb, "linear", 0.5, caps)
    if "plain" not in _cache:
        _cache["plain"] = dict(pb, values=pb["plain"])
    B1, B2 = vtr.bounds(ref, RTOL, ATOL), vtr.bounds(reference(_cache["plain"], "linear", 0.5, caps), RTOL, ATOL)
    B = {key: B1[key] + B2[key] for key in ("l", "s1", "Q", "beta")}   # either call within its own bound of the same number
    F = vtr.design("linear", pb["coords"])[1]
    hp = make_handle(native, pb["params"], EUC, pb["coords"], pb["plain"], F)        # z - X gamma
    for h in (hp, handles["linear"], handles["none"]):
        h.set_local_neighbours(*caps)
    a = handles["linear"].loglik_vecchia_trend(pb["ranks"], 0.5)
    b = hp.loglik_vecchia_trend(pb["ranks"], 0.5)
    hp.close()
    assert a[3] == b[3] == 0
    for k, key in ((0, "l"), (1, "s1"), (3, "Q")):
        assert abs(a[0][k] - b[0][k]) <= B[key], (key, a[0][k], b[0][k], B[key])
    assert a[0][1] == b[0][1]                                         # the variances do not see the values
    assert np.linalg.norm((a[1] - b[1]) - GAMMA) <= B["beta"], (a[1] - b[1], GAMMA, B["beta"])
    zero_mean = handles["none"].loglik_vecchia(pb["ranks"], 0.5)[0]
    print(f"profile value {a[0][0]:.3f}, zero-mean Vecchia value on the same data {zero_mean[0]:.3f}")
    assert a[0][0] > zero_mean[0] + 10.0                             # the trend is in the data


# ---------------------------------------------------------------------------------------------------------------------
# D. the gradient
# ---------------------------------------------------------------------------------------------------------------------
def grad_reference(pb, ref):
    """vecchia_grad_reference on the residual z - X beta_ref, on the reference's sets"""
    key = ("grad", id(ref))
    if key not in _cache:
        r = ref["z"] - ref["X"] @ ref["beta"]
        n0 = len(pb["coords"][0])
        rv = [r[:n0], r[n0:]]
        base = vr.vecchia_reference(pb["params"], pb["coords"], rv, pb["metric"], None, None,
                                    sets=(ref["keep"], ref["gap"], np.zeros(len(r), dtype=bool)))
        if ("dS", id(pb)) not in _cache:
            _cache["dS", id(pb)] = vgr.derivative_matrices(pb["params"], pb["coords"], pb["metric"])
        _cache[key] = vgr.vecchia_grad_reference(pb["params"], pb["coords"], rv, pb["metric"], base, dS=_cache["dS", id(pb)])
    return _cache[key]


@pytest.mark.parametrize("trend,caps", [("linear", (16, 16)), ("constant", (32, 32))])
def test_gradient_of_the_profiled_value(handles, trend, caps):
    pb = problem()
    ref = reference(pb, trend, 0.5, caps)
    want = grad_reference(pb, ref)
    h = handles[trend]
    h.set_local_neighbours(*caps)
    value = h.loglik_vecchia_trend(pb["ranks"], 0.5)
    out5, beta, cov, grad, info, st = h.loglik_vecchia_trend_grad(pb["ranks"], 0.5, scores=True)
    assert info == 0 and np.array_equal(out5, value[0]) and np.array_equal(beta, value[1]) and np.array_equal(cov, value[2])
    eg = vgr.measure(grad[:11], want["grad13"][:11])
    es = vgr.measure(st["score"][:, :11], want["score"][:, :11])
    print(f"{trend} caps {caps}: gradient measure max {eg.max():.2e}, score measure max {es.max():.2e}")
    assert eg.max() < TOL_GRAD and es.max() < TOL_GRAD, (grad, want["grad13"])
    assert np.all(grad[11:] == 0.0) and np.all(st["score"][:, 11:] == 0.0)
    # central differences of the numpy profile value on the same sets
    x0 = np.array(pb["params"], dtype=float)
    for k in (0, 3, 6, 9, 10):
        e = 1e-5 * max(abs(x0[k]), 1.0)
        f = []
        for sgn in (1.0, -1.0):
            x = x0.copy()
            x[k] += sgn * e
            f.append(vtr.profile_value(x, pb["coords"], pb["values"], ref["X"], EUC, ref["keep"]))
        fd = (f[0] - f[1]) / (2 * e)
        assert vgr.measure(grad[k], fd) < TOL_GRAD, (k, grad[k], fd)
    t = h.vecchia_trend_timings()
    assert t["grad_ms"] > 0 and t["solve_ms"] > 0 and t["p"] == ref["p"]
    # masked slots are exact zeros and the live slots keep their bits
    free = np.ones(13, dtype=bool)
    free[[1, 5, 10]] = False
    out5m, _, _, gm, infom, stm = h.loglik_vecchia_trend_grad(pb["ranks"], 0.5, free=free, scores=True)
    assert infom == 0 and np.array_equal(out5m, out5)
    assert np.all(gm[~free] == 0.0) and np.all(stm["score"][:, ~free] == 0.0)
    live = free.copy()
    live[11:] = False
    assert np.array_equal(gm[live], grad[live]) and np.array_equal(stm["score"][:, live], st["score"][:, live])


# ---------------------------------------------------------------------------------------------------------------------
# E. one process, haversine, measurement-error variances
# ---------------------------------------------------------------------------------------------------------------------
def test_univariate_model(native):
    pb = problem()
    coords, plain = pb["coords"][:1], pb["plain"][:1]
    values, _ = with_trend(coords, plain)
    uni = dict(coords=coords, values=values, params=[1.0, 1.5, 0.2, 0.02], metric=EUC,
               ranks=np.random.default_rng(12).permutation(150).astype(np.int64))
    _cache["uni"] = uni
    ref = reference(uni, "linear", 0.5, (8,))
    ref = dict(ref, count=np.column_stack([ref["count"][:, 0], np.zeros(150, dtype=np.int64)]))
    assert ref["p"] == 3
    h = make_handle(native, uni["params"], EUC, coords, values, ref["F"])
    h.set_local_neighbours(8, 0)
    _, beta, _, _ = check_case(h, uni, ref, 0.5, "univariate linear")
    out5, _, _, grad, info, _ = h.loglik_vecchia_trend_grad(uni["ranks"], 0.5)
    assert info == 0 and np.all(np.isfinite(grad[:4])) and np.all(grad[4:] == 0.0)
    h.close()


def test_haversine(native):
    """the problem of tests/test_gpu_vecchia.py: test_haversine, a constant per process added to its values"""
    from sif_xco2_cokriging_amd import synth
    rng = np.random.default_rng(4102)
    c0, c1 = synth.split_sites(np.column_stack([rng.uniform(30.0, 38.0, 225), rng.uniform(-105.0, -95.0, 225)]), 150)
    pb = dict(coords=[c0, c1], values=[rng.standard_normal(150) + 2.0, rng.standard_normal(150) - 1.0], params=list(synth.SET_A),
              metric=HAV, ranks=np.random.default_rng(13).permutation(300).astype(np.int64))
    _cache["hav"] = pb
    D, _ = vr.stacked_distances(pb["coords"], HAV)
    assert np.min(np.abs(D - 250.0)) > 1e-9 * 250.0                 # no pair on the radius itself
    ref = reference(pb, "constant", 250.0, (12, 12))
    assert ref["n_capped"] > 0
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"], ref["F"])
    h.set_local_neighbours(12, 12)
    check_case(h, pb, ref, 250.0, "haversine constant")
    h.close()


def test_measurement_error_variances(native):
    pb = problem()
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(150)
    ref = reference(pb, "constant", 0.5, (16, 16), noise=[2.0 * d0, None], key="noise")
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], ref["F"])
    h.set_noise(0, d0, 2.0)                                          # d > 0 on process 0 only, scale 2
    h.set_local_neighbours(16, 16)
    check_case(h, pb, ref, 0.5, "noise on process 0")
    assert np.all(ref["var"][:150] > reference(pb, "constant", 0.5, (16, 16))["var"][:150])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# F. repeatability and state
# ---------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_give_the_same_bits(handles):
    pb = problem()
    h = handles["linear"]
    h.set_local_neighbours(16, 16)
    a = h.loglik_vecchia_trend(pb["ranks"], 0.5, terms=True)
    b = h.loglik_vecchia_trend(pb["ranks"], 0.5, terms=True)
    for k in range(3):
        assert np.array_equal(a[k], b[k])
    for key in ("mean", "var", "count"):
        assert np.array_equal(a[4][key], b[4][key])
    ga = h.loglik_vecchia_trend_grad(pb["ranks"], 0.5, scores=True)
    gb = h.loglik_vecchia_trend_grad(pb["ranks"] * 5 - 3, 0.5, scores=True)     # any distinct integers: only their order counts
    assert np.array_equal(ga[3], gb[3]) and np.array_equal(ga[5]["score"], gb[5]["score"]) and np.array_equal(ga[0], a[0])


def test_a_trend_call_leaves_the_factor_and_the_predictions(native):
    pb = problem()
    pc = np.random.default_rng(5).random((40, 2))
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.assemble_joint()
    assert h.factor() == 0
    before = h.predict(0, pc)
    for k, F in enumerate(vtr.design("linear", pb["coords"])[1]):   # a new trend needs no new factorisation
        h.set_trend(k, F)
    h.set_local_neighbours(16, 16)
    out5, _, _, info, _ = h.loglik_vecchia_trend(pb["ranks"], 0.5)
    assert info == 0 and np.isfinite(out5).all()
    assert h.loglik_vecchia_trend_grad(pb["ranks"], 0.5)[4] == 0
    after = h.predict(0, pc)                                         # no new assembly, no new factorisation
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# G. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(native, handles):
    pb = problem()
    ranks = pb["ranks"]
    h = handles["constant"]
    h.set_local_neighbours(33, 32)                                   # one datum more than the LDS solver takes
    for call in (h.loglik_vecchia_trend, h.loglik_vecchia_trend_grad, h.debug_vecchia_trend):
        with pytest.raises(native.NativeError, match=r"conditioning set of more than 64 data \(the largest: 65\)"):
            call(ranks, 0.5)
    assert h.timings()["local_select_ms"] > 0                        # refused after the select passes
    h.set_local_neighbours(16, 16)
    for call in (h.loglik_vecchia, h.loglik_vecchia_grad, h.loglik_vecchia_fisher):   # the trend-free entry points: as before
        with pytest.raises(native.NativeError, match="a trend of 2 columns is set on the handle"):
            call(ranks, 0.5)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(native.NativeError, match="max_dist must be finite and >= 0"):
            h.loglik_vecchia_trend(ranks, bad)
    dup = ranks.copy()
    dup[200] = dup[17]
    with pytest.raises(native.NativeError, match=r"data 17 and 200 \(stacked order\) have the same rank"):
        h.loglik_vecchia_trend(dup, 0.5)
    L = native.lib()
    out5, g13, inf = np.zeros(5), np.zeros(13), ctypes.c_int64(0)
    rp = ranks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    none6 = (None,) * 6
    assert L.ck_loglik_vecchia_trend(h._h, None, 0.5, 0, native._p(out5), *none6, ctypes.byref(inf)) != 0
    assert "ck_loglik_vecchia_trend: null rank_host / out5" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia_trend(h._h, rp, 0.5, 0, None, *none6, ctypes.byref(inf)) != 0
    assert "null rank_host / out5" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia_trend(h._h, rp, 0.5, 0, native._p(out5), *none6, None) == 0   # every other output is optional
    assert np.isfinite(out5).all()
    assert L.ck_loglik_vecchia_trend_grad(h._h, rp, 0.5, None, native._p(out5), None, None, None, None, None, None) != 0
    assert "ck_loglik_vecchia_trend_grad: null rank_host / out5 / grad13" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia_trend_grad(h._h, rp, 0.5, None, native._p(out5), None, None, native._p(g13), None, None, None) == 0
    assert L.ck_debug_vecchia_trend(h._h, rp, 0.5, None, None, None) != 0
    assert "null rank_host / mu_host / vv_host / g_host" in L.ck_last_error().decode()

    def repeated(k, c):                                              # process 1: its third column is its first again
        one = np.ones(len(c))
        return np.column_stack([one, c[:, 0]]) if k == 0 else np.column_stack([one, c[:, 1], one])
    hd = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], vtr.design(repeated, pb["coords"])[1])
    hd.set_local_neighbours(16, 16)
    for call in (hd.loglik_vecchia_trend, hd.loglik_vecchia_trend_grad):
        with pytest.raises(native.NativeError, match="the trend design is rank deficient: regressor 2 of process 1"):
            call(ranks, 0.5)
    hd.close()


def test_without_a_trend_the_call_is_the_plain_likelihood(handles):
    pb = problem()
    h = handles["none"]
    for caps in ((16, 16), (0, 0)):                                  # (0, 0) at this radius: sets beyond the LDS limit
        h.set_local_neighbours(*caps)
        out3, info, st = h.loglik_vecchia(pb["ranks"], 0.5, terms=True)
        assert caps != (0, 0) or st["k_max"] > 64
        for reml in (False, True):
            out5, beta, cov, info5, st5 = h.loglik_vecchia_trend(pb["ranks"], 0.5, reml=reml, terms=True)
            assert info5 == info == 0 and beta.size == 0 and cov.size == 0
            assert np.array_equal(out5, [out3[0], out3[1], 0.0, out3[2], out3[2]])
            for key in ("mean", "var", "count"):
                assert np.array_equal(st5[key], st[key])
    h.set_local_neighbours(16, 16)
    out3, g13, info, _ = h.loglik_vecchia_grad(pb["ranks"], 0.5)
    out5, _, _, g, info5, _ = h.loglik_vecchia_trend_grad(pb["ranks"], 0.5)
    assert info5 == info == 0 and np.array_equal(g, g13) and np.array_equal(out5, [out3[0], out3[1], 0.0, out3[2], out3[2]])


# ---------------------------------------------------------------------------------------------------------------------
# H. the Python layer and the fits
# ---------------------------------------------------------------------------------------------------------------------
def _fields(coords, values):
    from sif_xco2_cokriging_amd import fields
    return fields.MultiField([fields.Field(coords[k], values[k]) for k in range(len(coords))])


def test_log_likelihood_and_terms_equal_the_native_call(native, handles):
    from sif_xco2_cokriging_amd import model, vecchia
    pb = problem()
    mf = _fields(pb["coords"], pb["values"])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(pb["params"])
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 4)
    h = handles["linear"]
    h.set_local_neighbours(16, 12)
    kw = dict(dist_units=None, fast_dist=False)
    for form in ("profile", "reml"):
        v = vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4, trend="linear", trend_likelihood=form,
                            gradient="analytic")
        out5, beta, cov, info, st = h.loglik_vecchia_trend(ranks, 0.5, reml=form == "reml", terms=True)
        assert info == 0 and mod.log_likelihood(mf, vecchia=v, **kw) == out5[0]
        df = mod.vecchia_terms(mf, v, **kw)
        assert np.array_equal(df["mean"].values, st["mean"]) and np.array_equal(df["variance"].values, st["var"])
        assert np.array_equal(df[["n0", "n1"]].values, st["count"]) and np.array_equal(df.attrs["out3"], out5)
        assert np.array_equal(df.attrs["beta"], beta) and np.array_equal(df.attrs["beta_cov"], cov)
    vp = vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4, trend="linear", gradient="analytic")
    out5, _, _, g13, info, _ = h.loglik_vecchia_trend_grad(ranks, 0.5)
    ll, g = mod.log_likelihood(mf, vecchia=vp, gradient=True, **kw)
    assert ll == out5[0] and np.array_equal(g, g13[:11])
    with pytest.raises(NotImplementedError, match="numeric route"):
        mod.log_likelihood(mf, vecchia=v, gradient=True, **kw)       # v: the restricted form
    # the information of the profile form: I^V of the handle without the trend, together with Cov(beta)
    inf = mod.information(mf, vecchia=vp, **kw)
    plain = mod.information(mf, vecchia=vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4), **kw)
    assert np.array_equal(inf.fisher, plain.fisher) and plain.beta_cov is None
    assert np.array_equal(inf.beta_cov, h.loglik_vecchia_trend(ranks, 0.5)[2])
    with pytest.raises(native.NativeError, match="sets of at most 64 data"):
        mod.log_likelihood(mf, vecchia=vecchia.Vecchia(0.5, trend="constant"), **kw)


LEN_BOUNDS = (0.02, 2.0)   # the unit square: the default bounds of len_scale are kilometres


def fit_problem():
    """the 65 sites of small_problem with values drawn from SET_B_UNIT plus a constant per process"""
    pb = small_problem()
    truth = list(pb["params"])
    S = orc.joint_cov(orc.Params.from_flat(truth), pb["coords"], EUC)
    z = np.linalg.cholesky(S) @ np.random.default_rng(31).standard_normal(65)
    return pb["coords"], [z[:40] + 1.5, z[40:] - 0.75], truth


def test_reml_fit_with_full_conditioning_finds_the_dense_optimum(native):
    """sigma_11, len_scale_11 and nugget_11 free.  The exact restricted log-likelihood at the Vecchia-REML optimum may not be more
    than 0.005 below the exact one at the dense REML optimum (tests/test_gpu_vecchia.py:
    test_fit_with_full_conditioning_finds_the_dense_optimum: a shift of t standard errors lowers l by t^2 / 2, 0.005 is t = 0.1)."""
    from sif_xco2_cokriging_amd import model, vecchia
    coords, values, truth = fit_problem()
    mf = _fields(coords, values)
    start = list(truth)
    start[0], start[5], start[8] = 1.3, 0.3, 0.05
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    kw = dict(dist_units=None, fast_dist=False)
    results = {}
    for label, v in (("dense", None), ("vecchia", vecchia.Vecchia(2.0, ordering="random", seed=2, trend="constant",
                                                                 trend_likelihood="reml", gradient="analytic"))):
        mod = model.MultivariateMatern(2)
        mod.params.set_values(start)
        mod.params.set_bounds(len_scale=LEN_BOUNDS)
        names = list(mod.params.get_names())
        mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free], vecchia=v,
                           trend="constant" if v is None else None, **kw)
        r = mod.fit_result
        x = mod.params.get_values().astype(float)
        assert r.method == ("REML" if v is None else "Vecchia-REML") and r.n_free == 3 and r.free == free
        exact = model.MultivariateMatern(2)
        exact.params.set_values(x)
        results[label] = (x, exact.log_likelihood(mf, trend="constant", **kw), r)
        print(f"{label}: x {x[[0, 5, 8]]}, exact l_R {results[label][1]:.6f}, reported {r.loglik:.6f}, n_eval {r.n_eval}, {r.message}")
    rv = results["vecchia"][2]
    assert abs(rv.loglik - results["vecchia"][1]) < 1e-6             # full conditioning: the value is the exact one
    assert results["vecchia"][1] >= results["dense"][1] - 0.005, (results["vecchia"][:2], results["dense"][:2])
    assert rv.beta.shape == (2,) and rv.beta_cov.shape == (2, 2) and results["dense"][2].beta is None
    assert rv.information is None and rv.std_error is None


def test_profile_fit_with_the_analytic_gradient(native, monkeypatch):
    from sif_xco2_cokriging_amd import model, vecchia
    coords, values, truth = fit_problem()
    mf = _fields(coords, values)
    calls = {"value": 0, "grad": 0}
    nat = native.Handle
    value0, grad0 = nat.loglik_vecchia_trend, nat.loglik_vecchia_trend_grad
    monkeypatch.setattr(nat, "loglik_vecchia_trend", lambda self, *a, **k: (calls.__setitem__("value", calls["value"] + 1), value0(self, *a, **k))[1])
    monkeypatch.setattr(nat, "loglik_vecchia_trend_grad", lambda self, *a, **k: (calls.__setitem__("grad", calls["grad"] + 1), grad0(self, *a, **k))[1])
    start = list(truth)
    start[0], start[5], start[8] = 1.3, 0.3, 0.05
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    v = vecchia.Vecchia(2.0, ordering="random", seed=2, trend="constant", gradient="analytic", information="expected")
    mod = model.MultivariateMatern(2)
    mod.params.set_values(start)
    mod.params.set_bounds(len_scale=LEN_BOUNDS)
    names = list(mod.params.get_names())
    mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free], vecchia=v, std_errors=True,
                       dist_units=None, fast_dist=False)
    r = mod.fit_result
    assert r.method == "Vecchia-ML" and r.success and r.free == free
    assert calls["grad"] == r.n_eval + 1 and calls["value"] == 2     # one native call per evaluation; beta at the end, twice
    assert np.max(np.abs(r.gradient[[0, 5, 8]])) < 1e-3 or r.at_bound
    assert r.beta.shape == (2,) and np.all(np.isfinite(r.beta)) and r.beta_cov.shape == (2, 2)
    assert np.all(np.linalg.eigvalsh(r.beta_cov) > 0) and np.array_equal(r.information.beta_cov, r.beta_cov)
    se = r.std_error
    live = [n for n in free if n not in r.at_bound]
    assert r.information is not None and np.all(np.isfinite(se[live])) and np.all(se[live] > 0)
    # full conditioning: the profile value at the optimum is dense GLS's
    x = mod.params.get_values().astype(float)
    X, _ = vtr.design("constant", coords)
    dense = vtr.dense_gls(x, coords, values, X, EUC)
    assert abs(r.loglik - dense["out5"][0]) < 1e-6 and np.allclose(r.beta, dense["beta"], rtol=1e-6, atol=1e-8)
    assert abs(r.beta[0] - 1.5) < 4 * np.sqrt(r.beta_cov[0, 0]) and abs(r.beta[1] + 0.75) < 4 * np.sqrt(r.beta_cov[1, 1])
