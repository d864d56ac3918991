"""GPU tests of the joint prediction and co-simulation of both processes: include/cokrige.h ck_predict_pair and
ck_conditional_draws_pair, native.Handle.predict_pair / conditional_draws_pair and the Predictor's joint forms, against the
single-process calls on the same handle and a dense chain on the stacked sites (oracle covariances, scipy's dense solver,
numpy.linalg.cholesky in the pinned internal order: the sites of process 0, then those of process 1, each set along its own
Hilbert curve from 256 sites on when site_order is on).

Bounds: 1e-12 against ck_predict (the same rows through the same sweep), 1e-9 against the dense chain (the project's parity
bound), 1e-8 in units of sqrt(S_aa S_bb) for a posterior cross-covariance, 1e-8 for draws (the bound of the draws test)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAV = 0
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
N_PER = 700
SIZES = [(1, 1), (63, 65), (64, 64), (65, 63), (0, 40), (40, 0), (300, 277), (512, 130)]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def rel(a, b):
    if np.size(b) == 0:
        return 0.0
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


class Data:
    """tests/test_gpu_conditional.py's make_data: 2 x 700 data, the second half of process 0 on the first half of process 1"""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.p = orc.Params.from_flat(BIV)
        pts = np.column_stack([rng.uniform(25, 50, 2 * N_PER), rng.uniform(-120, -70, 2 * N_PER)])
        self.coords = [pts[:N_PER], pts[N_PER // 2:N_PER // 2 + N_PER]]
        self.Sigma = orc.joint_cov(self.p, self.coords, HAV)
        z = np.linalg.cholesky(self.Sigma) @ rng.standard_normal(2 * N_PER)
        self.values = [z[:N_PER], z[N_PER:]]
        self.cf = cho_factor(self.Sigma, lower=True)
        # where the data lie: both processes | process 0 only | process 1 only
        self.both = self.coords[1][:N_PER // 2]
        self.only = [self.coords[0][:N_PER // 2], self.coords[1][N_PER // 2:]]


@pytest.fixture(scope="module")
def data():
    return Data()


def handle(native, d, site_order=None):
    p = d.p
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(HAV)
    for k in range(2):
        h.set_data(k, d.coords[k], d.values[k])
    if site_order is not None:
        h.set_option("site_order", site_order)
    h.assemble_joint()
    assert h.factor() == 0
    return h


@pytest.fixture(scope="module")
def handles(native, data):
    hs = {so: handle(native, data, so) for so in (0, 1)}
    yield hs
    for h in hs.values():
        h.close()


def site_sets(d, m0, m1, seed):
    """The two site sets, shuffled: shared free sites, free sites of its own, sites on data of both processes, on data of
    its own process only and (process 0) on data of process 1 only -- 40 / rest / 5 / 15 | 10 / 3 from 63 sites on, shrunk
    in proportion below.  Returns pc0, pc1, the expected deflation masks and the co-located pairs (a, b)."""
    rng = np.random.default_rng(seed)
    m = [m0, m1]
    f = [min(1.0, mk / 63.0) for mk in m]
    shared = 0 if min(m) == 0 else max(1, int(40 * min(f)))
    free_shared = np.column_stack([rng.uniform(26, 49, shared), rng.uniform(-118, -72, shared)])
    sets, defl, where_shared = [], [], []
    for k in range(2):
        n_both, n_own = int(5 * f[k]), int((15, 10)[k] * f[k])
        n_other = int(3 * f[k]) if k == 0 else 0
        n_free = m[k] - shared - n_both - n_own - n_other
        assert n_free >= 0
        parts = [free_shared, np.column_stack([rng.uniform(26, 49, n_free), rng.uniform(-118, -72, n_free)]),
                 d.both[rng.choice(len(d.both), n_both, replace=False)],
                 d.only[k][rng.choice(len(d.only[k]), n_own, replace=False)],
                 d.only[1 - k][rng.choice(len(d.only[1 - k]), n_other, replace=False)]]
        pc = np.vstack(parts)
        on = np.zeros(m[k], dtype=bool)
        on[shared + n_free:shared + n_free + n_both + n_own] = True
        perm = rng.permutation(m[k])
        sets.append(pc[perm])
        defl.append(on[perm])
        where_shared.append(np.argsort(perm)[:shared])
    pairs = np.column_stack(where_shared).astype(np.int64) if shared else np.zeros((0, 2), dtype=np.int64)
    return sets[0], sets[1], defl[0], defl[1], pairs


def chain(d, pc0, pc1, Sigma=None, cf=None):
    """pred and S of the stacked sites: S = C_pp - c0^T Sigma^-1 c0, C_pp = [[C00, C01], [C01^T, C11]]"""
    cf = d.cf if cf is None else cf
    live = [k for k, pc in enumerate((pc0, pc1)) if len(pc)]   # (the oracle's distances take no empty set)
    c0 = np.hstack([orc.pred_cross_cov(d.p, d.coords, (pc0, pc1)[k], k, HAV) for k in live])
    pred = c0.T @ cho_solve(cf, np.concatenate(d.values))
    Cpp = orc.joint_cov(d.p, [pc0, pc1], HAV) if len(live) == 2 else orc.pred_cov(d.p, (pc0, pc1)[live[0]], live[0], HAV)
    return pred, Cpp - c0.T @ cho_solve(cf, c0)


def internal_order(native, pc0, pc1, site_order):
    """the pinned order of the stacked sites (include/cokrige.h: ck_predict_pair)"""
    def one(pc):
        return native.hilbert_order(pc) if site_order and len(pc) >= 256 else np.arange(len(pc))
    return np.concatenate([one(pc0), len(pc0) + one(pc1)]).astype(np.int64)


def chain_draws(pred, S, defl, perm, eps):
    kept = perm[~defl[perm]]
    L = np.linalg.cholesky(S[np.ix_(kept, kept)])
    x = np.zeros_like(eps)
    x[:, kept] = eps[:, kept] @ L.T
    return pred + x


@pytest.fixture(scope="module")
def cases(data):
    """every (m0, m1): the sites and the chain's pred and S, computed once"""
    out = {}
    for n, (m0, m1) in enumerate(SIZES):
        pc0, pc1, d0, d1, pairs = site_sets(data, m0, m1, 500 + n)
        pred, S = chain(data, pc0, pc1)
        out[m0, m1] = dict(pc0=pc0, pc1=pc1, defl=np.concatenate([d0, d1]), co=pairs, pred=pred, S=S)
    return out


def test_site_sets_separate_deflated_from_kept(cases):
    """The chain itself: a site on a datum of its own process has S_kk = C(0) - c0^T Sigma^-1 c0 = 0 up to the rounding of
    terms of size C(0) ~ 1 (a few ulp of 1; 16 allowed), every other site keeps at least its nugget's worth of variance, and
    the kept S is well conditioned -- so numpy's Cholesky succeeds and the expected mask is exact at tol = 1e-10."""
    for (m0, m1) in [(65, 63), (300, 277), (512, 130)]:
        c = cases[m0, m1]
        sd = np.diag(c["S"])
        assert np.array_equal(np.abs(sd) <= 16 * np.finfo(float).eps, c["defl"])
        assert c["defl"][:m0].sum() == 20 and c["defl"][m0:].sum() == 15
        assert sd[~c["defl"]].min() >= 3e-2
        assert np.linalg.cond(c["S"][np.ix_(~c["defl"], ~c["defl"])]) <= 50


@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_predict_pair_matches_predict_and_the_chain(native, handles, cases, size, site_order):
    m0, m1 = size
    c, h = cases[size], handles[site_order]
    pc0, pc1, S, defl = c["pc0"], c["pc1"], c["S"], c["defl"]
    single = [h.predict(0, pc0), h.predict(1, pc1)]
    rng = np.random.default_rng(7)
    q_rand = 50 if min(m0, m1) > 1 else min(m0, m1)
    rnd = np.column_stack([rng.integers(0, max(m0, 1), q_rand), rng.integers(0, max(m1, 1), q_rand)])
    d0, d1 = np.flatnonzero(defl[:m0]), np.flatnonzero(defl[m0:])
    on_defl = np.array([(a, b) for a in d0[:3] for b in range(min(m1, 3))] + [(a, b) for b in d1[:3] for a in range(min(m0, 3))],
                       dtype=np.int64).reshape(-1, 2)
    pairs = np.vstack([c["co"], rnd, on_defl]).astype(np.int64)
    p0, e0, p1, e1, cov = h.predict_pair(pc0, pc1, pairs)
    # against ck_predict on the same handle
    for got, want in [(p0, single[0][0]), (e0, single[0][1]), (p1, single[1][0]), (e1, single[1][1])]:
        assert rel(got, want) < 1e-12
    print("bit-identical to ck_predict:", all(np.array_equal(g, w) for g, w in
                                              [(p0, single[0][0]), (e0, single[0][1]), (p1, single[1][0]), (e1, single[1][1])]))
    # against the dense chain
    assert rel(np.concatenate([p0, p1]), c["pred"]) < 1e-9
    want_err = np.sqrt(np.maximum(np.diag(S), 0.0))
    got_err = np.concatenate([e0, e1])
    assert rel(got_err[~defl], want_err[~defl]) < 1e-9
    assert np.all(got_err[defl] < 1e-6)   # sqrt of a rounded zero
    # the posterior cross-covariances
    if len(pairs):
        want = S[pairs[:, 0], m0 + pairs[:, 1]]
        sd = np.sqrt(np.abs(np.diag(S)))
        touched = defl[pairs[:, 0]] | defl[m0 + pairs[:, 1]]
        err = np.abs(cov - want)[~touched] / (sd[pairs[:, 0]] * sd[m0 + pairs[:, 1]])[~touched]
        print("pair_cov max scaled error:", err.max() if err.size else 0.0)
        assert np.all(err < 1e-8)
        assert np.all(np.abs(cov[touched]) <= 1e-12)
    if len(c["co"]) >= 40:
        corr = cov[:40] / (e0[c["co"][:, 0]] * e1[c["co"][:, 1]])
        assert np.max(np.abs(corr)) > 0.02
    t = h.pair_timings()
    assert t["pair_sweep_ms"] > 0 and t["pair_total_ms"] > 0


@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_given_noise_matches_the_dense_chain(native, handles, cases, size, site_order):
    m0, m1 = size
    c, h = cases[size], handles[site_order]
    pc0, pc1, defl = c["pc0"], c["pc1"], c["defl"]
    m = m0 + m1
    eps = np.random.default_rng(11).standard_normal((7, m))
    p0, e0, p1, e1, _ = h.predict_pair(pc0, pc1)
    draws, pred, err, got_defl, info = h.conditional_draws_pair(pc0, pc1, 7, noise=eps)
    assert info == 0
    assert np.array_equal(pred, np.concatenate([p0, p1])) and np.array_equal(err, np.concatenate([e0, e1]))
    assert np.array_equal(got_defl, defl)
    assert np.array_equal(draws[:, defl], np.broadcast_to(pred[defl], (7, int(defl.sum()))))
    want = chain_draws(pred, c["S"], defl, internal_order(native, pc0, pc1, site_order), eps)
    assert rel(draws, want) < 1e-8
    t = h.pair_timings()
    assert t["n_deflated"] == defl.sum() and t["n_chunks"] == 1 and t["product_ms"] > 0


def host_normals(seed, m, n):
    """the normals of csrc/ck_rng.h on the host, counter = (site index, d / 2)"""
    so = os.path.join(ROOT, "tests", "_build", "libck_host_rng_pair.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_rng_shim.cpp"), "-o", so], check=True)
    eps = np.empty((n, m))
    ctypes.CDLL(so).shim_normals(ctypes.c_uint64(seed), ctypes.c_long(m), ctypes.c_long(n),
                                 eps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return eps


def test_device_noise_is_keyed_on_the_stacked_index(native, handles, cases):
    c, h = cases[300, 277], handles[1]
    pc0, pc1, defl = c["pc0"], c["pc1"], c["defl"]
    m = len(defl)
    a, pred = h.conditional_draws_pair(pc0, pc1, 40, seed=77)[:2]
    try:
        for chunk in (1, 40):
            h.set_option("draw_chunk", chunk)
            assert np.array_equal(h.conditional_draws_pair(pc0, pc1, 40, seed=77)[0], a), chunk
            assert h.pair_timings()["n_chunks"] == 40 // chunk
    finally:
        h.set_option("draw_chunk", 0)
    assert np.array_equal(h.conditional_draws_pair(pc0, pc1, 9, seed=77)[0], a[:9])
    assert not np.array_equal(h.conditional_draws_pair(pc0, pc1, 9, seed=78)[0], a[:9])
    eps = host_normals(77, m, 40)
    want = chain_draws(pred, c["S"], defl, internal_order(native, pc0, pc1, 1), np.where(defl, 0.0, eps))
    assert rel(a, want) < 1e-8


def test_sites_at_one_location(native, handles, cases):
    c, h = cases[65, 63], handles[1]
    pc0, pc1, defl = c["pc0"], c["pc1"], c["defl"]
    a, b = c["co"][0]   # both processes at one free location: two random variables, nothing stops
    assert np.array_equal(pc0[a], pc1[b]) and not defl[a] and not defl[65 + b]
    assert h.conditional_draws_pair(pc0, pc1, 2, seed=1)[4] == 0
    # the same free site twice within process 1: the later one (caller's order here: no set reaches 256 sites) is named
    dup = np.vstack([pc1, pc1[[b]]])
    draws, pred, err, got_defl, info = h.conditional_draws_pair(pc0, dup, 2, seed=1)
    assert info == 1 + 65 + 63 and not draws.any()
    assert np.array_equal(got_defl[:128], defl)
    # ... and within process 0
    dup0 = np.vstack([pc0[[a]], pc0])
    assert h.conditional_draws_pair(dup0, pc1, 2, seed=1)[4] == 1 + (a + 1)
    # twice on a datum of its own process: deflated both times, nothing stops
    k = int(np.flatnonzero(defl[:65])[0])
    assert h.conditional_draws_pair(np.vstack([pc0, pc0[[k]]]), pc1, 2, seed=1)[4] == 0


def test_with_measurement_error(native, data, cases):
    c = cases[65, 63]
    pc0, pc1 = c["pc0"], c["pc1"]
    rng = np.random.default_rng(31)
    var = [rng.uniform(0.01, 0.05, N_PER), rng.uniform(0.01, 0.05, N_PER)]
    p = data.p
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(HAV)
    for k in range(2):
        h.set_data(k, data.coords[k], data.values[k])
        h.set_noise(k, var[k], 1.5)
    h.assemble_joint()
    assert h.factor() == 0
    p0, e0, p1, e1, cov = h.predict_pair(pc0, pc1, c["co"])
    for got, want in zip([p0, e0], h.predict(0, pc0)):
        assert rel(got, want) < 1e-12
    for got, want in zip([p1, e1], h.predict(1, pc1)):
        assert rel(got, want) < 1e-12
    # the noise is in Sigma only: C_pp and c0 are those of the chain without it
    Sn = data.Sigma + np.diag(1.5 * np.concatenate(var))
    pred, S = chain(data, pc0, pc1, cf=cho_factor(Sn, lower=True))
    assert rel(np.concatenate([p0, p1]), pred) < 1e-9
    sd = np.sqrt(np.diag(S))
    a, b = c["co"][:, 0], c["co"][:, 1]
    assert np.all(np.abs(cov - S[a, 65 + b]) / (sd[a] * sd[65 + b]) < 1e-8)
    h.close()


def test_handle_state_after_a_pair_call(native, handles, cases):
    c, h = cases[300, 277], handles[1]
    before = h.predict(0, c["pc0"])
    v0 = h.verify_model()
    h.predict_pair(c["pc0"], c["pc1"])
    with pytest.raises(native.NativeError, match="ck_verify_model: the last call was ck_predict_pair"):
        h.verify_model()
    after = h.predict(0, c["pc0"])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert h.verify_model() == v0
    h.conditional_draws_pair(c["pc0"], c["pc1"], 3, seed=5)
    with pytest.raises(native.NativeError, match="the last call was ck_predict_pair"):
        h.verify_model()
    again = h.predict(0, c["pc0"])
    assert np.array_equal(before[0], again[0]) and np.array_equal(before[1], again[1])


def test_refusals(native, data, handles, cases):
    c, h = cases[65, 63], handles[1]
    pc0, pc1 = c["pc0"], c["pc1"]
    for bad in ([[65, 0]], [[0, 63]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(native.NativeError, match="ck_predict_pair: pair 0 .* out of range"):
            h.predict_pair(pc0, pc1, np.array(bad, dtype=np.int64))
    with pytest.raises(native.NativeError, match="ck_conditional_draws_pair: m0 \\+ m1 = 0"):
        h.conditional_draws_pair(np.zeros((0, 2)), np.zeros((0, 2)), 1)
    big = np.column_stack([np.linspace(26, 49, 32769), np.linspace(-118, -72, 32769)])
    with pytest.raises(native.NativeError, match="65 536"):
        h.conditional_draws_pair(big, big[:32768], 1)
    with pytest.raises(native.NativeError, match="n_draws"):
        h.conditional_draws_pair(pc0, pc1, 0)
    with pytest.raises(native.NativeError, match="tol"):
        h.conditional_draws_pair(pc0, pc1, 1, tol=-1.0)
    assert h.predict_pair(pc0, pc1)[0].shape == (65,)   # the handle is still usable
    p = data.p
    u = native.Handle(0)
    u.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    u.set_metric(HAV)
    for k in range(2):
        u.set_data(k, data.coords[k], data.values[k])
    u.assemble_joint()
    for call in (lambda: u.predict_pair(pc0, pc1), lambda: u.conditional_draws_pair(pc0, pc1, 1)):
        with pytest.raises(native.NativeError, match="ck_factor has not been called"):
            call()
    u.close()
    one = native.Handle(0)
    one.set_model(1, [p.sigma[0]], [p.nu[0, 0]], [p.len_scale[0, 0]], [p.nugget[0]])
    one.set_metric(HAV)
    one.set_data(0, data.coords[0], data.values[0])
    one.assemble_joint()
    assert one.factor() == 0
    with pytest.raises(native.NativeError, match="ck_predict_pair: needs a model of two processes"):
        one.predict_pair(pc0, pc1)
    with pytest.raises(native.NativeError, match="ck_conditional_draws_pair: needs a model of two processes"):
        one.conditional_draws_pair(pc0, pc1, 1)
    one.close()
    q = native.Handle(devices=[0, 0], rank=0)
    with pytest.raises(native.NativeError, match="ck_predict_pair .* partitioned"):
        q.predict_pair(pc0, pc1)
    with pytest.raises(native.NativeError, match="ck_conditional_draws_pair .* partitioned"):
        q.conditional_draws_pair(pc0, pc1, 1)
    q.close()


# ---- the Python layer ------------------------------------------------------------------------------------------------------
class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


class _StubTrend:
    def predict(self, X):
        X = np.asarray(X, dtype=float)
        return 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.05


@pytest.fixture(scope="module")
def predictor(native, data):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    fs = [fields.Field(data.coords[k], data.values[k]) for k in range(2)]
    for k, f in enumerate(fs):
        f.ds = _Attrs(dict(scale_fact=(1.7, 0.6)[k], spatial_mean=0.25 * (k + 1), temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
                           covariate_scales=[12.0, 6.0], spatial_model=_StubTrend()))
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    P = joint_prediction.Predictor(mod, fields.MultiField(fs))
    yield P
    P.close()


def _frame(out):
    from sif_xco2_cokriging_amd import joint_prediction
    return out if joint_prediction.xr is None else out.to_dataframe()


def test_predictor_predict_pair(native, predictor, cases):
    P, c = predictor, cases[300, 277]
    pc = c["pc0"]
    p0, e0, p1, e1, cov = P.predict_pair_arrays(pc)
    a, b = P.predict_arrays(0, pc), P.predict_arrays(1, pc)
    assert rel(p0, a[0]) < 1e-12 and rel(e0, a[1]) < 1e-12 and rel(p1, b[0]) < 1e-12 and rel(e1, b[1]) < 1e-12
    raw = _frame(P.predict_pair(pc, postprocess=False))
    from sif_xco2_cokriging_amd import joint_prediction
    if joint_prediction.xr is None:   # (a Dataset is indexed by the sorted coordinates)
        assert np.array_equal(raw["pred_cov"].values, cov) and np.array_equal(raw["pred_0"].values, p0)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(e0 * e1 > 0, cov / (e0 * e1), np.nan)
        assert np.array_equal(raw["pred_corr"].values, want, equal_nan=True)
        on0 = c["defl"][:300]
        assert np.all(np.abs(raw["pred_corr"].values[~on0 & (e1 > 0)]) < 1.0)
        out = _frame(P.predict_pair(pc, postprocess=True))
        assert np.allclose(out["pred_cov"].values, 1.7 * 0.6 * cov, rtol=1e-14, atol=0)
        assert np.allclose(out["pred_err_1"].values, 0.6 * e1, rtol=1e-14, atol=0)
    # chunked equals unchunked
    budget = P.rhs_budget_bytes
    try:
        P.rhs_budget_bytes = 1   # the floor of 1024 rows a sweep: 479 sites of each process
        q0, f0, q1, f1, cov2 = P.predict_pair_arrays(np.vstack([pc, c["pc1"]]))
    finally:
        P.rhs_budget_bytes = budget
    r0, g0, r1, g1, cov1 = P.predict_pair_arrays(np.vstack([pc, c["pc1"]]))
    for got, want in [(q0, r0), (f0, g0), (q1, r1), (f1, g1)]:
        assert rel(got, want) < 1e-12
    assert np.max(np.abs(cov2 - cov1)) < 1e-12
    # explicit pairs across two site sets
    pairs = np.array([[0, 0], [5, 7], [299, 276]])
    (o0, o1), pc_cov = P.predict_pair(pc, c["pc1"], pairs=pairs, postprocess=False)
    S = c["S"]
    sd = np.sqrt(np.abs(np.diag(S)))
    assert np.all(np.abs(pc_cov - S[pairs[:, 0], 300 + pairs[:, 1]]) <= 1e-8 * sd[pairs[:, 0]] * sd[300 + pairs[:, 1]] + 1e-12)
    assert len(_frame(o0)) == 300 and len(_frame(o1)) == 277


def test_predictor_joint_simulation(native, predictor, cases):
    from numpy.linalg import LinAlgError
    from sif_xco2_cokriging_amd import joint_prediction
    P, c = predictor, cases[65, 63]
    pc0, pc1, defl = c["pc0"], c["pc1"], c["defl"]
    # repeated sites are removed per process and get the draws of their first occurrence
    dup0 = np.vstack([pc0, pc0[[3]]])
    draws, pred, err, got_defl, seed = P.conditional_draws_arrays((0, 1), dup0, 12, seed=11, pcoords1=pc1)
    assert seed == 11 and draws.shape == (12, 66 + 63)
    assert np.array_equal(draws[:, 65], draws[:, 3]) and np.array_equal(got_defl, np.concatenate([defl[:65], defl[[3]], defl[65:]]))
    ref = P._factored_handle().conditional_draws_pair(pc0, pc1, 12, seed=11)[0]
    assert np.array_equal(np.delete(draws, 65, axis=1), ref)
    out0, out1 = P.conditional_simulation((0, 1), pc0, 12, seed=11, postprocess=False, pcoords1=pc1)
    if joint_prediction.xr is None:
        (df0, d0), (df1, d1) = out0, out1
        assert d0.shape == (12, 65) and d1.shape == (12, 63) and np.array_equal(np.hstack([d0, d1]), ref)
        assert df0.attrs == {"seed": 11, "n_deflated": 20, "jitter": 0.0} and df1.attrs["n_deflated"] == 15
        (pf0, e0), (pf1, e1) = P.conditional_simulation((0, 1), pc0, 12, seed=11, postprocess=True, pcoords1=pc1)
        assert np.allclose(e1 - pf1["pred"].values, 0.6 * (d1 - df1["pred"].values), rtol=0, atol=1e-12)
    else:
        assert out0["draws"].dims[0] == "draw" and out0.attrs["n_deflated"] == 20 and out1.attrs["n_deflated"] == 15
    # the same sites for both processes by default
    same = P.conditional_draws_arrays((0, 1), pc0, 3, seed=2)
    assert same[0].shape == (3, 130) and np.array_equal(same[3][:65], defl[:65])
    # a factorisation that stops: the message names the process and the caller's site (here through a handle that reports
    # stacked site 65 + 2 of the de-duplicated sets, i.e. site 2 of process 1)
    h = P._factored_handle()
    real = h.conditional_draws_pair
    try:
        h.conditional_draws_pair = lambda a, b, n, **kw: (np.zeros((n, 128)), np.zeros(128), np.zeros(128), np.zeros(128, bool), 1 + 65 + 2)
        with pytest.raises(LinAlgError, match="at site 2 .* of process 1"):
            P.conditional_draws_arrays((0, 1), pc0, 2, seed=1, pcoords1=pc1)
    finally:
        h.conditional_draws_pair = real
