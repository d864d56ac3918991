"""GPU tests of ck_loglik, ck_loglik_reml, ck_predict_universal, ck_conditional_draws and ck_predict_blocks at the sizes
their kernels index by: data sets below a tile, on and around the 64-row strips and the 512-wide panels (CkLayout: n0p =
roundup(n0, 64)), prediction sites around the 128-row tiles, the 256-site Hilbert threshold and the Schur panels, draw
counts and chunks around the 128-row pitch, block counts around CK_AUX_ALIGN and CK_NB -- and sequences of calls on one
handle.  The references are the dense float64 chains of tests/dense_chains.py, whose own accuracy and whose data sets'
conditioning tests/test_dense_chains.py checks on the host."""
import functools

import numpy as np
import pytest

from tests import dense_chains as dc

pytestmark = pytest.mark.gpu

# The gradient against 1/2 tr(G dSigma) with dSigma by central differences of the oracle's covariance blocks.  That
# reference's own floor -- what halving its step changes -- at the largest rung (513, 511): 1.4e-10 BIV, 6.5e-9 BIV_EUC,
# 3.3e-10 BIV_HALF (univariate 513: 1.9e-10); one-ulp relative perturbations of Sigma and z move it by 5e-13 at most.
# Ten times the largest: 6.5e-8, in the measure of test_gradient_against_dense_differences (whose bound, 1e-6, is its FD
# reference's).
GRAD_TOL = 6.5e-8


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[3]}"


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def err(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))


def handle(native, ds, site_order=1, factor=True, values=None):
    p = ds.p
    h = native.Handle(0)
    if site_order != 1:
        h.set_option("site_order", site_order)
    if p.n_procs == 2:
        h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                    p.nugget, p.rho)
    else:
        h.set_model(1, p.sigma, [p.nu[0, 0]] * 3, [p.len_scale[0, 0]] * 3, p.nugget, 0.0)
    h.set_metric(ds.metric)
    for k in range(p.n_procs):
        h.set_data(k, ds.coords[k], (values or ds.values)[k])
    h.assemble_joint()
    if factor:
        assert h.factor() == 0
    return h


def same(a, b):
    """bit for bit, through tuples"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- 1. log-likelihood and gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.LIK_CASES, ids=case_id)
def test_loglik_and_gradient(native, case):
    ds = dc.data_set(case)
    ref = dc.dense_ll(ds.params, ds.coords, ds.values, ds.metric, S=ds.S)
    gref = dc.dense_ll_grad(ds.params, ds.coords, ds.values, ds.metric, S=ds.S)
    ll = []
    for so in (1, 0):
        h = handle(native, ds, so, factor=False)
        info, v, g0 = h.loglik(False)
        assert info == 0 and g0 is None
        h.close()
        h = handle(native, ds, so, factor=False)
        info, vg, g = h.loglik(True)
        assert info == 0 and g.shape == (len(ds.params),)
        assert vg == v                                  # with and without the gradient: the same three numbers
        info, v2, g2 = h.loglik(True)                   # the resident factor of the first call
        assert info == 0 and v2 == vg and np.array_equal(g2, g)
        assert h.loglik_timings()["factor_ms"] == 0.0
        h.close()
        print(f"{case} site_order {so}: l, log|Sigma|, quad rel {[abs(a - b) / abs(b) for a, b in zip(v, ref)]}, "
              f"gradient {err(g, gref):.2e}")
        for a, b in zip(v, ref):
            assert abs(a - b) <= 1e-8 * abs(b), (so, v, ref)
        assert err(g, gref) < GRAD_TOL, (so, g, gref)
        ll.append(v[0])
    assert abs(ll[0] - ll[1]) <= 1e-11 * abs(ll[1])   # site orders agree to rounding


# ---- 2. REML ------------------------------------------------------------------------------------------------------------------
REML_CASES = ([(c, kind) for c in dc.FIVE_RUNGS for kind in ("constant", "linear")]
              + [(dc.SMALL, "wide"), (dc.FIVE_RUNGS[4], "wide")])


@pytest.mark.parametrize("case,kind", REML_CASES, ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_reml_value_and_gradient(native, case, kind):
    ds = dc.data_set(case)
    values = [v + 0.3 for v in ds.values]   # a mean the zero-mean model does not know
    Fs = [dc.design(kind, c, c) for c in ds.coords]
    q = sum(F.shape[1] for F in Fs)
    assert ds.N >= q + 2
    h = handle(native, ds, factor=False, values=values)
    if kind == "wide":   # CK_TREND_PMAX = 8 columns per process, 16 in all for two: one more is refused
        assert all(F.shape[1] == 8 for F in Fs)
        with pytest.raises(RuntimeError, match="at most 8"):
            h.set_trend(0, np.column_stack([Fs[0], np.arange(len(Fs[0]))]))
    for k, F in enumerate(Fs):
        h.set_trend(k, F)
    info, out4, g = h.loglik_reml(True)
    assert info == 0
    ref = dc.dense_reml(ds.params, ds.coords, values, ds.metric, Fs)
    gref = dc.dense_reml_grad(ds.params, ds.coords, values, ds.metric, Fs, S=ds.S)
    print(f"{case} {kind}: values {[abs(a - b) / max(1.0, abs(b)) for a, b in zip(out4, ref)]}, gradient {err(g, gref):.2e}")
    for a, b in zip(out4, ref):
        assert abs(a - b) < 1e-8 * max(1.0, abs(b))
    info, out4v, _ = h.loglik_reml(False)
    assert abs(out4v[0] - out4[0]) < 1e-9 * abs(out4[0])
    assert err(g, gref) < 1e-6, (g, gref)
    h.close()


def test_reml_without_trend_is_loglik(native):
    h = handle(native, dc.data_set((64, 64, 40, "BIV", dc.HAV)), factor=False)
    info, out3, g = h.loglik(True)
    h.assemble_joint()
    info2, out4, g2 = h.loglik_reml(True)
    assert info == info2 == 0
    assert out4[0] == out3[0] and out4[1] == out3[1] and out4[2] == 0.0 and out4[3] == out3[2]
    assert np.array_equal(g, g2)
    h.close()


# ---- 3. universal prediction --------------------------------------------------------------------------------------------------
UNIV_KIND = {(5, 3): "constant", (63, 65): "linear", (448, 64): "constant", (513, 511): "linear", (65, 0): "linear"}
UNIV_CASES = [(c, UNIV_KIND[c[:2]], m) for c in dc.FIVE_RUNGS for m in (1, 255, 256, 257)] + [(dc.SMALL, "wide", 257)]


@pytest.mark.parametrize("case,kind,m", UNIV_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else case_id(v))
def test_universal_prediction(native, case, kind, m):
    ds = dc.data_set(case)
    values = [v + 0.3 for v in ds.values]
    Fs = [dc.design(kind, c, c) for c in ds.coords]
    h = handle(native, ds, values=values)
    for k, F in enumerate(Fs):
        h.set_trend(k, F)
    for i in range(ds.p.n_procs):
        pc = dc.pred_sites(np.random.default_rng(1000 * m + i), ds.metric, m)
        F0 = dc.design(kind, ds.coords[i], pc)
        pred, e, beta, cov = h.predict_universal(i, pc, F0)
        rp, rv, rb, rc = dc.dense_universal(ds.p, ds.coords, values, pc, i, ds.metric, Fs, F0, S=ds.S)
        print(f"{case} {kind} m={m} i={i}: pred {dc.rel(pred, rp):.2e} var {np.max(np.abs(e ** 2 - rv)):.2e} "
              f"beta {dc.rel(beta, rb):.2e} cov {dc.rel(cov, rc):.2e}")
        assert dc.rel(pred, rp) < 1e-9
        assert np.max(np.abs(e ** 2 - rv)) < 1e-10
        assert dc.rel(beta, rb) < 1e-9 and dc.rel(cov, rc) < 1e-9
        again = h.predict_universal(i, pc, F0)
        assert same(again, (pred, e, beta, cov))
    h.close()


# ---- 4. conditional draws, given noise ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draw_reference(data, i, m, n_on, seed):
    """(sites, mask of the sites on data, dense pred, dense S), computed once per case"""
    ds = dc.data_set(data)
    pc, on = dc.draw_sites(ds, i, m, n_on, seed)
    return (pc, on) + dc.posterior(ds.p, ds.coords, ds.values, pc, i, ds.metric, ds.cf)


def check_draws(native, h, i, pc, on, S, site_order, n_draws, eps, n_chunks):
    m = len(pc)
    draws, pred, e, defl, info = h.conditional_draws(i, pc, n_draws, noise=eps)
    assert info == 0
    assert np.array_equal(defl, on)
    assert np.array_equal(draws[:, defl], np.broadcast_to(pred[defl], (n_draws, int(defl.sum()))))
    want = dc.chain_draws(pred, S, defl, dc.internal_order(native.hilbert_order, pc, site_order), eps)
    print(f"m={m} n_draws={n_draws} site_order={site_order}: draws against the chain {dc.rel(draws, want):.2e}")
    assert dc.rel(draws, want) < 1e-8
    t = h.draws_timings()
    assert t["n_deflated"] == on.sum() and t["n_chunks"] == n_chunks
    return draws, pred, e


@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("case", dc.DRAW_CASES, ids=lambda c: f"{c[0][0]}-{c[0][1]}-i{c[1]}-m{c[2]}")
def test_draws_at_every_site_count(native, case, site_order):
    data, i, m, n_on, seed = case
    ds = dc.data_set(data)
    pc, on, rpred, S = draw_reference(*case)
    h = handle(native, ds, site_order)
    p0, e0 = h.predict(i, pc)
    eps = np.random.default_rng(seed + site_order).standard_normal((7, m))
    draws, pred, e = check_draws(native, h, i, pc, on, S, site_order, 7, eps, 1)
    assert np.array_equal(pred, p0) and np.array_equal(e, e0)
    assert dc.rel(pred, rpred) < 1e-9
    h.close()


@pytest.mark.parametrize("case", [c for c in dc.DRAW_CASES if c[2] in (129, 513)],
                         ids=lambda c: f"{c[0][0]}-{c[0][1]}-i{c[1]}-m{c[2]}")
def test_draw_counts_and_chunks(native, case):
    data, i, m, n_on, seed = case
    pc, on, rpred, S = draw_reference(*case)
    h = handle(native, dc.data_set(data))
    rng = np.random.default_rng(seed)
    whole = {}
    for n_draws, chunk in dc.DRAW_COUNTS:
        if n_draws not in whole:
            eps = rng.standard_normal((n_draws, m))
            h.set_option("draw_chunk", 0)
            whole[n_draws] = (eps, check_draws(native, h, i, pc, on, S, 1, n_draws, eps, 1)[0])
        if chunk:
            eps, one = whole[n_draws]
            h.set_option("draw_chunk", chunk)
            got = check_draws(native, h, i, pc, on, S, 1, n_draws, eps, -(-n_draws // chunk))[0]
            assert np.array_equal(got, one), (n_draws, chunk)   # every element sums in a fixed order whatever the chunk
    h.close()


# ---- 5. block cokriging -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_reference(data, i, m):
    ds = dc.data_set(data)
    pc = dc.pred_sites(np.random.default_rng(77 + i), ds.metric, m)
    return (pc,) + dc.posterior(ds.p, ds.coords, ds.values, pc, i, ds.metric, ds.cf)


def check_blocks(h, i, pc, lab, w, r, rpred, S, prior):
    A = dc.amat(lab, w, r)
    rp, rc = A @ rpred, A @ S @ A.T
    out = {}
    for chunk in (0, 100, 300):   # 100: chunks in the caller's row order; 300: Hilbert-sorted chunks
        h.set_option("block_chunk", chunk)
        pred, e, cov = h.predict_blocks(i, pc, lab, w, r, want_cov=True)
        assert h.timings()["blocks_chunks"] == (-(-len(pc) // chunk) if chunk else 1)
        print(f"m={len(pc)} r={r} chunk={chunk}: pred {dc.rel(pred, rp):.2e} var {np.max(np.abs(e ** 2 - np.maximum(np.diag(rc), 0))):.2e}"
              f" cov {np.max(np.abs(cov - rc)):.2e}")
        assert dc.rel(pred, rp) < 1e-9
        assert np.max(np.abs(e ** 2 - np.maximum(np.diag(rc), 0.0))) < 1e-10
        assert np.max(np.abs(cov - rc)) < 1e-10
        assert np.array_equal(cov, cov.T)
        assert np.all(e ** 2 <= np.diag(A @ prior @ A.T) + 1e-10)   # the posterior variance is at most the prior's
        out[chunk] = (pred, e, cov)
    h.set_option("block_chunk", 0)
    assert same(h.predict_blocks(i, pc, lab, w, r, want_cov=True), out[0])   # repeated: the same bits
    # include/cokrige.h: "every block's members are summed in the caller's order whatever the chunking"
    assert same(out[100], out[0]) and same(out[300], out[0])
    p2, e2, c2 = h.predict_blocks(i, pc, lab, w, r)
    assert c2 is None and same((p2, e2), out[0][:2])
    return out[0]


@pytest.mark.parametrize("r", dc.BLOCK_R)
@pytest.mark.parametrize("data", [dc.SMALL, dc.LARGE], ids=case_id)
def test_blocks_at_every_block_count(native, data, r):
    from oracle import cokrige_oracle as orc
    ds = dc.data_set(data)
    i = r % 2
    pc, rpred, S = block_reference(data, i, dc.BLOCK_M)
    rng = np.random.default_rng(r)
    lab = dc.block_labels(rng, r, dc.BLOCK_M)
    w = rng.uniform(0.2, 2.0, dc.BLOCK_M) / np.bincount(lab)[lab]   # weighted block means: every block's value is O(1)
    h = handle(native, ds)
    check_blocks(h, i, pc, lab, w, r, rpred, S, orc.pred_cov(ds.p, pc, i, ds.metric))
    h.close()


@pytest.mark.parametrize("data", [dc.SMALL, dc.LARGE], ids=case_id)
def test_singleton_blocks_and_the_empty_block(native, data):
    from oracle import cokrige_oracle as orc
    ds = dc.data_set(data)
    h = handle(native, ds)
    for i in (0, 1):
        pc, rpred, S = block_reference(data, i, 40)
        lab = dc.block_labels(np.random.default_rng(i), 40, 40)
        pred, e, cov = check_blocks(h, i, pc, lab, np.ones(40), 40, rpred, S, orc.pred_cov(ds.p, pc, i, ds.metric))
        pp, pe = h.predict(i, pc)
        assert dc.rel(pred[lab], pp) <= 1e-12 and dc.rel(e[lab], pe) <= 1e-12   # a block of one site is ck_predict
        # include/cokrige.h: "every block non-empty" -- a label nobody carries is refused, and the handle goes on
        with pytest.raises(native.NativeError, match="block 39 has no site"):
            h.predict_blocks(i, pc, np.where(lab == 40 - 1, 41, lab), np.ones(40), 42)
        assert same(h.predict_blocks(i, pc, lab, np.ones(40), 40, want_cov=True), (pred, e, cov))
    h.close()


# ---- 6. sequences on one handle -------------------------------------------------------------------------------------------------
def sequence_steps(ds):
    rng = np.random.default_rng(6)
    sites = {m: dc.pred_sites(rng, ds.metric, m) for m in (5, 40, 64, 300, 700)}
    d129, on129 = dc.draw_sites(ds, 0, 129, 20, 61)
    d513, on513 = dc.draw_sites(ds, 1, 513, 20, 62)
    eps = rng.standard_normal((3, 129))
    lab300 = dc.block_labels(rng, 7, 300)
    w300 = rng.uniform(0.2, 2.0, 300)
    lab40 = dc.block_labels(rng, 40, 40)
    F = [dc.design("linear", c, c) for c in ds.coords]

    def universal(h):
        for k in range(ds.p.n_procs):
            h.set_trend(k, F[k])
        return h.predict_universal(1, sites[5], dc.design("linear", ds.coords[1], sites[5]))

    return [("predict m=700", lambda h: h.predict(0, sites[700])),
            ("loglik", lambda h: h.loglik(True)),
            ("predict_universal m=5", universal),
            ("predict_blocks m=300 r=7", lambda h: h.predict_blocks(1, sites[300], lab300, w300, 7, want_cov=True)),
            ("conditional_draws m=129", lambda h: h.conditional_draws(0, d129, 3, noise=eps)),
            ("predict m=64", lambda h: h.predict(1, sites[64])),
            ("loocv", lambda h: h.loocv(0, len(ds.coords[0]))),
            ("conditional_draws m=513", lambda h: h.conditional_draws(1, d513, 5, seed=9)),
            ("predict_blocks m=40 r=40", lambda h: h.predict_blocks(0, sites[40], lab40, np.ones(40), 40, want_cov=True)),
            ("predict m=700 again", lambda h: h.predict(0, sites[700]))]


def test_sequence_on_one_handle(native):
    """every call of a sequence on one handle gives the bits of the same call on a fresh handle that did only
    assemble_joint, factor and that call: nothing a call leaves behind -- padding rows and columns of the right-hand
    sides, Schur buffers, block rows, the trend -- reaches a later one"""
    ds = dc.data_set(dc.LARGE)
    steps = sequence_steps(ds)
    h = handle(native, ds)
    for name, step in steps:
        got = step(h)
        f = handle(native, ds)
        want = step(f)
        f.close()
        assert same(got, want), name
    # ck_set_data on a handle whose data are laid out is refused (a new data set needs a new handle), and the handle goes
    # on as it was: assembled and factored again it still gives a fresh handle's bits
    small = dc.data_set(dc.SMALL)
    with pytest.raises(native.NativeError, match="create a new handle"):
        h.set_data(0, small.coords[0], small.values[0])
    h.assemble_joint()
    assert h.factor() == 0
    for name, step in (steps[1], steps[4], steps[3]):
        f = handle(native, ds)
        want = step(f)
        f.close()
        assert same(step(h), want), name + " after assembling again"
    h.close()


@pytest.mark.parametrize("data", [dc.SMALL, dc.REFIT], ids=case_id)
def test_handles_of_other_sizes_after_a_large_one(native, data):
    """the sequence's calls on data sets of other sizes, each on one handle created after the (513, 511) handles above
    have come and gone, against a fresh handle per call"""
    ds = dc.data_set(data)
    steps = sequence_steps(ds)
    h = handle(native, ds)
    for name, step in (steps[1], steps[4], steps[3]):
        got = step(h)
        f = handle(native, ds)
        want = step(f)
        f.close()
        assert same(got, want), name
    ref = dc.dense_ll(ds.params, ds.coords, ds.values, ds.metric, S=ds.S)
    h.assemble_joint()
    info, v, g = h.loglik(True)
    assert info == 0 and all(abs(a - b) <= 1e-8 * abs(b) for a, b in zip(v, ref))
    h.close()


def growing_steps(ds):
    rng = np.random.default_rng(66)
    sites = {m: dc.pred_sites(rng, ds.metric, m) for m in (5, 300, 700)}
    lab2, lab300 = dc.block_labels(rng, 2, 300), dc.block_labels(rng, 300, 300)
    w300 = rng.uniform(0.2, 2.0, 300)
    noise = [rng.uniform(0.01, 0.05, len(c)) for c in ds.coords]
    lags10, lags5000 = rng.uniform(0.0, 2000.0, 10), rng.uniform(0.0, 2000.0, 5000)
    v300 = (dc.pred_sites(rng, ds.metric, 300), rng.standard_normal(300))
    vi, vj = ((dc.pred_sites(rng, ds.metric, n), rng.standard_normal(n)) for n in (3000, 2500))
    folds = rng.integers(0, 10, len(ds.coords[0]))
    d129, _ = dc.draw_sites(ds, 0, 129, 20, 61)
    eps = rng.standard_normal((3, 129))
    from sif_xco2_cokriging_amd.variogram import variogram_arrays

    def predict(m):
        return lambda h: (h.predict(0, sites[m]), h.verify_model())

    def universal(kind):
        def step(h):
            for k in range(2):
                h.set_trend(k, dc.design(kind, ds.coords[k], ds.coords[k]) if kind else None)
            return h.predict_universal(1, sites[300], dc.design(kind, ds.coords[1], sites[300]) if kind else None)
        return step

    def noisy(on):
        def step(h):
            for k in range(2):
                h.set_noise(k, noise[k] if on else None)
            h.assemble_joint()
            return h.factor(), h.predict(1, sites[300])
        return step

    def vario(a, b=None):
        same = b is None
        return lambda h: variogram_arrays(h, a[0], a[1], None if same else b[0], None if same else b[1], same, 1500.0, 20)

    def local(m, max_dist, reserve=0):
        def step(h):
            if reserve:
                h.local_reserve(reserve)
            pred, e, info = h.predict_local(0, sites[m], max_dist=max_dist)
            return pred.view(np.uint64), e.view(np.uint64), sorted(info.items())   # the bits: sites without a neighbour give NaN
        return step

    return [("predict m=5", predict(5)), ("predict m=300", predict(300)), ("predict m=700", predict(700)),
            ("predict m=5 again", predict(5)),
            ("predict_blocks r=2", lambda h: h.predict_blocks(1, sites[300], lab2, w300, 2, want_cov=True)),
            ("predict_blocks r=300", lambda h: h.predict_blocks(1, sites[300], lab300, w300, 300, want_cov=True)),
            ("trend constant", universal("constant")), ("trend linear", universal("linear")), ("trend cleared", universal(None)),
            ("noise on", noisy(True)), ("noise cleared", noisy(False)),
            ("model_variogram 10", lambda h: h.model_variogram(0, 1, lags10)),
            ("model_variogram 5000", lambda h: h.model_variogram(0, 1, lags5000)),
            ("variogram 300", vario(v300)), ("variogram 3000 x 2500", vario(vi, vj)), ("variogram 300 again", vario(v300)),
            # five sites at 2000 km: neighbourhoods of most of the data (the tiled path) in a slab of tens of MB -- from 1 GiB on
            # the slab takes its whole budget, a quarter of the card's free memory, which is also what local_reserve(0) does
            ("predict_local 150 km", local(300, 150.0)), ("predict_local 2000 km", local(5, 2000.0)),
            ("local_reserve", local(5, 2000.0, reserve=64 << 20)),
            ("cv_folds", lambda h: h.cv_folds(0, folds, want_stats=True)),
            ("conditional_draws", lambda h: h.conditional_draws(0, d129, 3, noise=eps))], sites, v300


def test_growing_sequence_and_handle_life_cycle(native):
    """as test_sequence_on_one_handle, with every buffer of the handle growing on the way: right-hand sides over two mpad
    steps (Schur panels 512 -> 1024 -> 512), block rows, trend, noise, variogram rows and lists, the local slab -- each call
    gives the bits of the same call on a fresh handle.  Then handles closed at every stage of their life, and an arena"""
    import torch
    ds = dc.data_set(dc.REFIT)
    steps, sites, v300 = growing_steps(ds)
    h = handle(native, ds)
    for name, step in steps:
        got = step(h)
        f = handle(native, ds)
        want = step(f)
        f.close()
        assert same(got, want), name
    # ---- closing a handle at every stage
    for _ in range(20):
        native.Handle(0).close()
    f = native.Handle(0)
    p = ds.p
    f.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    for k in range(2):
        f.set_data(k, ds.coords[k], ds.values[k])
    f.close()
    f = native.Handle(0)
    f.vario_begin(*v300)   # no vario_end
    f.close()
    f = handle(native, ds)
    f.set_option("gemm_stamps", 1)
    f.close()
    # ---- an arena of estimate_bytes(700): the largest m first.  The arena never takes a carve back, so under it only
    # non-growing orders fit the estimate (m = 5 first and 700 after it would need both right-hand-side buffers)
    want = [h.predict(0, sites[m]) for m in (700, 5, 700)]
    h.close()
    a = native.Handle(0)
    a.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    a.set_metric(ds.metric)
    for k in range(2):
        a.set_data(k, ds.coords[k], ds.values[k])
    nbytes = a.estimate_bytes(700)
    arena = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    a.set_arena(arena.data_ptr(), nbytes, keepalive=arena)
    a.assemble_joint()
    assert a.factor() == 0
    assert same([a.predict(0, sites[m]) for m in (700, 5, 700)], want)
    a.close()


def test_arena_refusal_leaves_the_handle_usable(native):
    """an arena of estimate_bytes(700) has no room for the gradient's Npad + 1 unit rows: the call is refused in front of its first
    allocation, with the amounts, and the handle goes on giving the bits it gave before"""
    import re
    import torch
    ds = dc.data_set(dc.REFIT)
    p = ds.p
    sites = dc.pred_sites(np.random.default_rng(66), ds.metric, 700)
    a = native.Handle(0)
    a.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    a.set_metric(ds.metric)
    for k in range(2):
        a.set_data(k, ds.coords[k], ds.values[k])
    nbytes = a.estimate_bytes(700)
    arena = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    a.set_arena(arena.data_ptr(), nbytes, keepalive=arena)
    a.assemble_joint()
    assert a.factor() == 0
    pred = a.predict(0, sites)
    value = a.loglik(False)
    assert value[0] == 0 and same(a.predict(0, sites), pred)
    with pytest.raises(native.NativeError, match="of the arena") as err:
        a.loglik(True)
    rows = int(re.search(r"for its (\d+) right-hand-side rows", str(err.value)).group(1))
    N = sum(len(c) for c in ds.coords)
    assert rows > N and (rows - 1) % 512 == 0       # Npad + 1: the data row and the unit row of every internal position
    assert same(a.loglik(False), value)
    assert same(a.predict(0, sites), pred)
    a.close()
