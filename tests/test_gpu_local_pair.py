"""GPU tests of both processes in the moving neighbourhood: include/cokrige.h ck_predict_local_pair, native.Handle.
predict_local_pair, point_prediction.Predictor.predict_pair; ck_simulate_local_pair, ck_debug_simulate_local_pair_weights,
point_prediction.Predictor.conditional_simulation((0, 1), ...).

1. bits: pred / err of either process equal predict_local(0) / predict_local(1) (cv off) on the same handle, in the LDS class
   and at every tiled size of item 2;
2. padding boundaries: every neighbour in every set (max_dist = 1e9) at sizes that put k + 3 on and one past multiples of 64,
   on both sides of the LDS limit, all five outputs against tests/local_pair_ref.py; several batches against one;
3. variants: both metrics, measurement-error variances, caps that bind, both site orders; |cov| <= err0 err1;
4. degenerate points; 5. the co-simulation (its own header below); 6. the contract: every refusal with its message, the handle's state; 7. the Python layer.
Tolerances are the local path's own (tests/test_gpu_local.py): rtol 1e-8, atol 1e-10.  The numpy / device agreement condition
gap > 1e-9 is asserted for every case."""
import numpy as np
import pytest

from tests import local_pair_ref as lp

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10
FIVE = ("pred0", "err0", "pred1", "err1", "cov")
# (n0, n1): k + 3 on and one past multiples of 64, both sides of the LDS limit
SIZES = [(1, 1), (2, 1), (30, 31), (31, 31), (32, 31), (32, 32), (33, 32), (63, 62), (63, 63), (64, 63), (100, 89), (100, 90),
         (120, 7)]
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_handle(native, params, metric, coords, values, caps=(0, 0), noise=None, **options):
    h = native.Handle(0)
    for name, value in options.items():
        h.set_option(name, value)
    pv = list(params)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
        if noise is not None:
            h.set_noise(k, noise[k], 1.0)
    h.set_local_neighbours(*caps)
    return h


def conus(n0, n1):
    """conus_problem(120, seed=41) truncated to (n0, n1) data, 9 of its sites"""
    from sif_xco2_cokriging_amd import synth
    pb = synth.conus_problem(120, seed=41)
    return dict(params=pb["params"], metric=HAV, coords=[pb["coords"][0][:n0], pb["coords"][1][:n1]],
                values=[pb["values"][0][:n0], pb["values"][1][:n1]], sites=pb["pcoords"][::997][:9])


def reference(key, pb, max_dist, caps=(0, 0), noise=None):
    if key not in _cache:
        ref = lp.local_pair_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["sites"], max_dist, caps, noise)
        assert ref["gap"] > 1e-9, (key, ref["gap"])   # numpy and the device must agree on every set
        _cache[key] = ref
    return _cache[key]


def check_five(got, ref, what):
    for name, g in zip(FIVE, got):
        print(what, name, "max abs diff", np.nanmax(np.abs(g - ref[name])) if np.any(~np.isnan(ref[name])) else 0.0)
        assert np.array_equal(np.isnan(g), np.isnan(ref[name])), (what, name)
        assert np.allclose(g, ref[name], rtol=RTOL, atol=ATOL, equal_nan=True), (what, name)


def check_bits(h, got, sites, max_dist, what, k, k_hi=64):
    """pred / err of the pair call against the single calls on the same handle: equal bits, except at tiled systems (k > k_hi)
    of k = 62 (mod 64) neighbours -- the one size where the pair call's padded height roundup(k + 3, 64) is not the single
    call's roundup(k + 2, 64): the rows ride through one more 64-column block and the last bits may differ.  Measured on the
    MI355X at k = 62, 126, 190: max |d pred| 8.9e-16, max |d err| 7.8e-16 on values of order 1.  Those points are held to the reference by check_five, and here to the single calls at the same
    tolerances."""
    k = np.asarray(k)
    loose = (k > k_hi) & (k % 64 == 62)
    for q in range(2):
        pred, err, _ = h.predict_local(q, sites, max_dist=max_dist)
        for name, a, b in (("pred", got[2 * q], pred), ("err", got[2 * q + 1], err)):
            assert np.array_equal(a[~loose], b[~loose], equal_nan=True), (what, q, name)
            if loose.any():
                print(what, name, q, "pair call against the single call at k = 62 (mod 64): max abs diff",
                      np.nanmax(np.abs(a[loose] - b[loose])))
                assert np.allclose(a[loose], b[loose], rtol=RTOL, atol=ATOL, equal_nan=True), (what, q, name)


# ---- 1. bits, the LDS class ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [(6, 6), (0, 0)])
@pytest.mark.parametrize("max_dist", [0.12, 0.2])
def test_pair_bits_lds_class(native, caps, max_dist):
    from sif_xco2_cokriging_amd import synth
    pb = synth.unit_square_problem(40, grid_side=2, seed=20002)
    sites = np.random.default_rng(7).random((50, 2))
    pb = dict(params=pb["params"], metric=pb["metric"], coords=pb["coords"], values=pb["values"], sites=sites)
    ref = reference(("unit", caps, max_dist), pb, max_dist, caps)
    h = make_handle(native, pb["params"], pb["metric"], pb["coords"], pb["values"], caps)
    *got, info = h.predict_local_pair(sites, max_dist=max_dist)
    assert info == dict(n_empty=ref["n_empty"], n_not_pd=0, k_max=ref["k_max"])
    assert ref["k_max"] <= 64
    check_bits(h, got, sites, max_dist, ("unit", caps, max_dist), ref["k"])
    check_five(got, ref, ("unit", caps, max_dist))
    h.close()


# ---- 2. padding boundaries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_min", [None, 0])
@pytest.mark.parametrize("n0,n1", SIZES)
def test_pair_padding_boundaries(native, n0, n1, tile_min):
    pb = conus(n0, n1)
    ref = reference(("conus", n0, n1), pb, 1e9)
    options = {} if tile_min is None else dict(local_tile_min=tile_min)
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"], **options)
    *got, info = h.predict_local_pair(pb["sites"], max_dist=1e9)
    assert info == dict(n_empty=0, n_not_pd=0, k_max=n0 + n1)
    check_five(got, ref, (n0, n1, tile_min))
    check_bits(h, got, pb["sites"], 1e9, (n0, n1, tile_min), ref["k"], k_hi=64 if tile_min is None else 0)
    h.close()


def count_k(h, sites, max_dist):
    count, _ = h.local_neighbours(0, sites, max_dist=max_dist)
    return count.sum(axis=1)


def test_pair_batches_keep_the_bits(native):
    """several batches of the tiled class (local_slab_mb = 3, neighbourhoods above 300) against one"""
    from sif_xco2_cokriging_amd import synth
    pb = synth.conus_problem(1500, seed=9)
    sites = pb["pcoords"][::173][:40]
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    *one, info = h.predict_local_pair(sites, max_dist=900.0)
    assert info["k_max"] > 300 and info["n_not_pd"] == 0
    tm = h.local_pair_timings()
    assert tm["n_tiled"] > 1 and tm["n_tiled_batches"] == 1
    h.set_option("local_slab_mb", 3)
    *many, info2 = h.predict_local_pair(sites, max_dist=900.0)
    assert info2 == info
    # 3 MiB = 393 216 doubles; a system of more than 189 neighbours has kq >= 256 and needs at least (256 + 128)^2 + 8 * 64^2 =
    # 180 224 doubles (ck_host.h: ck_local_tiled_doubles), so at most two of them share a batch
    tm3 = h.local_pair_timings()
    n_large = np.count_nonzero(count_k(h, sites, 900.0) > 189)
    assert n_large > 4 and tm3["n_tiled"] == tm["n_tiled"] and tm3["n_tiled_batches"] >= (n_large + 1) // 2
    for a, b in zip(one, many):
        assert np.array_equal(a, b, equal_nan=True)
    h.set_option("local_slab_mb", 0)
    check_bits(h, one, sites, 900.0, "batches", count_k(h, sites, 900.0))
    h.close()


# ---- 3. variants -----------------------------------------------------------------------------------------------------------------
def variant(name):
    from sif_xco2_cokriging_amd import synth
    rng = np.random.default_rng(31)
    if name == "euclid_noise_caps":
        pb = synth.unit_square_problem(150, grid_side=2, seed=20002)
        return dict(params=pb["params"], metric=EUC, coords=pb["coords"], values=pb["values"], sites=rng.random((33, 2)),
                    noise=[0.05 + 0.1 * rng.random(150), 0.02 + 0.1 * rng.random(150)], caps=(7, 9), max_dist=0.3)
    if name == "euclid_tiled_noise":
        pb = synth.unit_square_problem(150, grid_side=2, seed=20002)
        return dict(params=pb["params"], metric=EUC, coords=pb["coords"], values=pb["values"], sites=rng.random((17, 2)),
                    noise=[0.05 + 0.1 * rng.random(150), 0.02 + 0.1 * rng.random(150)], caps=(0, 0), max_dist=0.45)
    if name == "haversine_caps":
        pb = synth.conus_problem(300, seed=5)
        return dict(params=pb["params"], metric=HAV, coords=pb["coords"], values=pb["values"], sites=pb["pcoords"][::211][:40],
                    noise=None, caps=(40, 50), max_dist=1500.0)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["euclid_noise_caps", "euclid_tiled_noise", "haversine_caps"])
def test_pair_variants(native, name):
    pb = variant(name)
    ref = reference(name, pb, pb["max_dist"], pb["caps"], pb["noise"])
    outs = []
    for order in (0, 1):
        h = make_handle(native, pb["params"], pb["metric"], pb["coords"], pb["values"], pb["caps"], pb["noise"], site_order=order)
        *got, info = h.predict_local_pair(pb["sites"], max_dist=pb["max_dist"])
        count, _ = h.local_neighbours(0, pb["sites"], max_dist=pb["max_dist"])
        assert np.array_equal(count, ref["count"])
        assert info == dict(n_empty=ref["n_empty"], n_not_pd=0, k_max=int(count.sum(axis=1).max()))
        check_five(got, ref, (name, order))
        check_bits(h, got, pb["sites"], pb["max_dist"], (name, order), ref["k"])
        e0, e1, cov = got[1], got[3], got[4]
        both = (e0 > 0) & (e1 > 0)
        assert np.all(np.abs(cov[both]) <= e0[both] * e1[both] * (1 + 1e-12))
        outs.append(got)
        h.close()
    for a, b in zip(*outs):
        assert np.allclose(a, b, rtol=1e-9, atol=0, equal_nan=True)


# ---- 4. degenerate points ------------------------------------------------------------------------------------------------------
def test_pair_empty_neighbourhood_and_sizes(native):
    pb = conus(30, 31)
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    far = np.array([[-60.0, 20.0]])
    *got, info = h.predict_local_pair(far, max_dist=500.0)   # m = 1
    assert info == dict(n_empty=1, n_not_pd=0, k_max=0)
    assert all(np.isnan(g).all() and g.shape == (1,) for g in got)
    from sif_xco2_cokriging_amd import synth
    sites = np.vstack([synth.conus_problem(120, seed=41)["pcoords"][::34][:256], far])   # m = 257, the last one empty
    pb = dict(pb, sites=sites)
    ref = reference("m257", pb, 700.0)
    *got, info = h.predict_local_pair(sites, max_dist=700.0)
    assert info == dict(n_empty=ref["n_empty"], n_not_pd=0, k_max=ref["k_max"]) and ref["n_empty"] >= 1
    check_five(got, ref, "m257")
    check_bits(h, got, sites, 700.0, "m257", ref["k"])
    h.close()


def test_pair_not_positive_definite(native, golden):
    g = golden("joint_not_pd")
    pv = g["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(0)
    h.set_data(0, g["coords0"], np.zeros(260))
    h.set_data(1, g["coords1"], np.zeros(260))
    pc = g["coords0"][:7] + 0.013
    *got, info = h.predict_local_pair(pc, max_dist=1e9)
    assert info == dict(n_empty=0, n_not_pd=7, k_max=520)
    assert all(np.isnan(x).all() for x in got)
    h.close()


# ---- 6. the contract -----------------------------------------------------------------------------------------------------------
def test_pair_refusals(native):
    pb = conus(30, 31)
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    sites = pb["sites"]
    with pytest.raises(native.NativeError, match="ck_predict_local_pair: max_dist must be finite and >= 0"):
        h.predict_local_pair(sites, max_dist=-1.0)
    with pytest.raises(native.NativeError, match="ck_predict_local_pair: max_dist must be finite and >= 0"):
        h.predict_local_pair(sites, max_dist=np.inf)
    with pytest.raises(native.NativeError, match="ck_predict_local_pair: m = 0 points; at least 1"):
        h.predict_local_pair(np.zeros((0, 2)), max_dist=10.0)
    import ctypes
    out = np.zeros(4)
    cnt = ctypes.c_int64(0)
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = out.ctypes.data_as(dp)
    rc = native.lib().ck_predict_local_pair(h._h, ptr, 1, 10.0, ptr, ptr, None, ptr, None, ctypes.byref(cnt), ctypes.byref(cnt),
                                            ctypes.byref(cnt))
    assert rc != 0 and b"ck_predict_local_pair: null" in native.lib().ck_last_error()
    h.set_trend(0, np.ones((30, 1)))
    with pytest.raises(native.NativeError, match="ck_predict_local_pair: a trend of 1 columns .*clear it with ck_set_trend"):
        h.predict_local_pair(sites, max_dist=10.0)
    h.close()
    one = native.Handle(0)
    pv = pb["params"]
    one.set_model(1, pv[0:1], pv[2:3], pv[5:6], pv[8:9])
    one.set_metric(HAV)
    one.set_data(0, pb["coords"][0], pb["values"][0])
    with pytest.raises(native.NativeError, match="ck_predict_local_pair: needs a model of two processes"):
        one.predict_local_pair(sites, max_dist=10.0)
    one.close()
    q = native.Handle(devices=[0, 0], rank=0)
    with pytest.raises(native.NativeError, match="ck_predict_local_pair .* partitioned"):
        q.predict_local_pair(sites, max_dist=10.0)
    q.close()


def test_pair_leaves_the_handle_alone(native):
    """a resident factor and the bits of predict / predict_local before and after the pair call"""
    pb = conus(100, 90)
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    sites = pb["sites"]
    h.assemble_joint()
    assert h.factor() == 0
    before = [h.predict(0, sites), h.predict_local(0, sites, max_dist=900.0)[:2], h.predict_local(1, sites, max_dist=1e9)[:2]]
    h.predict_local_pair(sites, max_dist=1e9)
    h.predict_local_pair(sites, max_dist=400.0)
    after = [h.predict(0, sites), h.predict_local(0, sites, max_dist=900.0)[:2], h.predict_local(1, sites, max_dist=1e9)[:2]]
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    h.close()


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------
class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


class _StubTrend:
    def predict(self, X):
        X = np.asarray(X, dtype=float)
        return 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.05


@pytest.fixture(scope="module")
def predictor(native):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    pb = conus(100, 90)
    fs = [fields.Field(pb["coords"][k], pb["values"][k]) for k in range(2)]
    for k, f in enumerate(fs):
        f.ds = _Attrs(dict(scale_fact=(1.7, 0.6)[k], spatial_mean=0.25 * (k + 1), temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
                           covariate_scales=[12.0, 6.0], spatial_model=_StubTrend()))
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(pb["params"]))
    P = point_prediction.Predictor(mod, fields.MultiField(fs), max_neighbours=(5, 6))
    yield P, pb
    P.close()


def _frame(out):
    from sif_xco2_cokriging_amd import joint_prediction
    return out if joint_prediction.xr is None else out.to_dataframe()


def test_predictor_predict_pair(native, predictor):
    from sif_xco2_cokriging_amd import joint_prediction
    P, pb = predictor
    pc = np.vstack([pb["sites"], [[-60.0, 20.0]]])   # the last site has no datum within 900 km
    with pytest.warns(UserWarning, match="No data within maximum distance 900.0 at 1 location"):
        p0, e0, p1, e1, cov = P.predict_pair_arrays(pc, max_dist=900.0)
    assert P.info["n_empty"] == 1 and P.info["n_capped"] > 0 and np.isnan(cov[-1])
    with pytest.warns(UserWarning):
        a, b = P.predict_arrays(0, pc, max_dist=900.0), P.predict_arrays(1, pc, max_dist=900.0)
    for got, want in [(p0, a[0]), (e0, a[1]), (p1, b[0]), (e1, b[1])]:
        assert np.array_equal(got, want, equal_nan=True)
    with pytest.warns(UserWarning):
        raw = _frame(P.predict_pair(pc, max_dist=900.0, postprocess=False))
        out = _frame(P.predict_pair(pc, max_dist=900.0, postprocess=True))
    assert set(raw.columns) >= {"pred_0", "pred_err_0", "pred_1", "pred_err_1", "pred_cov", "pred_corr"} and len(raw) == len(pc)
    if joint_prediction.xr is None:   # (a Dataset is indexed by the sorted coordinates)
        assert np.array_equal(raw["pred_cov"].values, cov, equal_nan=True) and np.array_equal(raw["pred_0"].values, p0, equal_nan=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(e0 * e1 > 0, cov / (e0 * e1), np.nan)
        assert np.array_equal(raw["pred_corr"].values, want, equal_nan=True)
        assert np.all(np.abs(want[:-1]) < 1.0)
        assert np.allclose(out["pred_cov"].values, 1.7 * 0.6 * cov, rtol=1e-14, atol=0, equal_nan=True)
        assert np.allclose(out["pred_err_1"].values, 0.6 * e1, rtol=1e-14, atol=0, equal_nan=True)
        assert np.allclose(out["pred_corr"].values, want, rtol=1e-12, atol=0, equal_nan=True)


def test_predictor_predict_pair_refusals(native, predictor):
    """both are raised before any device work: the handle is replaced by one that fails on use"""
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    P, pb = predictor
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(pb["params"]))
    fs = [fields.Field(pb["coords"][k], pb["values"][k]) for k in range(2)]
    Q = point_prediction.Predictor(mod, fields.MultiField(fs))

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    Q._handle = no_device
    with pytest.raises(ValueError, match="different neighbourhoods"):
        Q.predict_pair(pb["sites"], max_dist=900.0, pcoords1=pb["sites"][:3])
    Q.trend = "constant"
    with pytest.raises(NotImplementedError, match="simple cokriging only"):
        Q.predict_pair(pb["sites"], max_dist=900.0)
    with pytest.raises(NotImplementedError, match="simple cokriging only"):
        Q.predict_pair_arrays(pb["sites"], max_dist=900.0)
    Q.trend, Q.devices = None, [0, 1]                     # more than one device: refused as predict_blocks is
    with pytest.raises(NotImplementedError, match=r"predict_pair runs on one device; this predictor has devices=\[0, 1\]"):
        Q.predict_pair(pb["sites"], max_dist=900.0)
    with pytest.raises(NotImplementedError, match=r"conditional simulation runs on one device; this predictor has devices=\[0, 1\]"):
        Q.conditional_simulation((0, 1), pb["sites"], 900.0, 2)
    Q.devices = None


# ---- 5. co-simulation (ck_simulate_local_pair) --------------------------------------------------------------------------------
# The stacked sites: index k for site k of process 0, m0 + k for site k of process 1.  Members, counts and stats4 exactly against
# tests/local_pair_ref.local_cosim_reference; weights, means, variances at RTOL / ATOL; draws at rtol 1e-8 and atol 1e-8
# sqrt(sigma_q^2 + nugget_q) of the column's process.
def cosim_case(name):
    from oracle import cokrige_oracle as orc
    from sif_xco2_cokriging_amd import synth
    from tests import local_sim_ref as ls
    key = ("cosim", name)
    if key in _cache:
        return _cache[key]
    noise = None
    rng = np.random.default_rng(7)
    if name in ("m25", "m150"):   # rows 2 / 3 of tests/local_sim_ref.py with sites of both processes, five of them co-located
        m = 25 if name == "m25" else 150
        pb = dict(ls.row_inputs(2 if name == "m25" else 3))
        s0, s1 = rng.random((m, 2)), rng.random((m, 2))
        s1[:5] = s0[3:8]
        pb.update(sites0=s0, sites1=s1, ranks=rng.permutation(2 * m).astype(np.int64))
    elif name == "haversine":
        cp = synth.conus_problem(60)
        s0 = np.column_stack([rng.uniform(24, 56, 20), rng.uniform(-123, -67, 20)])
        s1 = np.column_stack([rng.uniform(24, 56, 20), rng.uniform(-123, -67, 20)])
        s1[:3] = s0[:3]
        pb = dict(params=cp["params"], coords=cp["coords"], values=cp["values"], metric=HAV, sites0=s0, sites1=s1,
                  ranks=rng.permutation(40).astype(np.int64), caps=(6, 6), max_dist=800.0)
    elif name in ("full", "full_noise"):   # every datum and every earlier stacked site in every set: 40 data + 23 sites = 63
        pb = dict(ls.row_inputs(4))
        s0, s1 = rng.random((12, 2)), rng.random((12, 2))
        s1[:2] = s0[:2]
        pb.update(sites0=s0, sites1=s1, ranks=rng.permutation(24).astype(np.int64))
        if name == "full_noise":
            nr = np.random.default_rng(21)
            noise = [0.05 + 0.1 * nr.random(20), 0.02 + 0.1 * nr.random(20)]
    else:
        raise KeyError(name)
    ref = lp.local_cosim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["sites0"], pb["sites1"], pb["ranks"],
                                   pb["max_dist"], pb["caps"], noise=noise)
    assert ref["gap"] > 1e-9, (name, ref["gap"])   # numpy and the device must agree on every set
    assert ref["info"] == 0
    p = orc.Params.from_flat(pb["params"])
    m0 = len(pb["sites0"])
    c0 = np.concatenate([np.full(len(pb[s]), p.sigma[q] ** 2 + p.nugget[q]) for q, s in enumerate(("sites0", "sites1"))])
    pb = dict(pb, noise=noise, c0=c0, N=sum(len(c) for c in pb["coords"]), m0=m0, m=m0 + len(pb["sites1"]))
    _cache[key] = (pb, ref)
    return _cache[key]


def cosim_handle(native, pb, **options):
    return make_handle(native, pb["params"], pb["metric"], pb["coords"], pb["values"], pb["caps"], pb["noise"], **options)


def padded(rows, fill, dtype):
    out = np.full((len(rows), 64), fill, dtype=dtype)
    for t, r in enumerate(rows):
        out[t, :len(r)] = r
    return out


def cosim(h, pb, n_draws, **kw):
    return h.simulate_local_pair(pb["sites0"], pb["sites1"], pb["ranks"], pb["max_dist"], n_draws, **kw)


@pytest.mark.parametrize("name", ["m25", "m150", "haversine"])
def test_cosim_sets_weights_and_recursion(native, name):
    pb, ref = cosim_case(name)
    h = cosim_handle(native, pb)
    idx, w = h.simulate_local_pair_weights(pb["sites0"], pb["sites1"], pb["ranks"], pb["max_dist"])
    assert np.array_equal(idx, padded(ref["members"], -1, np.int64)), name     # the member lists, exactly
    wr = padded(ref["weights"], 0.0, np.float64)
    eps = np.random.default_rng(5).standard_normal((6, pb["m"]))
    Y, info, st = cosim(h, pb, 6, noise=eps)
    print(f"{name}: max |dw| {np.max(np.abs(w - wr)):.2e}, max |dmean| {np.max(np.abs(st['mean'] - ref['mean'])):.2e}, "
          f"max rel dvar {np.max(np.abs(st['var'] - ref['var']) / ref['var']):.2e}, k_max {st['k_max']}, levels {st['n_levels']}")
    np.testing.assert_allclose(w, wr, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["mean"], ref["mean"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"], ref["var"], rtol=RTOL, atol=ATOL)
    assert info == 0
    assert np.array_equal(st["count"], ref["count"])
    assert ref["count"][:, 2].sum() > 0 and ref["count"][:, 3].sum() > 0     # sets hold earlier sites of both processes
    assert (st["n_empty"], st["k_max"], st["n_capped"], st["n_levels"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"],
                                                                            ref["n_levels"])
    # the recursion replayed in numpy on the device's own weights: at most 66 terms per site, <= 1e-11 (1 + max |Y|)
    N = pb["N"]
    pos = ref["pos"]
    want = np.full(eps.shape, np.nan)
    for t in np.argsort(pos):
        mem = idx[t][idx[t] >= 0]
        s = mem >= N
        want[:, t] = st["mean"][t] + want[:, mem[s] - N] @ w[t][:len(mem)][s] + np.sqrt(st["var"][t]) * eps[:, t]
    err, scale = np.max(np.abs(Y - want)), 1.0 + np.max(np.abs(want))
    print(f"{name}: recursion against its numpy replay: max |dY| {err:.2e}, bound {1e-11 * scale:.2e}")
    assert err <= 1e-11 * scale
    # end to end against the reference under the same noise
    full = ref["draws"](eps)
    print(f"{name}: draws against the reference: max |dY| {np.max(np.abs(Y - full)):.2e}")
    assert np.all(np.abs(Y - full) <= 1e-8 * np.abs(full) + 1e-8 * np.sqrt(pb["c0"])[None, :])
    h.close()


@pytest.mark.parametrize("name", ["full", "full_noise"])
def test_cosim_full_conditioning_is_the_stacked_dense_posterior(native, name):
    pb, ref = cosim_case(name)
    h = cosim_handle(native, pb)
    eps = np.random.default_rng(5).standard_normal((6, pb["m"]))
    Y, info, st = cosim(h, pb, 6, noise=eps)
    pred, L, order = lp.dense_chain_pair(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["sites0"], pb["sites1"],
                                         pb["ranks"], noise=pb["noise"])
    want = np.empty(eps.shape)
    want[:, order] = eps[:, order] @ L.T
    want += pred
    print(f"{name}: draws against the stacked dense chain: max |dY| {np.max(np.abs(Y - want)):.2e}")
    assert info == 0 and (st["k_max"], st["n_levels"], st["n_empty"], st["n_capped"]) == (63, 24, 0, 0)
    assert np.all(np.abs(Y - want) <= 1e-8 * np.abs(want) + 1e-8 * np.sqrt(pb["c0"])[None, :])
    h.close()


def test_cosim_with_one_empty_site_set_is_the_single_call(native):
    pb, _ = cosim_case("m25")
    h = cosim_handle(native, pb)
    rng = np.random.default_rng(3)
    for q, key in ((0, "sites0"), (1, "sites1")):
        sites, ranks = pb[key], rng.permutation(25).astype(np.int64)
        for kw in (dict(seed=77), dict(noise=rng.standard_normal((5, 25)))):
            a, ia, sa = h.simulate_local(q, sites, ranks, pb["max_dist"], 5, **kw)
            pair = (sites, None) if q == 0 else (None, sites)
            b, ib, sb = h.simulate_local_pair(*pair, ranks, pb["max_dist"], 5, **kw)
            assert ia == ib == 0 and np.array_equal(a, b)
            assert np.array_equal(sa["mean"], sb["mean"]) and np.array_equal(sa["var"], sb["var"])
            assert np.array_equal(sa["count"][:, :2], sb["count"][:, :2]) and np.array_equal(sa["count"][:, 2], sb["count"][:, 2 + q])
            assert not sb["count"][:, 3 - q].any()
            assert {k: sa[k] for k in ("n_empty", "k_max", "n_capped", "n_levels")} == {k: sb[k] for k in ("n_empty", "k_max", "n_capped", "n_levels")}
        i1, w1 = h.simulate_local_weights(q, sites, ranks, pb["max_dist"])
        i2, w2 = h.simulate_local_pair_weights(*pair, ranks, pb["max_dist"])
        assert np.array_equal(i1, i2) and np.array_equal(w1, w2)
    h.close()


def test_cosim_device_normals_and_chunking(native):
    """The device's normals, keyed on (stacked index, d / 2), against the host's Philox (tests/host_rng_shim.cpp) carried through
    the recursion (the bound of tests/test_gpu_local_simulation.py), and the bits of draws 0 - 4 across n_draws, draw_chunk and
    repeated calls."""
    from tests.test_gpu_local_simulation import host_normals
    pb, ref = cosim_case("m150")
    m, seed = pb["m"], 2024
    h = cosim_handle(native, pb)
    eps = host_normals(seed, m, 37)
    Yn, info, _ = cosim(h, pb, 37, noise=eps)
    Y37, info2, _ = cosim(h, pb, 37, seed=seed)
    assert info == 0 and info2 == 0
    bound = np.zeros_like(eps)
    for t in np.argsort(ref["pos"]):
        u, wu = ref["nbr_sites"][t], np.abs(ref["weights"][t][ref["members"][t] >= pb["N"]])
        sd = np.sqrt(ref["var"][t])
        size = np.abs(ref["mean"][t]) + np.abs(Yn[:, u]) @ wu + sd * np.abs(eps[:, t])
        bound[:, t] = bound[:, u] @ wu + sd * 2 * np.spacing(np.abs(eps[:, t])) + 66 * 2.0 ** -52 * size
    print(f"device normals against the host's: max |dY| {np.max(np.abs(Y37 - Yn)):.2e}, largest bound {bound.max():.2e}")
    assert np.all(np.abs(Y37 - Yn) <= bound)
    Y5 = cosim(h, pb, 5, seed=seed)[0]
    assert np.array_equal(Y5, Y37[:5]) and np.array_equal(cosim(h, pb, 5, seed=seed)[0], Y5)
    h.set_option("draw_chunk", 8)
    assert np.array_equal(cosim(h, pb, 37, seed=seed)[0], Y37) and np.array_equal(cosim(h, pb, 5, seed=seed)[0], Y5)
    assert np.array_equal(cosim(h, pb, 37, noise=eps)[0], Yn)
    assert not np.array_equal(cosim(h, pb, 5, seed=seed + 1)[0], Y5)
    h.close()


def test_cosim_a_set_of_65_is_refused_before_any_solve(native):
    pb, _ = cosim_case("full")
    rng = np.random.default_rng(7)
    s0, s1, ranks = rng.random((13, 2)), rng.random((13, 2)), rng.permutation(26).astype(np.int64)
    h = cosim_handle(native, pb)
    with pytest.raises(native.NativeError, match=r"ck_simulate_local_pair: 1 sites have a conditioning set of more than 64 data "
                                                 r"\(the largest: 65\); the draws are for sets the LDS solver takes"):
        h.simulate_local_pair(s0, s1, ranks, pb["max_dist"], 2)
    tm = h.simulate_local_timings()
    assert tm["select_ms"] > 0 and tm["weights_ms"] == 0 and tm["recursion_ms"] == 0       # the select pass ran, nothing else
    with pytest.raises(native.NativeError, match="ck_debug_simulate_local_pair_weights: 1 sites have a conditioning set of more than 64"):
        h.simulate_local_pair_weights(s0, s1, ranks, pb["max_dist"])
    h.close()


def test_cosim_identical_sites(native):
    """two sites of one process at one point are reported through info; the two processes at one point stop nothing"""
    pb, ref = cosim_case("m25")
    h = cosim_handle(native, pb)
    s1, ranks = pb["sites1"].copy(), pb["ranks"]
    a, b = (25 + 9, 25 + 17) if ranks[25 + 9] < ranks[25 + 17] else (25 + 17, 25 + 9)   # stacked; b is visited after a
    s1[b - 25] = s1[a - 25]
    eps = np.random.default_rng(5).standard_normal((3, 50))
    Y, info, st = h.simulate_local_pair(pb["sites0"], s1, ranks, pb["max_dist"], 3, noise=eps)
    assert st["count"][b, 3] >= 1 and info == b + 1
    assert np.all(np.isnan(Y[:, b])) and not np.any(np.isnan(Y[:, a]))
    # sites 0 - 4 of process 1 lie on sites 3 - 7 of process 0 (cosim_case): the reference run has info 0 and finite draws
    Y, info, st = cosim(h, pb, 3, noise=eps)
    assert info == 0 and np.all(np.isfinite(Y)) and np.all(st["var"] > 0)
    later = [max(3 + k, 25 + k, key=lambda t: ranks[t]) for k in range(5)]
    assert all(st["count"][t, 2 if t >= 25 else 3] >= 1 for t in later)   # each conditions on its partner of the other process
    h.close()


def test_cosim_refusals_and_state(native):
    pb, _ = cosim_case("m25")
    h = cosim_handle(native, pb)
    s0, s1, ranks, md = pb["sites0"], pb["sites1"], pb["ranks"], pb["max_dist"]
    E = native.NativeError
    with pytest.raises(E, match="ck_simulate_local_pair: m = 0 sites; at least 1"):
        h.simulate_local_pair(None, None, np.zeros(0, dtype=np.int64), md, 2)
    with pytest.raises(E, match="ck_simulate_local_pair: n_draws = 0; at least 1"):
        h.simulate_local_pair(s0, s1, ranks, md, 0)
    with pytest.raises(E, match="ck_simulate_local_pair: max_dist must be finite and >= 0"):
        h.simulate_local_pair(s0, s1, ranks, -1.0, 2)
    dup = ranks.copy()
    lo, hi = sorted((3, 25 + 4))
    dup[hi] = dup[lo]
    with pytest.raises(E, match=f"ck_simulate_local_pair: sites {lo} and {hi} have the same rank {dup[lo]}"):
        h.simulate_local_pair(s0, s1, dup, md, 2)
    with pytest.raises(E, match="ck_debug_simulate_local_pair_weights: sites"):
        h.simulate_local_pair_weights(s0, s1, dup, md)
    import ctypes
    ip = ctypes.POINTER(ctypes.c_int64)
    rc = native.lib().ck_simulate_local_pair(h._h, None, 25, None, 0, ranks.ctypes.data_as(ip), md, 2, 0, None, None, None, None, None,
                                             None, None)
    assert rc != 0 and b"ck_simulate_local_pair: null pcoords0_host" in native.lib().ck_last_error()
    p0 = s0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    L, rk, err = native.lib(), ranks.ctypes.data_as(ip), native.lib().ck_last_error
    out = np.zeros(64)
    dp, st = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), np.zeros(4, dtype=np.int64)
    tail = (rk, md, 2, 0, None, dp, None, None, None, st.ctypes.data_as(ip), st.ctypes.data_as(ip))
    # (none of these reads a coordinate or a rank: the 25-row buffers stand for any size)
    assert L.ck_simulate_local_pair(h._h, p0, 2 ** 31, None, 0, *tail) != 0
    assert b"ck_simulate_local_pair: more than 2^31 - 1 data and sites" in err()
    assert L.ck_simulate_local_pair(h._h, p0, 2 ** 31 - 1 - 80, p0, 1, *tail) != 0      # N = 80: N + m0 + m1 = 2^31
    assert b"ck_simulate_local_pair: more than 2^31 - 1 data and sites" in err()
    assert L.ck_simulate_local_pair(h._h, p0, -1, p0, 25, *tail) != 0
    assert b"ck_simulate_local_pair: m0 = -1, m1 = 25; both must be >= 0" in err()
    assert L.ck_simulate_local_pair(h._h, p0, 25, p0, -3, *tail) != 0
    assert b"ck_simulate_local_pair: m0 = 25, m1 = -3; both must be >= 0" in err()
    assert L.ck_simulate_local_pair(h._h, p0, 25, None, 5, *tail) != 0
    assert b"ck_simulate_local_pair: null pcoords0_host / pcoords1_host" in err()
    wi = np.zeros(64, dtype=np.int64).ctypes.data_as(ip)
    assert L.ck_debug_simulate_local_pair_weights(h._h, p0, 25, p0, 25, rk, md, None, dp) != 0
    assert b"ck_debug_simulate_local_pair_weights: null rank_host / idx_host / w_host" in err()
    assert L.ck_debug_simulate_local_pair_weights(h._h, p0, 25, p0, 25, None, md, wi, dp) != 0
    assert b"ck_debug_simulate_local_pair_weights: null rank_host / idx_host / w_host" in err()
    assert L.ck_debug_simulate_local_pair_weights(h._h, p0, 25, None, 5, rk, md, wi, dp) != 0
    assert b"ck_debug_simulate_local_pair_weights: null pcoords0_host / pcoords1_host" in err()
    assert L.ck_debug_simulate_local_pair_weights(h._h, p0, -1, p0, 25, rk, md, wi, dp) != 0
    assert b"ck_debug_simulate_local_pair_weights: m0 = -1, m1 = 25; both must be >= 0" in err()
    assert L.ck_debug_simulate_local_pair_weights(h._h, p0, 2 ** 31, None, 0, rk, md, wi, dp) != 0
    assert b"ck_debug_simulate_local_pair_weights: more than 2^31 - 1 data and sites" in err()
    rc = native.lib().ck_simulate_local_pair(h._h, p0, 25, None, 0, ranks.ctypes.data_as(ip), md, 2, 0, None, None, None, None, None,
                                             None, None)
    assert rc != 0 and b"ck_simulate_local_pair: null rank_host / draws_host / stats4 / info" in native.lib().ck_last_error()
    # the caller's handle: a resident factor and the bits of predict / predict_local / simulate_local across the new calls
    grid = np.random.default_rng(4).random((70, 2))
    h.assemble_joint()
    assert h.factor() == 0
    r25 = np.random.default_rng(1).permutation(25).astype(np.int64)
    before = [h.predict(0, grid), h.predict_local(0, grid, max_dist=md)[:2], (h.simulate_local(1, s1, r25, md, 4, seed=9)[0],)]
    h.simulate_local_pair(s0, s1, ranks, md, 4, seed=9)
    h.simulate_local_pair_weights(s0, s1, ranks, md)
    h.predict_local_pair(grid, max_dist=md)
    after = [h.predict(0, grid), h.predict_local(0, grid, max_dist=md)[:2], (h.simulate_local(1, s1, r25, md, 4, seed=9)[0],)]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert np.array_equal(u, v, equal_nan=True)
    assert h.verify_model() == 0
    h.set_trend(0, np.ones((40, 1)))
    with pytest.raises(E, match="ck_simulate_local_pair: a trend of 1 columns"):
        h.simulate_local_pair(s0, s1, ranks, md, 2)
    h.close()
    one = native.Handle(0)
    pv = pb["params"]
    one.set_model(1, pv[0:1], pv[2:3], pv[5:6], pv[8:9])
    one.set_metric(pb["metric"])
    one.set_data(0, pb["coords"][0], pb["values"][0])
    with pytest.raises(E, match="ck_simulate_local_pair: needs a model of two processes"):
        one.simulate_local_pair(s0, s1, ranks, md, 2)
    one.close()
    q = native.Handle(devices=[0, 0], rank=0)
    with pytest.raises(E, match="ck_simulate_local_pair .* partitioned"):
        q.simulate_local_pair(s0, s1, ranks, md, 2)
    q.close()


def test_predictor_pair_conditional_simulation(native, predictor):
    from sif_xco2_cokriging_amd import joint_prediction
    P, pb = predictor
    pc0 = np.vstack([pb["sites"], pb["sites"][[2]]])            # a repeated row of process 0: pinned to its first occurrence
    pc1 = np.vstack([pb["sites"][:4] + 0.25, pb["coords"][1][[5]]])   # the last site of process 1 lies on one of its data
    draws, pred, err, pinned, seed = P.conditional_draws_arrays((0, 1), pc0, 900.0, 6, seed=11, pcoords1=pc1)
    assert seed == 11 and draws.shape == (6, 10 + 5) and pred.shape == err.shape == (15,)
    assert np.array_equal(draws[:, 9], draws[:, 2]) and np.all(draws[:, 14] == pb["values"][1][5])
    assert pinned[9] and pinned[14] and pinned.sum() == 2
    assert P.sim_info["n_pinned"] == 2 and P.sim_info["ordering"] == "random" and P.sim_info["n_levels"] >= 1
    free = np.flatnonzero(~pinned)
    from sif_xco2_cokriging_amd.vecchia import ordering_ranks
    ranks = ordering_ranks([pc0[:9], pc1[:4]], "random", 11)
    ref = P._capped_handle().simulate_local_pair(pc0[:9], pc1[:4], ranks, 900.0, 6, seed=11)[0]
    assert np.array_equal(draws[:, free], ref)
    eps = np.random.default_rng(2).standard_normal((6, 15))
    a = P.conditional_draws_arrays((0, 1), pc0, 900.0, 6, seed=11, pcoords1=pc1, noise=eps)[0]
    b = P._capped_handle().simulate_local_pair(pc0[:9], pc1[:4], ranks, 900.0, 6, noise=eps[:, free])[0]
    assert np.array_equal(a[:, free], b)
    out0, out1 = P.conditional_simulation((0, 1), pc0, 900.0, 6, seed=11, postprocess=False, pcoords1=pc1)
    if joint_prediction.xr is None:
        (df0, d0), (df1, d1) = out0, out1
        assert d0.shape == (6, 10) and d1.shape == (6, 5) and np.array_equal(np.hstack([d0, d1]), draws)
        assert df0.attrs["seed"] == 11 and df1.attrs["n_pinned"] == 2 and df0.attrs["ordering"] == "random"
        (pf0, e0), (pf1, e1) = P.conditional_simulation((0, 1), pc0, 900.0, 6, seed=11, postprocess=True, pcoords1=pc1)
        assert np.allclose(e1 - pf1["pred"].values, 0.6 * (d1 - df1["pred"].values), rtol=0, atol=1e-12)
    else:
        assert out0["draws"].dims[0] == "draw" and out0.attrs["seed"] == 11 and out1.attrs["n_pinned"] == 2
    same = P.conditional_draws_arrays((0, 1), pb["sites"], 900.0, 3, seed=2)     # the same sites for both by default
    assert same[0].shape == (3, 18)
    with pytest.raises(ValueError, match="the joint form is i=\\(0, 1\\)"):
        P.conditional_draws_arrays((1, 0), pc0, 900.0, 2)
    with pytest.raises(ValueError, match="noise has shape"):
        P.conditional_draws_arrays((0, 1), pc0, 900.0, 2, pcoords1=pc1, noise=np.zeros((2, 10)))
