"""GPU tests of the Vecchia likelihood on the local solver: include/cokrige.h ck_loglik_vecchia, native.Handle.loglik_vecchia,
vecchia.Vecchia and MultivariateMatern.log_likelihood / vecchia_terms / fit_likelihood(vecchia=...).

A. the selection with precedence, bit for bit, on the lattice of tests/test_gpu_local_nmax.py (coordinates on multiples of 1/8:
   the device distance equals numpy's, ties included), on three handles: defaults, the re-scan path, the caller's site order;
B. terms and totals on random sites against the numpy loop of tests/vecchia_ref.py, caps (4,4) .. (32,32) and an uncapped radius
   whose sets straddle the LDS limit (also through k_local_solve_big);
C. exactness under full conditioning: the dense numpy log-density, ck_loglik on a second handle, two orderings;
D. measurement-error variances, one process, haversine;
E. state and refusals;
F. the Python layer and the fit.
Per datum the tolerances are the local path's own (tests/test_gpu_local.py): rtol 1e-8, atol 1e-10 on the mean and on the
variance.  For the totals the bound is computed from the reference's terms (vecchia_ref.totals_bound):
    sum_t |e_t| / s_t^2 tol(mu_t) + 1/2 |1 / s_t^2 - e_t^2 / s_t^4| tol(s_t^2)."""
import ctypes

import numpy as np
import pytest
from numpy.linalg import LinAlgError

from oracle import cokrige_oracle as orc
from tests import vecchia_ref as vr

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_handle(native, params, metric, coords, values, **options):
    h = native.Handle(0)
    for name, value in options.items():
        h.set_option(name, value)
    pv = list(params)
    if len(coords) == 2:
        h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    else:
        h.set_model(1, pv[0:1], pv[1:2], pv[2:3], pv[3:4])
    h.set_metric(metric)
    for k in range(len(coords)):
        h.set_data(k, coords[k], values[k])
    return h


def check_against(ref, out3, info, st, label=""):
    """mean / var per datum, the three totals within the bound of the reference's terms, the counters"""
    assert info == ref["info"] == 0, (label, info)
    assert np.array_equal(st["count"], ref["count"]), label
    print(f"{label}: max |dmean| {np.max(np.abs(st['mean'] - ref['mean'])):.2e}, max rel dvar "
          f"{np.max(np.abs(st['var'] - ref['var']) / ref['var']):.2e}, out3 - ref {out3 - ref['out3']}, "
          f"bound {vr.totals_bound(ref, RTOL, ATOL)[2]:.2e}, k_max {st['k_max']}")
    np.testing.assert_allclose(st["mean"], ref["mean"], rtol=RTOL, atol=ATOL, err_msg=label)
    np.testing.assert_allclose(st["var"], ref["var"], rtol=RTOL, atol=ATOL, err_msg=label)
    bound = vr.totals_bound(ref, RTOL, ATOL)[2]
    for k in range(3):
        assert abs(out3[k] - ref["out3"][k]) <= bound, (label, k, out3[k], ref["out3"][k], bound)
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"]), label


# ---------------------------------------------------------------------------------------------------------------------
# A. selection with precedence, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def lattice():
    """process 0 on a 24 x 24 lattice of spacing 1/4, process 1 on its even nodes: 576 + 144 sites, more than two 256-site
    chunks; a random ranking"""
    if "lattice" not in _cache:
        g = np.arange(24) * 0.25
        X, Y = np.meshgrid(g, g, indexing="ij")
        c0 = np.column_stack([X.ravel(), Y.ravel()])
        c1 = np.column_stack([X[::2, ::2].ravel(), Y[::2, ::2].ravel()])
        assert np.array_equal(c0 * 8, np.round(c0 * 8))
        rng = np.random.default_rng(8)
        values = [rng.standard_normal(len(c0)), rng.standard_normal(len(c1))]
        ranks = np.random.default_rng(9).permutation(len(c0) + len(c1)).astype(np.int64)
        D, proc = vr.stacked_distances([c0, c1], EUC)
        _cache["lattice"] = ([c0, c1], values, ranks, D, proc)
    return _cache["lattice"]


@pytest.fixture(scope="module")
def lattice_handles(native):
    from sif_xco2_cokriging_amd import synth
    coords, values = lattice()[:2]
    hs = {"default": make_handle(native, synth.SET_B_UNIT, EUC, coords, values),
          "rescan": make_handle(native, synth.SET_B_UNIT, EUC, coords, values, local_select_cap=16),
          "caller_order": make_handle(native, synth.SET_B_UNIT, EUC, coords, values, site_order=0)}
    yield hs
    for h in hs.values():
        h.close()


CAPS_A = [(1, 1), (2, 3), (4, 4), (64, 64), (0, 0)]


@pytest.mark.parametrize("max_dist", [0.3, 1.0])
def test_selection_with_precedence_bit_for_bit(lattice_handles, max_dist):
    coords, values, ranks, D, proc = lattice()
    n_ties = n_rescan = n_colocated = 0
    first = int(np.argmin(ranks))
    for caps in CAPS_A:
        keep, gap, capped = vr.conditioning_sets(D, proc, ranks, max_dist, caps)
        ref_count = np.column_stack([np.count_nonzero(keep & (proc == q)[None, :], axis=1) for q in range(2)])
        assert not np.any(keep & (ranks[None, :] >= ranks[:, None]))          # only earlier data
        if caps != (0, 0):
            n_ties += int(np.count_nonzero(ref_count > np.array(caps)))
        n_colocated += int(np.count_nonzero(keep & (D == 0.0)))               # an earlier co-located partner in the set
        for name, h in lattice_handles.items():
            h.set_local_neighbours(*caps)
            out3, info, st = h.loglik_vecchia(ranks, max_dist, terms=True)
            assert np.array_equal(st["count"], ref_count), (name, caps)       # ties included
            assert st["count"][first].sum() == 0 and st["mean"][first] == 0.0 # the datum of rank 0: an empty set
            ktot = ref_count.sum(axis=1)
            assert (st["n_empty"], st["k_max"], st["n_capped"]) == (np.count_nonzero(ktot == 0), ktot.max(),
                                                                    np.count_nonzero(capped)), (name, caps)
            t = h.timings()
            assert t["local_n_capped"] == np.count_nonzero(capped)
            if name == "rescan":
                n_rescan += t["local_n_rescan"]
            else:
                assert t["local_n_rescan"] == 0
            tv = h.vecchia_timings()
            assert tv["n_lds"] == np.count_nonzero(ktot <= 64) and tv["n_tiled"] == np.count_nonzero(ktot > 64)
            assert tv["select_ms"] > 0 and tv["total_ms"] > 0
    assert n_ties > 0                       # strictly more than the cap where the cut distance is shared
    assert n_colocated > 0                  # the case occurs: d = 0 is a legitimate conditioning datum
    assert n_rescan > 0 or max_dist < 1.0   # 16 keys per process: the 1.0 radius goes through the re-scan path


# ---------------------------------------------------------------------------------------------------------------------
# B. terms and totals on random sites
# ---------------------------------------------------------------------------------------------------------------------
def random_problem():
    """n = 150 per process uniform on the unit square, half of process 1 co-located with process 0; SET_B_UNIT, Euclid"""
    if "random" not in _cache:
        from sif_xco2_cokriging_amd import synth
        coords, values = vr.half_colocated_sites(150)
        ranks = np.random.default_rng(11).permutation(300).astype(np.int64)
        _cache["random"] = dict(coords=coords, values=values, params=list(synth.SET_B_UNIT), ranks=ranks, metric=EUC)
    return _cache["random"]


def reference(pb, max_dist, caps, ranks=None, noise=None, key=None):
    key = ("ref", id(pb), max_dist, caps, key)
    if key not in _cache:
        ref = vr.vecchia_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["ranks"] if ranks is None else ranks,
                                   max_dist, caps, noise=noise)
        assert ref["gap"].min() > 1e-9, (caps, ref["gap"].min())   # numpy and the device must agree on every set: no datum left out
        _cache[key] = ref
    return _cache[key]


@pytest.fixture(scope="module")
def random_handle(native):
    pb = random_problem()
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    yield h
    h.close()


@pytest.mark.parametrize("caps", [(4, 4), (16, 16), (32, 32)])
def test_capped_terms_and_totals(random_handle, caps):
    pb = random_problem()
    ref = reference(pb, 0.5, caps)
    h = random_handle
    h.set_local_neighbours(*caps)
    out3, info, st = h.loglik_vecchia(pb["ranks"], 0.5, terms=True)
    check_against(ref, out3, info, st, f"caps {caps}")
    assert ref["n_capped"] > 0 and ref["var"].min() > 0.02
    if caps == (32, 32):
        assert ref["k_max"] == 64                                   # the largest system the LDS class takes


@pytest.mark.parametrize("tile_min", [None, 128])
def test_uncapped_radius_straddles_the_lds_limit(native, random_handle, tile_min):
    pb = random_problem()
    ref = reference(pb, 0.3, (0, 0))
    ktot = ref["count"].sum(axis=1)
    assert ktot.min() == 0 and 64 < ktot.max() <= 128 and np.count_nonzero(ktot == 64) + np.count_nonzero(ktot == 65) > 0
    h = random_handle if tile_min is None else make_handle(native, pb["params"], EUC, pb["coords"], pb["values"],
                                                           local_tile_min=tile_min)   # 128: k_local_solve_big runs the predicate
    h.set_local_neighbours(0, 0)
    out3, info, st = h.loglik_vecchia(pb["ranks"], 0.3, terms=True)
    check_against(ref, out3, info, st, f"uncapped, local_tile_min {tile_min}")
    tv = h.vecchia_timings()
    assert tv["n_lds"] > 0 and tv["n_tiled"] > 0                    # both classes
    assert tv["n_lds"] == np.count_nonzero(ktot <= 64) and tv["n_tiled"] == np.count_nonzero(ktot > 64)
    assert tv["solve_ms"] > 0 and tv["terms_ms"] > 0
    if tile_min is not None:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. exactness under full conditioning
# ---------------------------------------------------------------------------------------------------------------------
def test_full_conditioning_is_the_dense_likelihood(native, random_handle):
    from sif_xco2_cokriging_amd import vecchia
    pb = random_problem()
    dense = vr.dense_logpdf(pb["params"], pb["coords"], pb["values"], EUC)
    h2 = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h2.assemble_joint()
    info2, out3_dense, _ = h2.loglik(False)
    h2.close()
    assert info2 == 0
    h = random_handle
    h.set_local_neighbours(0, 0)
    got = []
    for ordering in ("random", "hilbert"):
        ranks = vecchia.ordering_ranks(pb["coords"], ordering, 1)
        ref = reference(pb, 2.0, (0, 0), ranks=ranks, key=ordering)   # 2.0: above the domain's diameter
        assert ref["k_max"] == 299 and ref["n_empty"] == 1
        out3, info, st = h.loglik_vecchia(ranks, 2.0, terms=True)
        check_against(ref, out3, info, st, f"full conditioning, {ordering}")
        bound = vr.totals_bound(ref, RTOL, ATOL)[2]
        for k in range(3):
            assert abs(out3[k] - dense[k]) <= bound, (ordering, k, out3[k], dense[k], bound)
            assert abs(out3[k] - out3_dense[k]) <= bound, (ordering, k, out3[k], out3_dense[k], bound)
        got.append((out3, bound))
    for k in range(3):
        assert abs(got[0][0][k] - got[1][0][k]) <= 2 * max(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# D. noise, one process, haversine
# ---------------------------------------------------------------------------------------------------------------------
def test_measurement_error_variances(native):
    pb = random_problem()
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(150)
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.set_noise(0, d0, 2.0)                                          # d > 0 on process 0 only, scale 2
    h.set_local_neighbours(16, 16)
    ref = reference(pb, 0.5, (16, 16), noise=[2.0 * d0, None], key="noise")
    out3, info, st = h.loglik_vecchia(pb["ranks"], 0.5, terms=True)
    check_against(ref, out3, info, st, "noise on process 0")
    plain = reference(pb, 0.5, (16, 16))
    assert np.all(ref["var"][:150] > plain["var"][:150])             # the datum's own s d is in its variance
    h.close()


def test_univariate_model(native):
    pb = random_problem()
    uni = dict(coords=pb["coords"][:1], values=pb["values"][:1], params=[1.0, 1.5, 0.2, 0.02], metric=EUC,
               ranks=np.random.default_rng(12).permutation(150).astype(np.int64))
    _cache["uni"] = uni
    h = make_handle(native, uni["params"], EUC, uni["coords"], uni["values"])
    for caps, max_dist in (((8, 0), 0.5), ((0, 0), 0.8)):
        h.set_local_neighbours(*caps)
        ref = reference(uni, max_dist, caps[:1])
        out3, info, st = h.loglik_vecchia(uni["ranks"], max_dist, terms=True)
        assert np.all(st["count"][:, 1] == 0)
        ref = dict(ref, count=np.column_stack([ref["count"][:, 0], np.zeros(150, dtype=np.int64)]))
        check_against(ref, out3, info, st, f"univariate {caps}")
    h.close()


def test_haversine(native):
    """conus_problem's parameters and its half co-located sampling, n = 150 per process, on uniformly random sites (on the
    0.05-degree lattice symmetric sites tie up to rounding, and numpy's haversine is not the device's to the bit)"""
    from sif_xco2_cokriging_amd import synth
    rng = np.random.default_rng(4102)
    c0, c1 = synth.split_sites(np.column_stack([rng.uniform(30.0, 38.0, 225), rng.uniform(-105.0, -95.0, 225)]), 150)
    pb = dict(coords=[c0, c1], values=[rng.standard_normal(150), rng.standard_normal(150)], params=list(synth.SET_A), metric=HAV,
              ranks=np.random.default_rng(13).permutation(300).astype(np.int64))
    _cache["hav"] = pb
    D, _ = vr.stacked_distances(pb["coords"], HAV)
    max_dist = 250.0
    assert np.min(np.abs(D - max_dist)) > 1e-9 * max_dist          # no pair on the radius itself
    ref = reference(pb, max_dist, (12, 12))
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    h.set_local_neighbours(12, 12)
    out3, info, st = h.loglik_vecchia(pb["ranks"], max_dist, terms=True)
    check_against(ref, out3, info, st, "haversine")
    assert ref["n_capped"] > 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. state and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_give_the_same_bits(random_handle):
    pb = random_problem()
    h = random_handle
    for caps, max_dist in (((16, 16), 0.5), ((0, 0), 0.3)):
        h.set_local_neighbours(*caps)
        a = h.loglik_vecchia(pb["ranks"], max_dist, terms=True)
        b = h.loglik_vecchia(pb["ranks"], max_dist, terms=True)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 0
        for key in ("mean", "var", "count"):
            assert np.array_equal(a[2][key], b[2][key])
        shifted = h.loglik_vecchia(pb["ranks"] * 5 - 3, max_dist)    # any distinct integers: only their order counts
        assert np.array_equal(shifted[0], a[0])


def test_a_vecchia_call_leaves_the_factor_and_the_predictions(native):
    pb = random_problem()
    pc = np.random.default_rng(5).random((40, 2))
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.assemble_joint()
    assert h.factor() == 0
    before = h.predict(0, pc)
    h.set_local_neighbours(16, 16)
    out3, info, _ = h.loglik_vecchia(pb["ranks"], 0.5)
    assert info == 0 and np.isfinite(out3).all()
    after = h.predict(0, pc)                                         # no new assembly, no new factorisation
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    h.close()
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])   # and a handle that never saw a Vecchia call
    h.assemble_joint()
    assert h.factor() == 0
    fresh = h.predict(0, pc)
    assert np.array_equal(before[0], fresh[0]) and np.array_equal(before[1], fresh[1])
    h.close()


def test_refusals(native):
    pb = random_problem()
    ranks = pb["ranks"]
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    dup = ranks.copy()
    dup[200] = dup[17]
    with pytest.raises(native.NativeError, match=r"data 17 and 200 \(stacked order\) have the same rank " + str(int(ranks[17]))):
        h.loglik_vecchia(dup, 0.5)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(native.NativeError, match="max_dist must be finite and >= 0"):
            h.loglik_vecchia(ranks, bad)
    L = native.lib()
    out3, inf = np.zeros(3), ctypes.c_int64(0)
    rp = ranks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert L.ck_loglik_vecchia(h._h, None, 0.5, native._p(out3), None, None, None, None, ctypes.byref(inf)) != 0
    assert "null rank_host / out3" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia(h._h, rp, 0.5, None, None, None, None, None, ctypes.byref(inf)) != 0
    assert "null rank_host / out3" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia(h._h, rp, 0.5, native._p(out3), None, None, None, None, None) == 0   # every output but out3 is optional
    h.set_trend(0, np.ones((150, 1)))
    with pytest.raises(native.NativeError, match="a trend of 1 columns is set on the handle"):
        h.loglik_vecchia(ranks, 0.5)
    h.set_trend(0, None)
    assert h.loglik_vecchia(ranks, 0.5)[1] == 0
    with pytest.raises(ValueError, match="rank has 299 entries"):
        h.loglik_vecchia(ranks[:-1], 0.5)
    h.close()
    hp = native.Handle(devices=[0, 0], rank=0)                       # a partitioned handle: the single-process form only
    hp.set_model(2, pb["params"][0:2], pb["params"][2:5], pb["params"][5:8], pb["params"][8:10], pb["params"][10])
    hp.set_metric(EUC)
    for k in range(2):
        hp.set_data(k, pb["coords"][k], pb["values"][k])
    with pytest.raises(native.NativeError, match=r"single-process form: this handle is partitioned \(world = 2\)"):
        hp.loglik_vecchia(ranks, 0.5)
    hp.close()


def test_duplicate_sites_without_nugget_name_the_later_datum(native):
    """two sites of process 0 at the same place, far from everything else, nugget 0, no noise: the later of the two (by rank)
    is conditioned on its copy alone and has the variance 1 - 1 = 0"""
    pb = random_problem()
    coords = [pb["coords"][0].copy(), pb["coords"][1]]
    coords[0][3] = coords[0][10] = (5.0, 5.0)
    params = list(pb["params"])
    params[8] = params[9] = 0.0
    ranks = pb["ranks"].copy()
    if ranks[3] < ranks[10]:
        ranks[[3, 10]] = ranks[[10, 3]]                              # datum 3 is the later one, datum 10 its earlier copy
    ref = vr.vecchia_reference(params, coords, pb["values"], EUC, ranks, 0.5, (16, 16))
    assert ref["info"] == 4 and ref["var"][3] == 0.0 and ref["count"][3].tolist() == [1, 0] and ref["count"][10].sum() == 0
    assert np.all(np.isnan(ref["out3"])) and np.count_nonzero(np.isnan(ref["logv"])) == 1
    h = make_handle(native, params, EUC, coords, pb["values"])
    h.set_local_neighbours(16, 16)
    out3, info, st = h.loglik_vecchia(ranks, 0.5, terms=True)
    assert info == 4 and np.all(np.isnan(out3))
    assert np.array_equal(st["count"], ref["count"])
    ok = np.arange(300) != 3
    np.testing.assert_allclose(st["mean"][ok], ref["mean"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"][ok], ref["var"][ok], rtol=RTOL, atol=ATOL)
    assert not st["var"][3] > 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# F. the Python layer and the fit
# ---------------------------------------------------------------------------------------------------------------------
def _fields(coords, values):
    from sif_xco2_cokriging_amd import fields
    return fields.MultiField([fields.Field(coords[k], values[k]) for k in range(len(coords))])


def test_log_likelihood_and_terms_equal_the_native_call(native):
    from sif_xco2_cokriging_amd import model, vecchia
    pb = random_problem()
    mf = _fields(pb["coords"], pb["values"])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(pb["params"])
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(150)
    v = vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4)
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 4)
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.set_local_neighbours(16, 12)
    for me, scale in ((None, None), ([d0, None], (2.0, 1.0))):
        h.set_noise(0, None if me is None else d0, 1.0 if me is None else 2.0)
        out3, info, st = h.loglik_vecchia(ranks, 0.5, terms=True)
        ll = mod.log_likelihood(mf, dist_units=None, fast_dist=False, vecchia=v, measurement_error=me, noise_scale=scale)
        assert info == 0 and ll == out3[0]
        df = mod.vecchia_terms(mf, v, dist_units=None, fast_dist=False, measurement_error=me, noise_scale=scale)
        assert list(df.columns) == ["process", "index", "mean", "variance", "n0", "n1"] and len(df) == 300
        assert np.array_equal(df["mean"].values, st["mean"]) and np.array_equal(df["variance"].values, st["var"])
        assert np.array_equal(df[["n0", "n1"]].values, st["count"])
        assert df["process"].tolist() == [0] * 150 + [1] * 150 and df["index"].tolist() == list(range(150)) * 2
        assert np.array_equal(df.attrs["out3"], out3)
    h.close()
    c0 = pb["coords"][0].copy()
    c0[3] = c0[10] = (5.0, 5.0)                                      # a duplicate pair of process 0 on its own, nugget 0:
    dup = _fields([c0, pb["coords"][1]], pb["values"])              # the later of the two has the variance 0
    bad = model.MultivariateMatern(2)
    x = np.array(pb["params"])
    x[8:10] = 0.0
    bad.params.set_values(x)
    with pytest.raises(LinAlgError, match=r"datum \d+ \(stacked order\)"):
        bad.log_likelihood(dup, dist_units=None, fast_dist=False, vecchia=vecchia.Vecchia(0.5, max_neighbours=4))


def test_fit_with_full_conditioning_finds_the_dense_optimum(native):
    """N = 2 x 200 data simulated from known parameters; sigma_11, len_scale_11 and nugget_11 free.  The exact log-likelihood at
    the Vecchia optimum may not be more than 0.005 below the exact one at the dense optimum: a shift of t standard errors
    along any direction lowers l by t^2 / 2, so 0.005 is t = 0.1."""
    from sif_xco2_cokriging_amd import model, vecchia
    truth = [1.0, 0.8, 1.5, 1.5, 1.5, 450.0, 450.0, 450.0, 0.05, 0.03, 0.5]
    rng = np.random.default_rng(31)
    pts = np.column_stack([rng.uniform(25, 50, 300), rng.uniform(-120, -70, 300)])
    coords = [pts[:200].copy(), pts[100:300].copy()]
    S = orc.joint_cov(orc.Params.from_flat(truth), coords, HAV)
    z = np.linalg.cholesky(S) @ rng.standard_normal(400)
    mf = _fields(coords, [z[:200], z[200:]])
    start = list(truth)
    start[0], start[5], start[8] = 1.3, 600.0, 0.1
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    results = {}
    for label, v in (("dense", None), ("vecchia", vecchia.Vecchia(1e5, ordering="random", seed=2))):
        mod = model.MultivariateMatern(2)
        mod.params.set_values(start)
        names = list(mod.params.get_names())
        assert set(free) <= set(names)
        mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free], vecchia=v)
        r = mod.fit_result
        x = mod.params.get_values().astype(float)
        assert r.method == ("ML" if v is None else "Vecchia-ML") and r.n_free == 3 and r.free == free
        assert np.array_equal(np.delete(x, [0, 5, 8]), np.delete(np.array(start), [0, 5, 8]))
        exact = model.MultivariateMatern(2)
        exact.params.set_values(x)
        results[label] = (x, exact.log_likelihood(mf), r)
        print(f"{label}: x {x[[0, 5, 8]]}, exact l {results[label][1]:.6f}, reported {r.loglik:.6f}, n_eval {r.n_eval}, {r.message}")
    assert abs(results["vecchia"][2].loglik - results["vecchia"][1]) < 1e-6   # full conditioning: the value is the exact one
    assert results["vecchia"][1] >= results["dense"][1] - 0.005, (results["vecchia"][:2], results["dense"][:2])
