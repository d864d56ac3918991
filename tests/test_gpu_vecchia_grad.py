"""GPU tests of the analytic gradient of the Vecchia likelihood: include/cokrige.h ck_loglik_vecchia_grad,
native.Handle.loglik_vecchia_grad, vecchia.Vecchia(gradient="analytic") in MultivariateMatern.log_likelihood / fit_likelihood.

The reference is the numpy loop of tests/vecchia_grad_ref.py on the sets of tests/vecchia_ref.py (fourth-order block differences
of the oracle's covariance, a different formula from the device's analytic Matern derivatives); tests/test_vecchia_grad_host.py
ties it to differences of the reference's value.  The measure is the project's gradient measure |g - ref| / max(|ref|, 1)
(tests/test_gpu_likelihood.py: test_gradient_against_dense_differences), bound 1e-6, for the sum and for every datum's score.
The fixtures are those of tests/test_gpu_vecchia.py: 2 x 150 half co-located sites on the unit square, the ranks
default_rng(11).permutation(300), SET_B_UNIT (closed-form nu) and GEN = SET_A with the length scales 0.2 (generic nu)."""
import ctypes

import numpy as np
import pytest

from tests import dense_chains as dc
from tests import vecchia_grad_ref as vgr
from tests import vecchia_ref as vr

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
TOL = 1e-6
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


def parameter_set(name):
    from sif_xco2_cokriging_amd import synth
    if name == "SET_B_UNIT":
        return list(synth.SET_B_UNIT)
    if name == "SET_A":
        return list(synth.SET_A)
    gen = list(synth.SET_A)
    gen[5:8] = [0.2, 0.2, 0.2]
    return gen


def problem(name):
    if ("pb", name) not in _cache:
        coords, values = vr.half_colocated_sites(150)
        _cache["pb", name] = dict(coords=coords, values=values, params=parameter_set(name), metric=EUC,
                                  ranks=np.random.default_rng(11).permutation(300).astype(np.int64))
    return _cache["pb", name]


def small_problem(name):
    """N = 65: 33 + 32 sites, one conditioning set of 64 under full conditioning"""
    if ("small", name) not in _cache:
        coords, values = vr.half_colocated_sites(33)
        _cache["small", name] = dict(coords=[coords[0], coords[1][:32]], values=[values[0], values[1][:32]],
                                     params=parameter_set(name), metric=EUC)
    return _cache["small", name]


def reference(pb, max_dist, caps, ranks=None, noise_d=None, scales=(1.0, 1.0), key=None):
    """(the value's reference, the gradient's) -- computed once per case and left unchanged"""
    key = ("ref", id(pb), max_dist, caps, key)
    if key not in _cache:
        ranks = pb["ranks"] if ranks is None else ranks
        noise = None if noise_d is None else [None if d is None else scales[q] * d for q, d in enumerate(noise_d)]
        ref = vr.vecchia_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], ranks, max_dist, caps, noise=noise)
        assert ref["gap"].min() > 1e-9, (caps, ref["gap"].min())   # numpy and the device agree on every set: no datum left out
        dkey = ("dS", id(pb))
        if dkey not in _cache:
            _cache[dkey] = vgr.derivative_matrices(pb["params"], pb["coords"], pb["metric"])
        _cache[key] = (ref, vgr.vecchia_grad_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], ref, noise_d=noise_d,
                                                       scales=scales, dS=_cache[dkey]))
    return _cache[key]


def check_scores(got_grad, got_score, want, slots, label):
    eg = vgr.measure(got_grad[slots], want["grad13"][slots])
    es = vgr.measure(got_score[:, slots], want["score"][:, slots])
    print(f"{label}: gradient measure max {eg.max():.2e}, score measure max {es.max():.2e}")
    assert eg.max() < TOL, (label, got_grad, want["grad13"])
    assert es.max() < TOL, (label, np.unravel_index(np.argmax(es), es.shape))


@pytest.fixture(scope="module")
def handles(native):
    hs = {}
    for name in ("SET_B_UNIT", "GEN"):
        pb = problem(name)
        hs[name] = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    yield hs
    for h in hs.values():
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. capped sets against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
@pytest.mark.parametrize("caps", [(4, 4), (16, 16), (32, 32)])
def test_capped_gradient_and_scores(handles, name, caps):
    pb = problem(name)
    ref, want = reference(pb, 0.5, caps)
    ktot = ref["count"].sum(axis=1)
    assert ref["gap"].min() > 3e-5 and ref["info"] == 0 and ref["var"].min() > 0.029 - 1e-3
    assert ref["n_empty"] == 3 and ref["k_max"] == {4: 8, 16: 32, 32: 64}[caps[0]]
    h = handles[name]
    h.set_local_neighbours(*caps)
    value = h.loglik_vecchia(pb["ranks"], 0.5)
    out3, grad, info, st = h.loglik_vecchia_grad(pb["ranks"], 0.5, scores=True)
    assert info == 0 and np.array_equal(out3, value[0])
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"])
    check_scores(grad, st["score"], want, np.arange(11), f"{name} caps {caps}")
    assert np.all(grad[11:] == 0.0) and np.all(st["score"][:, 11:] == 0.0)
    for t in np.flatnonzero(ktot == 0):                             # sigma_i and nugget_i only
        q = int(t >= 150)
        assert all((st["score"][t, k] != 0.0) == (k in (q, 8 + q)) for k in range(13)), st["score"][t]
    tg = h.vecchia_grad_timings()
    assert tg["n_data"] == 300 and tg["n_pairs"] == np.sum((ktot + 1) * (ktot + 2) // 2)
    assert tg["select_ms"] > 0 and tg["solve_ms"] > 0 and tg["reduce_ms"] > 0 and tg["total_ms"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. full conditioning within the 64-data limit: the dense gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
def test_full_conditioning_is_the_dense_gradient(native, name):
    from sif_xco2_cokriging_amd import vecchia
    pb = small_problem(name)
    dense_np = dc.dense_ll_grad(pb["params"], pb["coords"], pb["values"], EUC)
    h2 = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h2.assemble_joint()
    info2, out3_dense, g_dense = h2.loglik(True)
    h2.close()
    assert info2 == 0
    d_dense = vgr.measure(g_dense, dense_np).max()
    assert d_dense < TOL
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    for ordering in ("random", "hilbert"):
        ranks = vecchia.ordering_ranks(pb["coords"], ordering, 1)
        ref, want = reference(pb, 2.0, (0, 0), ranks=ranks, key=ordering)
        assert ref["k_max"] == 64 and ref["n_empty"] == 1 and ref["info"] == 0
        out3, grad, info, st = h.loglik_vecchia_grad(ranks, 2.0, scores=True)
        assert info == 0 and st["k_max"] == 64
        check_scores(grad, st["score"], want, np.arange(11), f"{name} full conditioning, {ordering}")
        d_vecchia = vgr.measure(grad[:11], dense_np).max()
        between = (np.abs(grad[:11] - g_dense) / np.maximum(np.abs(dense_np), 1.0)).max()
        print(f"{name} {ordering}: vecchia - numpy {d_vecchia:.2e}, dense device - numpy {d_dense:.2e}, between {between:.2e}")
        assert d_vecchia < TOL
        assert between <= max(d_vecchia, d_dense)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. noise
# ---------------------------------------------------------------------------------------------------------------------
SCALES = (0.7, 1.3)


def test_noise_all_thirteen_slots(native):
    pb = problem("GEN")
    rng = np.random.default_rng(21)
    d = [rng.uniform(0.01, 0.05, 150) for _ in range(2)]
    ref, want = reference(pb, 0.5, (16, 16), noise_d=d, scales=SCALES, key="noise")
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    for k in range(2):
        h.set_noise(k, d[k], SCALES[k])
    h.set_local_neighbours(16, 16)
    value = h.loglik_vecchia(pb["ranks"], 0.5)
    out3, grad, info, st = h.loglik_vecchia_grad(pb["ranks"], 0.5, scores=True)
    assert info == ref["info"] == 0 and np.array_equal(out3, value[0])
    check_scores(grad, st["score"], want, np.arange(13), "noise, caps (16, 16)")
    assert np.all(grad[11:] != 0.0)
    h.close()


def test_noise_slots_under_full_conditioning(native):
    from sif_xco2_cokriging_amd import vecchia
    pb = small_problem("GEN")
    rng = np.random.default_rng(22)
    d = [rng.uniform(0.01, 0.05, 33), rng.uniform(0.01, 0.05, 32)]
    h2 = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    for k in range(2):
        h2.set_noise(k, d[k], SCALES[k])
        h.set_noise(k, d[k], SCALES[k])
    h2.assemble_joint()
    info2, _, g_dense = h2.loglik(True)
    gs_dense = h2.loglik_noise_grad()
    h2.close()
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 1)
    out3, grad, info, _ = h.loglik_vecchia_grad(ranks, 2.0)
    h.close()
    assert info == info2 == 0
    print("noise slots", grad[11:], gs_dense, "model slots measure", vgr.measure(grad[:11], g_dense).max())
    assert vgr.measure(grad[11:], gs_dense).max() < TOL
    assert vgr.measure(grad[:11], g_dense).max() < TOL


# ---------------------------------------------------------------------------------------------------------------------
# 4. one process, 5. haversine
# ---------------------------------------------------------------------------------------------------------------------
def test_univariate_model(native):
    pb = problem("GEN")
    uni = dict(coords=pb["coords"][:1], values=pb["values"][:1], params=[1.0, 1.2, 0.2, 0.02], metric=EUC,
               ranks=np.random.default_rng(12).permutation(150).astype(np.int64))
    _cache["uni"] = uni
    ref, want = reference(uni, 0.5, (8,))
    h = make_handle(native, uni["params"], EUC, uni["coords"], uni["values"])
    h.set_local_neighbours(8, 0)
    value = h.loglik_vecchia(uni["ranks"], 0.5)
    out3, grad, info, st = h.loglik_vecchia_grad(uni["ranks"], 0.5, scores=True)
    h.close()
    assert info == ref["info"] == 0 and np.array_equal(out3, value[0])
    check_scores(grad, st["score"], want, np.arange(4), "univariate")
    assert np.all(grad[:4] != 0.0) and np.all(grad[4:] == 0.0) and np.all(st["score"][:, 4:] == 0.0)


@pytest.mark.parametrize("name", ["GEN", "SET_A"])
def test_haversine(native, name):
    """the sites of tests/test_gpu_vecchia.py: test_haversine (n = 150 per process, 250 km, caps (12, 12)).  GEN's length scales
    of 0.2 are kilometres here -- every correlation beyond a co-located pair underflows, the gradient is that of nearly
    independent data; SET_A is the same nu with its own length scales of 460 km, where the sets matter."""
    from sif_xco2_cokriging_amd import synth
    rng = np.random.default_rng(4102)
    c0, c1 = synth.split_sites(np.column_stack([rng.uniform(30.0, 38.0, 225), rng.uniform(-105.0, -95.0, 225)]), 150)
    pb = dict(coords=[c0, c1], values=[rng.standard_normal(150), rng.standard_normal(150)], params=parameter_set(name), metric=HAV,
              ranks=np.random.default_rng(13).permutation(300).astype(np.int64))
    _cache["hav", name] = pb
    ref, want = reference(pb, 250.0, (12, 12))
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    h.set_local_neighbours(12, 12)
    value = h.loglik_vecchia(pb["ranks"], 250.0)
    out3, grad, info, st = h.loglik_vecchia_grad(pb["ranks"], 250.0, scores=True)
    h.close()
    assert info == ref["info"] == 0 and np.array_equal(out3, value[0]) and ref["n_capped"] > 0
    check_scores(grad, st["score"], want, np.arange(11), f"haversine {name}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. free13, 7. state and determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_slots_are_zero_and_live_slots_keep_their_bits(native):
    pb = problem("GEN")
    rng = np.random.default_rng(21)
    d = [rng.uniform(0.01, 0.05, 150) for _ in range(2)]
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    for k in range(2):
        h.set_noise(k, d[k], SCALES[k])
    h.set_local_neighbours(16, 16)
    full = h.loglik_vecchia_grad(pb["ranks"], 0.5, scores=True)
    free = np.ones(13, dtype=bool)
    free[[2, 3, 4, 12]] = False                                     # the three nu slots and one noise slot
    part = h.loglik_vecchia_grad(pb["ranks"], 0.5, free=free, scores=True)
    with pytest.raises(ValueError, match="13 flags"):
        h.loglik_vecchia_grad(pb["ranks"], 0.5, free=np.ones(11, dtype=bool))
    h.close()
    assert np.array_equal(part[0], full[0]) and part[2] == full[2] == 0
    assert np.all(part[1][~free] == 0.0) and np.all(part[3]["score"][:, ~free] == 0.0)
    assert np.array_equal(part[1][free], full[1][free]) and np.array_equal(part[3]["score"][:, free], full[3]["score"][:, free])
    assert np.all(full[1] != 0.0)


def test_repeated_calls_give_the_same_bits_and_leave_the_state(native):
    pb = problem("SET_B_UNIT")
    pc = np.random.default_rng(5).random((40, 2))
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.assemble_joint()
    assert h.factor() == 0
    before = h.predict(0, pc)
    h.set_local_neighbours(16, 16)
    value = h.loglik_vecchia(pb["ranks"], 0.5, terms=True)
    a = h.loglik_vecchia_grad(pb["ranks"], 0.5, scores=True)
    b = h.loglik_vecchia_grad(pb["ranks"], 0.5, scores=True)
    assert a[2] == b[2] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[3]["score"], b[3]["score"])
    after = h.predict(0, pc)                                         # no new assembly, no new factorisation
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    again = h.loglik_vecchia(pb["ranks"], 0.5, terms=True)
    assert np.array_equal(again[0], value[0]) and np.array_equal(again[0], a[0])
    for key in ("mean", "var", "count"):
        assert np.array_equal(again[2][key], value[2][key])
    h.close()


def test_value_and_gradient_report_the_same_select_statistics(native):
    """The lattice of tests/test_gpu_vecchia.py (576 + 144 sites: more than two 256-site chunks) on a handle that keeps 16
    candidates per process in LDS, caps (4, 4) at radius 1.0, so that the re-scan path runs.  The counts in timings() and stats3
    are those of the numpy reference over the passes of both processes, after the value and after the gradient alike; an uncapped
    prediction on the same handle then reports no select pass."""
    from sif_xco2_cokriging_amd import synth
    from tests.test_gpu_vecchia import lattice
    coords, values, ranks, D, proc = lattice()
    caps, max_dist, key_cap = (4, 4), 1.0, 16
    keep, _, capped = vr.conditioning_sets(D, proc, ranks, max_dist, caps)
    ktot = np.count_nonzero(keep, axis=1)
    cand = np.column_stack([np.count_nonzero((proc == q)[None, :] & (ranks[None, :] < ranks[:, None]) & (D <= max_dist), axis=1)
                            for q in range(2)])
    want = dict(local_n_capped=np.count_nonzero(capped), local_cand_max=cand.sum(axis=1).max(),
                local_n_rescan=np.count_nonzero(np.any(cand > max(key_cap, caps[0]), axis=1)))
    want_stats = dict(n_empty=np.count_nonzero(ktot == 0), k_max=ktot.max(), n_capped=np.count_nonzero(capped))
    assert np.array_equal(capped, np.any(cand > np.array(caps), axis=1)) and ktot.max() <= 64
    assert 0 < want["local_n_rescan"] < want["local_n_capped"] < len(ranks)   # every path of the pass is taken
    h = make_handle(native, synth.SET_B_UNIT, EUC, coords, values, local_select_cap=key_cap)
    h.set_local_neighbours(*caps)
    seen = {}
    for entry in ("value", "gradient"):
        out = h.loglik_vecchia(ranks, max_dist) if entry == "value" else h.loglik_vecchia_grad(ranks, max_dist)
        t = h.timings()
        print(f"{entry}: stats3 {out[-1]}, timings [60 ..] {[t[k] for k in ('local_select_ms', *want)]}")
        assert out[-2] == 0, entry
        assert t["local_select_ms"] > 0, entry
        seen[entry] = ({k: t[k] for k in want}, {k: out[-1][k] for k in want_stats})
        assert seen[entry] == (want, want_stats), entry
    assert seen["value"] == seen["gradient"]
    h.set_local_neighbours(0, 0)
    _, _, info = h.predict_local(0, coords[1][:40] + 0.05, 0.3)
    t = h.timings()
    assert info["k_max"] > 0 and t["local_ms"] > 0
    assert t["local_select_ms"] == 0 and t["local_n_capped"] == 0 and t["local_cand_max"] == 0 and t["local_n_rescan"] == 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals, 9. a datum without a term
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    pb = problem("SET_B_UNIT")
    ranks = pb["ranks"]
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.set_local_neighbours(0, 0)                                     # the uncapped 0.3 radius: sets up to 128
    ref = vr.vecchia_reference(pb["params"], pb["coords"], pb["values"], EUC, ranks, 0.3, (0, 0))
    ktot = ref["count"].sum(axis=1)
    n_over, k_max = int(np.count_nonzero(ktot > 64)), int(ktot.max())
    assert n_over > 0 and 64 < k_max <= 128
    with pytest.raises(native.NativeError, match=rf"{n_over} data have a conditioning set of more than 64 data \(the largest: {k_max}\)"):
        h.loglik_vecchia_grad(ranks, 0.3)
    h.set_local_neighbours(16, 16)
    assert h.loglik_vecchia_grad(ranks, 0.3)[2] == 0                 # the caps bring the same radius under the limit
    dup = ranks.copy()
    dup[200] = dup[17]
    with pytest.raises(native.NativeError, match=r"data 17 and 200 \(stacked order\) have the same rank " + str(int(ranks[17]))):
        h.loglik_vecchia_grad(dup, 0.5)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(native.NativeError, match="max_dist must be finite and >= 0"):
            h.loglik_vecchia_grad(ranks, bad)
    L = native.lib()
    out3, g13, inf = np.zeros(3), np.zeros(13), ctypes.c_int64(0)
    rp = ranks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    for args in ((None, native._p(out3), native._p(g13)), (rp, None, native._p(g13)), (rp, native._p(out3), None)):
        assert L.ck_loglik_vecchia_grad(h._h, args[0], 0.5, None, args[1], args[2], None, None, ctypes.byref(inf)) != 0
        assert "null rank_host / out3 / grad13" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia_grad(h._h, rp, 0.5, None, native._p(out3), native._p(g13), None, None, None) == 0
    h.set_trend(0, np.ones((150, 1)))
    with pytest.raises(native.NativeError, match="a trend of 1 columns is set on the handle"):
        h.loglik_vecchia_grad(ranks, 0.5)
    h.set_trend(0, None)
    with pytest.raises(ValueError, match="rank has 299 entries"):
        h.loglik_vecchia_grad(ranks[:-1], 0.5)
    h.close()
    hp = native.Handle(devices=[0, 0], rank=0)                       # a partitioned handle: the single-process form only
    hp.set_model(2, pb["params"][0:2], pb["params"][2:5], pb["params"][5:8], pb["params"][8:10], pb["params"][10])
    hp.set_metric(EUC)
    for k in range(2):
        hp.set_data(k, pb["coords"][k], pb["values"][k])
    with pytest.raises(native.NativeError, match=r"single-process form: this handle is partitioned \(world = 2\)"):
        hp.loglik_vecchia_grad(ranks, 0.5)
    hp.close()


def test_duplicate_sites_without_nugget_name_the_later_datum(native):
    """the case of tests/test_gpu_vecchia.py: datum 3 is conditioned on its copy alone and has the variance 0"""
    pb = problem("SET_B_UNIT")
    coords = [pb["coords"][0].copy(), pb["coords"][1]]
    coords[0][3] = coords[0][10] = (5.0, 5.0)
    params = list(pb["params"])
    params[8] = params[9] = 0.0
    ranks = pb["ranks"].copy()
    if ranks[3] < ranks[10]:
        ranks[[3, 10]] = ranks[[10, 3]]
    dup = dict(coords=coords, values=pb["values"], params=params, metric=EUC, ranks=ranks)
    _cache["dup"] = dup
    ref = vr.vecchia_reference(params, coords, pb["values"], EUC, ranks, 0.5, (16, 16))
    assert ref["info"] == 4 and ref["var"][3] == 0.0
    want = vgr.vecchia_grad_reference(params, coords, pb["values"], EUC, ref)
    h = make_handle(native, params, EUC, coords, pb["values"])
    h.set_local_neighbours(16, 16)
    out3, grad, info, st = h.loglik_vecchia_grad(ranks, 0.5, scores=True)
    h.close()
    assert info == 4 and np.all(np.isnan(out3)) and np.all(np.isnan(grad[:11])) and np.all(grad[11:] != grad[11:])
    assert np.all(np.isnan(st["score"][3, :11])) and np.all(st["score"][3, 11:] == 0.0)
    ok = np.arange(300) != 3
    es = vgr.measure(st["score"][ok][:, :11], want["score"][ok][:, :11])
    assert es.max() < TOL and np.all(st["score"][ok][:, 11:] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 10. the Python layer and the fit
# ---------------------------------------------------------------------------------------------------------------------
def _fields(coords, values):
    from sif_xco2_cokriging_amd import fields
    return fields.MultiField([fields.Field(coords[k], values[k]) for k in range(len(coords))])


def test_log_likelihood_with_gradient_equals_the_native_call(native):
    from sif_xco2_cokriging_amd import model, vecchia
    pb = problem("GEN")
    mf = _fields(pb["coords"], pb["values"])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(pb["params"])
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(150)
    v = vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4, gradient="analytic")
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 4)
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.set_local_neighbours(16, 12)
    out3, grad, info, _ = h.loglik_vecchia_grad(ranks, 0.5)
    got = mod.log_likelihood(mf, dist_units=None, fast_dist=False, vecchia=v, gradient=True)
    assert info == 0 and len(got) == 2 and got[0] == out3[0] and got[1].shape == (11,) and np.array_equal(got[1], grad[:11])
    assert mod.log_likelihood(mf, dist_units=None, fast_dist=False, vecchia=v) == out3[0]
    h.set_noise(0, d0, 2.0)
    out3, grad, info, _ = h.loglik_vecchia_grad(ranks, 0.5)
    got = mod.log_likelihood(mf, dist_units=None, fast_dist=False, vecchia=v, gradient=True, measurement_error=[d0, None],
                             noise_scale=(2.0, 1.0))
    assert len(got) == 3 and got[0] == out3[0] and np.array_equal(got[1], grad[:11]) and np.array_equal(got[2], grad[11:])
    assert got[2][0] != 0.0 and got[2][1] == 0.0
    h.close()
    with pytest.raises(native.NativeError, match=r"conditioning set of more than 64 data.*gradient=\"numeric\""):
        mod.log_likelihood(mf, dist_units=None, fast_dist=False, gradient=True,
                           vecchia=vecchia.Vecchia(0.3, ordering="random", seed=4, gradient="analytic"))


def test_fit_with_the_analytic_gradient(native, monkeypatch):
    """the simulated data of tests/test_gpu_vecchia.py's fit test, caps (16, 16), sigma_11, len_scale_11 and nugget_11 free, the
    same start both ways.  The analytic fit may not end below the numeric one by more than 100 x the numeric path's ftol
    (1e-10) x max(1, |l|), and makes fewer native likelihood calls."""
    from oracle import cokrige_oracle as orc
    from sif_xco2_cokriging_amd import model, vecchia
    calls = {"value": 0, "grad": 0}
    value_call, grad_call = native.Handle.loglik_vecchia, native.Handle.loglik_vecchia_grad

    def counted_value(self, *a, **k):
        calls["value"] += 1
        return value_call(self, *a, **k)

    def counted_grad(self, *a, **k):
        calls["grad"] += 1
        return grad_call(self, *a, **k)

    monkeypatch.setattr(native.Handle, "loglik_vecchia", counted_value)
    monkeypatch.setattr(native.Handle, "loglik_vecchia_grad", counted_grad)
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
    res = {}
    for how in ("numeric", "analytic"):
        calls["value"] = calls["grad"] = 0
        mod = model.MultivariateMatern(2)
        mod.params.set_values(start)
        names = list(mod.params.get_names())
        mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free],
                           vecchia=vecchia.Vecchia(1e5, max_neighbours=16, ordering="random", seed=2, gradient=how))
        r = mod.fit_result
        assert r.method == "Vecchia-ML" and r.n_free == 3 and r.free == free
        x = mod.params.get_values().astype(float)
        assert np.array_equal(np.delete(x, [0, 5, 8]), np.delete(np.array(start), [0, 5, 8]))
        res[how] = (r.loglik, calls["value"] + calls["grad"], dict(calls), r.n_eval, x[[0, 5, 8]])
        print(f"{how}: l {r.loglik:.9f}, native calls {res[how][2]}, n_eval {r.n_eval}, x {x[[0, 5, 8]]}, {r.message}")
    assert res["numeric"][2]["grad"] == 0 and res["analytic"][2]["value"] == 0
    assert res["analytic"][2]["grad"] == res["analytic"][3] + 1       # one native call per cost evaluation, one at the end
    assert res["analytic"][0] >= res["numeric"][0] - 100 * 1e-10 * max(1.0, abs(res["numeric"][0]))
    assert res["analytic"][1] < res["numeric"][1]
    assert np.all(np.isfinite(mod.fit_result.gradient)) and np.all(mod.fit_result.gradient[[1, 2, 3, 4, 6, 7, 9, 10]] == 0.0)
