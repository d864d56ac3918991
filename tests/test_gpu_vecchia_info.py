"""GPU tests of the expected information of the Vecchia likelihood: include/cokrige.h ck_loglik_vecchia_fisher,
native.Handle.loglik_vecchia_fisher, MultivariateMatern.information(vecchia=...) and
fit_likelihood(vecchia=Vecchia(..., information="expected"), std_errors=True).

The reference is the numpy loop of tests/vecchia_info_ref.py on the sets of tests/vecchia_ref.py: the set-difference form
sum_t [fisher_of(S_t) - fisher_of(c_t)] with differenced nu and length-scale derivatives, a different formula from the device's
last-row form with analytic derivatives; tests/test_vecchia_info_host.py ties it to the dense information and measures its floor.
The measure is dense_chains.class_errors(dense_chains.normalised(I, ref)): 1e-9 for the exact class, 1e-6 for the nu class,
max(1e-9, 10 x the fixture's floor) for the length-scale class (vecchia_info_ref.info_tol).  The fixtures are those of
tests/test_gpu_vecchia_grad.py: 2 x 150 half co-located sites on the unit square, the ranks default_rng(11).permutation(300),
SET_B_UNIT (closed-form nu) and GEN = SET_A with the length scales 0.2 (generic nu)."""
import ctypes

import numpy as np
import pytest

from tests import dense_chains as dc
from tests import vecchia_info_ref as vir
from tests import vecchia_ref as vr

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1


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


def handle_of(native, label, noise=True):
    f = vir.fixture(label)
    h = make_handle(native, f["params"], f["metric"], f["coords"], f["values"])
    if noise and f["noise_d"] is not None:
        for k in range(len(f["coords"])):
            h.set_noise(k, f["noise_d"][k], f["scales"][k])
    caps = tuple(f["caps"]) + (0,) * (2 - len(f["caps"]))
    h.set_local_neighbours(*caps)
    return h


def check_matrix(I, ref, label, npar=11, tol=None):
    e = dc.class_errors(dc.normalised(I, ref), npar)
    tol = vir.info_tol(label) if tol is None else tol
    print(f"{label}: exact {e['exact']:.2e} (bound {tol['exact']:.0e}), length scale {e['len']:.2e} (bound {tol['len']:.2e}), "
          f"nu {e['nu']:.2e} (bound {tol['nu']:.0e})")
    for cls in ("exact", "len", "nu"):
        assert e[cls] < tol[cls], (label, cls, e[cls], tol[cls])


def check_shape(I, live):
    """symmetric to the bit, exact zeros outside the live block, the unit-diagonal-scaled live block positive semi-definite"""
    live = np.asarray(live)
    dead = np.setdiff1d(np.arange(13), live)
    assert np.array_equal(I, I.T)
    assert np.all(I[dead] == 0.0) and np.all(I[:, dead] == 0.0)
    sub = I[np.ix_(live, live)]
    d = np.diag(sub)
    assert np.all(d > 0.0)
    s = 1.0 / np.sqrt(d)
    assert np.linalg.eigvalsh(sub * np.outer(s, s)).min() >= -1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 1. capped sets against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
@pytest.mark.parametrize("cap", [4, 16, 32])
def test_capped_information(native, name, cap):
    label = f"caps{cap}/{name}"
    f, ref = vir.fixture(label), vir.sets_of(label)
    ktot = ref["count"].sum(axis=1)
    assert ref["gap"].min() > 1e-9 and ref["n_empty"] == 3 and ref["info"] == 0   # the comparison leaves no datum out
    assert ref["k_max"] == {4: 8, 16: 32, 32: 64}[cap]
    h = handle_of(native, label)
    I, info, st = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    tg = h.vecchia_fisher_timings()
    h.close()
    assert info == 0
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"])
    check_matrix(I, vir.reference(label), label)
    check_shape(I, np.arange(11))
    assert tg["n_data"] == 300 and tg["n_entries"] == np.sum((ktot + 1) ** 2)
    assert tg["select_ms"] > 0 and tg["kernel_ms"] > 0 and tg["reduce_ms"] > 0 and tg["total_ms"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. full conditioning within the 64-data limit: the dense information
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SET_B_UNIT", "GEN"])
def test_full_conditioning_is_the_dense_information(native, name):
    f = vir.fixture(f"full_random/{name}")
    dense_np = dc.dense_fisher(f["params"], f["coords"], EUC)
    h2 = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    h2.assemble_joint()
    info2, I_dense = h2.fisher()
    h2.close()
    assert info2 == 0
    scale = np.sqrt(np.outer(np.diag(dense_np), np.diag(dense_np)))
    pos = scale > 0

    def distance(A, B):
        """max |A - B| in the scale of numpy's dense information"""
        return float(np.max(np.abs(A - B)[pos] / scale[pos]))

    d_dense = distance(I_dense, dense_np)
    for ordering in ("random", "hilbert"):
        label = f"full_{ordering}/{name}"
        fo, ref = vir.fixture(label), vir.sets_of(label)
        assert ref["k_max"] == 64 and ref["n_empty"] == 1 and ref["info"] == 0
        h = handle_of(native, label)
        I, info, st = h.loglik_vecchia_fisher(fo["ranks"], 2.0)
        h.close()
        assert info == 0 and st["k_max"] == 64 and st["n_empty"] == 1
        check_matrix(I, vir.reference(label), label)
        check_matrix(I, dense_np, f"{label} against numpy dense_fisher", tol=vir.info_tol(label))
        check_shape(I, np.arange(11))
        d_vecchia, between = distance(I, dense_np), distance(I, I_dense)
        print(f"{label}: vecchia - numpy {d_vecchia:.2e}, dense device - numpy {d_dense:.2e}, between {between:.2e}")
        assert between <= max(d_vecchia, d_dense)


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. noise
# ---------------------------------------------------------------------------------------------------------------------
def test_noise_all_thirteen_slots(native):
    label = "noise16/GEN"
    f, ref = vir.fixture(label), vir.sets_of(label)
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0
    h = handle_of(native, label)
    I, info, st = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    h.close()
    assert info == 0 and st["n_capped"] == ref["n_capped"]
    check_matrix(I, vir.reference(label), label)
    check_shape(I, np.arange(13))
    assert I[11, 11] > 0.0 and I[12, 12] > 0.0


def test_noise_slots_under_full_conditioning(native):
    label = "full_random/GEN"
    f = vir.fixture(label)
    rng = np.random.default_rng(22)
    d = [rng.uniform(0.01, 0.05, 33), rng.uniform(0.01, 0.05, 32)]
    h2 = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    h = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    for k in range(2):
        h2.set_noise(k, d[k], vir.SCALES[k])
        h.set_noise(k, d[k], vir.SCALES[k])
    h2.assemble_joint()
    info2, I_dense = h2.fisher()
    h2.close()
    I, info, _ = h.loglik_vecchia_fisher(f["ranks"], 2.0)
    h.close()
    assert info == info2 == 0
    # two device results with the same analytic derivatives: no differenced reference between them, the exact bound everywhere
    e = dc.normalised(I, I_dense)
    print("noise, full conditioning: vecchia against the dense device information, max", e.max(), "noise rows", e[11:].max())
    assert e.max() < 1e-9
    check_shape(I, np.arange(13))


# ---------------------------------------------------------------------------------------------------------------------
# 5. one process, 6. haversine
# ---------------------------------------------------------------------------------------------------------------------
def test_univariate_model(native):
    label = "uni8/GEN"
    f, ref = vir.fixture(label), vir.sets_of(label)
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0
    h = handle_of(native, label)
    I, info, st = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    h.close()
    assert info == 0 and st["k_max"] == ref["k_max"] == 8
    check_matrix(I, vir.reference(label), label, npar=4)
    check_shape(I, np.arange(4))


def test_haversine(native):
    label = "hav12/SET_A"
    f, ref = vir.fixture(label), vir.sets_of(label)
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0 and ref["n_capped"] > 0
    h = handle_of(native, label)
    I, info, st = h.loglik_vecchia_fisher(f["ranks"], 250.0)
    h.close()
    assert info == 0 and (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"])
    check_matrix(I, vir.reference(label), label)
    check_shape(I, np.arange(11))


# ---------------------------------------------------------------------------------------------------------------------
# 7. free13, 8. state and determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_slots_are_zero_and_live_slots_keep_their_bits(native):
    f = vir.fixture("noise16/GEN")
    h = handle_of(native, "noise16/GEN")
    full = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    free = np.ones(13, dtype=bool)
    free[[2, 3, 4, 12]] = False                                     # the three nu slots and one noise slot
    part = h.loglik_vecchia_fisher(f["ranks"], 0.5, free=free)
    with pytest.raises(ValueError, match="13 flags"):
        h.loglik_vecchia_fisher(f["ranks"], 0.5, free=np.ones(11, dtype=bool))
    h.close()
    assert part[1] == full[1] == 0
    assert np.all(part[0][~free] == 0.0) and np.all(part[0][:, ~free] == 0.0)
    assert np.array_equal(part[0][np.ix_(free, free)], full[0][np.ix_(free, free)])
    assert np.all(full[0] != 0.0)
    check_shape(part[0], np.flatnonzero(free))


def test_repeated_calls_give_the_same_bits_and_leave_the_state(native):
    f = vir.fixture("caps16/SET_B_UNIT")
    pc = np.random.default_rng(5).random((40, 2))
    h = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    h.assemble_joint()
    assert h.factor() == 0
    before = h.predict(0, pc)
    h.set_local_neighbours(16, 16)
    value = h.loglik_vecchia(f["ranks"], 0.5, terms=True)
    grad = h.loglik_vecchia_grad(f["ranks"], 0.5, scores=True)
    a = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    b = h.loglik_vecchia_fisher(f["ranks"], 0.5)
    assert a[1] == b[1] == 0 and np.array_equal(a[0], b[0]) and a[2] == b[2]
    after = h.predict(0, pc)                                         # no new assembly, no new factorisation
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    again = h.loglik_vecchia(f["ranks"], 0.5, terms=True)
    assert np.array_equal(again[0], value[0])
    for key in ("mean", "var", "count"):
        assert np.array_equal(again[2][key], value[2][key])
    grad2 = h.loglik_vecchia_grad(f["ranks"], 0.5, scores=True)
    assert np.array_equal(grad2[0], grad[0]) and np.array_equal(grad2[1], grad[1])
    assert np.array_equal(grad2[3]["score"], grad[3]["score"])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals, 10. a datum without a term
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    f = vir.fixture("caps16/SET_B_UNIT")
    ranks = f["ranks"]
    h = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    h.set_local_neighbours(0, 0)                                     # the uncapped 0.3 radius: sets up to 128
    ref = vr.vecchia_reference(f["params"], f["coords"], f["values"], EUC, ranks, 0.3, (0, 0))
    ktot = ref["count"].sum(axis=1)
    n_over, k_max = int(np.count_nonzero(ktot > 64)), int(ktot.max())
    assert n_over > 0 and 64 < k_max <= 128
    with pytest.raises(native.NativeError, match=rf"ck_loglik_vecchia_fisher: {n_over} data have a conditioning set of more than 64 "
                                                 rf"data \(the largest: {k_max}\)"):
        h.loglik_vecchia_fisher(ranks, 0.3)
    h.set_local_neighbours(16, 16)
    assert h.loglik_vecchia_fisher(ranks, 0.3)[1] == 0               # the caps bring the same radius under the limit
    dup = ranks.copy()
    dup[200] = dup[17]
    with pytest.raises(native.NativeError, match=r"data 17 and 200 \(stacked order\) have the same rank " + str(int(ranks[17]))):
        h.loglik_vecchia_fisher(dup, 0.5)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(native.NativeError, match="max_dist must be finite and >= 0"):
            h.loglik_vecchia_fisher(ranks, bad)
    L = native.lib()
    out, inf = np.zeros((13, 13)), ctypes.c_int64(0)
    rp = ranks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    for args in ((None, native._p(out)), (rp, None)):
        assert L.ck_loglik_vecchia_fisher(h._h, args[0], 0.5, None, args[1], None, ctypes.byref(inf)) != 0
        assert "null rank_host / fisher_host" in L.ck_last_error().decode()
    assert L.ck_loglik_vecchia_fisher(h._h, rp, 0.5, None, native._p(out), None, None) == 0
    h.set_trend(0, np.ones((150, 1)))
    with pytest.raises(native.NativeError, match="a trend of 1 columns is set on the handle"):
        h.loglik_vecchia_fisher(ranks, 0.5)
    h.set_trend(0, None)
    with pytest.raises(ValueError, match="rank has 299 entries"):
        h.loglik_vecchia_fisher(ranks[:-1], 0.5)
    h.close()
    hp = native.Handle(devices=[0, 0], rank=0)                       # a partitioned handle: the single-process form only
    hp.set_model(2, f["params"][0:2], f["params"][2:5], f["params"][5:8], f["params"][8:10], f["params"][10])
    hp.set_metric(EUC)
    for k in range(2):
        hp.set_data(k, f["coords"][k], f["values"][k])
    with pytest.raises(native.NativeError, match=r"single-process form: this handle is partitioned \(world = 2\)"):
        hp.loglik_vecchia_fisher(ranks, 0.5)
    hp.close()


def test_duplicate_sites_without_nugget_name_the_later_datum(native):
    """the case of tests/test_gpu_vecchia_grad.py: datum 3 is conditioned on its copy alone and has the variance 0"""
    f = vir.fixture("caps16/SET_B_UNIT")
    coords = [f["coords"][0].copy(), f["coords"][1]]
    coords[0][3] = coords[0][10] = (5.0, 5.0)
    params = list(f["params"])
    params[8] = params[9] = 0.0
    ranks = f["ranks"].copy()
    if ranks[3] < ranks[10]:
        ranks[[3, 10]] = ranks[[10, 3]]
    ref = vr.vecchia_reference(params, coords, f["values"], EUC, ranks, 0.5, (16, 16))
    assert ref["info"] == 4 and ref["var"][3] == 0.0
    h = make_handle(native, params, EUC, coords, f["values"])
    h.set_local_neighbours(16, 16)
    I, info, st = h.loglik_vecchia_fisher(ranks, 0.5)
    h.close()
    assert info == 4 and st["k_max"] == ref["k_max"]
    assert np.all(np.isnan(I[:11, :11])) and np.all(I[11:] == 0.0) and np.all(I[:, 11:] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 11. the Python layer, 12. the fit
# ---------------------------------------------------------------------------------------------------------------------
def _fields(coords, values):
    from sif_xco2_cokriging_amd import fields
    return fields.MultiField([fields.Field(coords[k], values[k]) for k in range(len(coords))])


def test_information_with_vecchia_equals_the_native_call(native):
    from sif_xco2_cokriging_amd import model, vecchia
    f = vir.fixture("caps16/GEN")
    mf = _fields(f["coords"], f["values"])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(f["params"])
    names = list(mod.params.get_names())
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(150)
    v = vecchia.Vecchia(0.5, max_neighbours=(16, 12), ordering="random", seed=4)   # information="none": an explicit call is consent
    ranks = vecchia.ordering_ranks(f["coords"], "random", 4)
    h = make_handle(native, f["params"], EUC, f["coords"], f["values"])
    h.set_local_neighbours(16, 12)
    I, info, _ = h.loglik_vecchia_fisher(ranks, 0.5)
    got = mod.information(mf, dist_units=None, fast_dist=False, vecchia=v)
    assert info == 0 and got.names == names and np.array_equal(got.fisher, I[:11, :11])
    assert got.std_error.shape == (11,) and np.all(np.isfinite(got.std_error)) and np.all(got.std_error > 0)
    assert got.conf_int().shape == (11, 2) and got.positive_definite
    h.set_noise(0, d0, 2.0)
    fixed = ["nu_11", "nu_12", "nu_22"]
    free = np.ones(13, dtype=bool)
    free[[2, 3, 4, 12]] = False                                     # the fixed nu slots; process 1 has no noise
    I, info, _ = h.loglik_vecchia_fisher(ranks, 0.5, free=free)
    got = mod.information(mf, dist_units=None, fast_dist=False, vecchia=v, measurement_error=[d0, None], noise_scale=(2.0, 1.0),
                          fixed=fixed)
    h.close()
    live = np.flatnonzero(free)
    assert info == 0 and got.names == [n for n in names if n not in fixed] + ["noise_scale_0"]
    assert np.array_equal(got.fisher, I[np.ix_(live, live)])
    assert got.std_error.shape == (9,) and np.all(got.std_error > 0) and got.conf_int().shape == (9, 2)
    assert got.estimates["noise_scale_0"] == 2.0
    with pytest.raises(native.NativeError, match=r"conditioning set of more than 64 data.*smaller max_neighbours"):
        mod.information(mf, dist_units=None, fast_dist=False, vecchia=vecchia.Vecchia(0.3, ordering="random", seed=4))


def test_fit_with_standard_errors(native):
    """the simulated data of tests/test_gpu_vecchia_grad.py's fit test: 400 data, cap 16, sigma_11, len_scale_11 and nugget_11
    free"""
    from oracle import cokrige_oracle as orc
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
    mod = model.MultivariateMatern(2)
    mod.params.set_values(start)
    names = list(mod.params.get_names())
    fixed = [n for n in names if n not in free]
    v = vecchia.Vecchia(1e5, max_neighbours=16, ordering="random", seed=2, gradient="analytic", information="expected")
    mod.fit_likelihood(mf, guess=mod.params, fixed=fixed, vecchia=v, std_errors=True)
    r = mod.fit_result
    assert r.method == "Vecchia-ML" and r.free == free and r.at_bound == []
    assert r.information is not None and r.information.names == free
    se = np.asarray(r.std_error)
    print("estimates", mod.params.get_values()[[0, 5, 8]], "standard errors", se)
    assert se.shape == (3,) and np.all(np.isfinite(se)) and np.all(se > 0)
    assert r.conf_int().shape == (3, 2)
    again = mod.information(mf, vecchia=v, fixed=fixed)              # re-evaluated at the optimum
    assert np.array_equal(r.information.fisher, again.fisher)
    mod2 = model.MultivariateMatern(2)
    mod2.params.set_values(start)
    mod2.fit_likelihood(mf, guess=mod2.params, fixed=fixed,
                        vecchia=vecchia.Vecchia(1e5, max_neighbours=16, ordering="random", seed=2, gradient="analytic"))
    assert mod2.fit_result.information is None and mod2.fit_result.std_error is None
