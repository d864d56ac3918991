"""GPU tests of the nearest-neighbour cap per process of the local predictor: include/cokrige.h ck_set_local_neighbours /
ck_debug_local_neighbours, native.Handle.set_local_neighbours / local_neighbours and
point_prediction.Predictor(max_neighbours=...).

A. the selection itself, bit for bit, on a lattice whose coordinates are multiples of 1/8 (squares and sums are exact, so the
   device distance equals numpy's to the bit, ties included);
B. predictions against oracle.local_predict given only the sites numpy selects for each point, on uniformly random sites
   (the test first asserts that every cut lies in a gap of the distances: relative gap > 1e-9, no point left out);
C. the universal form and measurement-error variances against the bordered / noisy system in numpy on the selected sites;
D. caps that do not bind give the bits of the uncapped call; the counters of ck_timings [60 ..];
E. the Python layer.
Tolerances are the local path's own (tests/test_gpu_local.py, tests/test_gpu_local_universal.py): rtol 1e-8, atol 1e-10 on pred
and on pred_err^2."""
import warnings

import numpy as np
import pytest

from oracle import cokrige_oracle as orc

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
        h.set_model(1, pv[0:1], pv[1:2], pv[2:3], pv[3:4])   # the univariate flat form: sigma, nu, len_scale, nugget
    h.set_metric(metric)
    for k in range(len(coords)):
        h.set_data(k, coords[k], values[k])
    return h


def select(D, max_dist, cap, withhold_zero):
    """the rule of include/cokrige.h for one process: D (m, n) distances -> (keep (m, n), rcut (m,), candidates (m,), gap (m,))
    gap: relative distance between the last kept and the first dropped candidate (inf where the cap does not bind)"""
    cand = D <= max_dist
    if withhold_zero:
        cand &= D > 0
    m = D.shape[0]
    rcut, gap = np.full(m, float(max_dist)), np.full(m, np.inf)
    for s in range(m):
        d = D[s, cand[s]]
        if cap > 0 and d.size > cap:
            rcut[s] = np.partition(d, cap - 1)[cap - 1]
            dropped = d[d > rcut[s]]
            if dropped.size:
                gap[s] = (dropped.min() - rcut[s]) / rcut[s] if rcut[s] > 0 else np.inf
    return cand & (D <= rcut[:, None]), rcut, cand.sum(axis=1), gap


# ---------------------------------------------------------------------------------------------------------------------
# A. selection, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def lattice():
    """process 0 on a 24 x 24 lattice of spacing 1/4, process 1 on its even nodes; about 40 points on multiples of 1/8"""
    if "lattice" not in _cache:
        g = np.arange(24) * 0.25
        X, Y = np.meshgrid(g, g, indexing="ij")
        c0 = np.column_stack([X.ravel(), Y.ravel()])
        c1 = np.column_stack([X[::2, ::2].ravel(), Y[::2, ::2].ravel()])
        rng = np.random.default_rng(7)
        nodes = rng.integers(0, 24, (12, 2)) * 0.25                              # a datum at d = 0
        centres = rng.integers(0, 23, (12, 2)) * 0.25 + 0.125                    # four equidistant sites
        mids = rng.integers(0, 23, (10, 2)) * 0.25 + np.array([0.125, 0.0])      # two
        off = np.array([[-0.125, 0.375], [2.875, 6.0], [1.375, 2.5], [0.0, 0.0], [5.75, 5.75], [9.0, 9.0], [3.125, 3.0]])
        pc = np.vstack([nodes, centres, mids, off])
        assert np.array_equal(pc * 8, np.round(pc * 8)) and np.array_equal(c0 * 8, np.round(c0 * 8))
        rngv = np.random.default_rng(8)
        values = [rngv.standard_normal(len(c0)), rngv.standard_normal(len(c1))]
        _cache["lattice"] = ([c0, c1], values, pc, [orc.distance_matrix(pc, c, EUC) for c in (c0, c1)])
    return _cache["lattice"]


@pytest.fixture(scope="module")
def lattice_handles(native):
    from sif_xco2_cokriging_amd import synth
    coords, values, _, _ = lattice()
    hs = {"default": make_handle(native, synth.SET_B_UNIT, EUC, coords, values),
          "rescan": make_handle(native, synth.SET_B_UNIT, EUC, coords, values, local_select_cap=16),
          "caller_order": make_handle(native, synth.SET_B_UNIT, EUC, coords, values, site_order=0)}
    yield hs
    for h in hs.values():
        h.close()


CAPS_A = [(1, 1), (2, 3), (4, 4), (5, 9), (64, 64), (1000, 1000)]


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("cv", [False, True])
@pytest.mark.parametrize("max_dist", [0.3, 1.0])
def test_selection_bit_for_bit(lattice_handles, max_dist, cv, i):
    _, _, pc, D = lattice()
    n_ties = n_rescan = 0
    for caps in CAPS_A:
        ref = [select(D[q], max_dist, caps[q], cv and q == i) for q in range(2)]
        ref_count = np.column_stack([r[0].sum(axis=1) for r in ref])
        ref_rcut = np.column_stack([r[1] for r in ref])
        ref_cand = ref[0][2] + ref[1][2]
        n_capped = int(np.count_nonzero((ref[0][2] > caps[0]) | (ref[1][2] > caps[1])))
        n_ties += int(np.count_nonzero(ref_count > np.array(caps)))
        for name, h in lattice_handles.items():
            h.set_local_neighbours(*caps)
            count, rcut = h.local_neighbours(i, pc, max_dist, cv)
            assert np.array_equal(rcut, ref_rcut), (name, caps)            # numpy's order statistic, or max_dist
            assert np.array_equal(count, ref_count), (name, caps)          # every candidate <= rcut: the ties too
            t = h.timings()
            assert t["local_n_capped"] == n_capped and t["local_cand_max"] == ref_cand.max(), (name, caps, t)
            assert t["local_select_ms"] > 0
            if name == "rescan":
                n_rescan += t["local_n_rescan"]
                over = ((ref[0][2] > max(caps[0], 16)) & (caps[0] > 0)) | ((ref[1][2] > max(caps[1], 16)) & (caps[1] > 0))
                assert t["local_n_rescan"] == np.count_nonzero(over), (caps, t)
            else:
                assert t["local_n_rescan"] == 0
    assert n_ties > 0                       # strictly more than the cap at the tie points
    assert n_rescan > 0 or max_dist < 1.0   # 16 keys per process: the 1.0 radius goes through the re-scan path


def test_selection_without_a_cap_returns_candidates(lattice_handles):
    _, _, pc, D = lattice()
    h = lattice_handles["default"]
    h.set_local_neighbours(0, 0)
    count, rcut = h.local_neighbours(0, pc, 1.0, True)
    assert np.array_equal(count[:, 0], np.count_nonzero((D[0] <= 1.0) & (D[0] > 0), axis=1))
    assert np.array_equal(count[:, 1], np.count_nonzero(D[1] <= 1.0, axis=1))
    assert np.all(rcut == 1.0) and h.timings()["local_n_capped"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# B. predictions against the oracle on the selected sites
# ---------------------------------------------------------------------------------------------------------------------
CAPS_GAP = [(1, 1), (8, 5), (12, 12), (40, 24), (40, 25), (64, 64), (150, 100)]


def random_problem(metric):
    """700 + 500 uniformly random sites, 300 candidate points (no lattice: symmetric sites tie up to rounding)"""
    if ("random", metric) not in _cache:
        from sif_xco2_cokriging_amd import synth
        rng = np.random.default_rng(4101)
        lo, hi = ((30.0, -105.0), (38.0, -95.0)) if metric == HAV else ((0.0, 0.0), (1.0, 1.0))
        coords = [np.column_stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n)]) for n in (700, 500)]
        pc = np.column_stack([rng.uniform(lo[0], hi[0], 300), rng.uniform(lo[1], hi[1], 300)])
        values = [rng.standard_normal(700), rng.standard_normal(500)]
        params = synth.conus_problem(8)["params"] if metric == HAV else synth.unit_square_problem(8, grid_side=2)["params"]
        _cache["random", metric] = dict(coords=coords, values=values, pc=pc, params=list(params), metric=metric,
                                        max_dist=250.0 if metric == HAV else 0.25)
    return _cache["random", metric]


def selection(pb, pc_key, pc, i, caps, cv):
    """numpy's neighbour sets of the points pc (cached), with the gap condition asserted for every point and process"""
    key = ("sel", pb["metric"], pc_key, i, caps, cv)
    if key not in _cache:
        out = []
        for q in range(len(caps)):
            D = _cache.setdefault(("D", pb["metric"], pc_key, q), orc.distance_matrix(pc, pb["coords"][q], pb["metric"]))
            keep, rcut, cand, gap = select(D, pb["max_dist"], caps[q], cv and q == i)
            assert gap.min() > 1e-9, (caps, q, gap.min())      # numpy and the device must agree on the set
            out.append((keep, rcut, cand))
        _cache[key] = out
    return _cache[key]


def oracle_on_selection(pb, pc, sel, i, params, pick):
    """oracle.local_predict per point, given only that point's selected sites and an infinite radius"""
    key = ("ref", id(sel), tuple(pick))
    if key not in _cache:
        n = len(sel)
        op = orc.Params.from_flat(params)
        pred, err = np.full(len(pick), np.nan), np.full(len(pick), np.nan)
        for a, s in enumerate(pick):
            coords = [pb["coords"][q][sel[q][0][s]] for q in range(n)]
            values = [pb["values"][q][sel[q][0][s]] for q in range(n)]
            pred[a], err[a] = (x[0] for x in orc.local_predict(op, coords, values, pc[s:s + 1], i, pb["metric"], np.inf)[:2])
        _cache[key] = (pred, err, sel)   # sel kept alive: its id is the key
    return _cache[key][:2]


def run_case(native, metric, caps, i=0, cv=False, tile_min=None, univariate=False, at_data=False):
    pb = random_problem(metric)
    params = pb["params"]
    if univariate:
        pb = dict(pb, coords=pb["coords"][:1], values=pb["values"][:1])
        params = [params[0], params[2], params[5], params[8]]
    pc_key, pc = ("data", i), pb["coords"][i][:300]
    if not at_data:
        pc_key, pc = "grid", pb["pc"]
    sel = selection(pb, pc_key, pc, i, caps, cv)
    pick = np.arange(0, 300, 5)                                           # 60 of the points
    ref_pred, ref_err = oracle_on_selection(pb, pc, sel, i, params, pick)
    h = make_handle(native, params, metric, pb["coords"], pb["values"], **({} if tile_min is None else {"local_tile_min": tile_min}))
    h.set_local_neighbours(*caps)
    pred, err, info = h.predict_local(i, pc[pick], max_dist=pb["max_dist"], cv=cv)
    k = sum(s[0].sum(axis=1) for s in sel)[pick]
    assert info["k_max"] == k.max() and info["n_empty"] == 0 and info["n_not_pd"] == 0, info
    np.testing.assert_allclose(pred, ref_pred, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err ** 2, ref_err ** 2, rtol=RTOL, atol=ATOL)
    capped = np.zeros(len(pick), bool)
    for q in range(len(sel)):
        capped |= (sel[q][2][pick] > caps[q]) & (caps[q] > 0)
    assert h.timings()["local_n_capped"] == np.count_nonzero(capped)
    h.close()
    return k


@pytest.mark.parametrize("metric", [HAV, EUC])
@pytest.mark.parametrize("caps", [(1, 1), (8, 5), (40, 24)])
def test_capped_predictions_in_the_lds_class(native, metric, caps):
    k = run_case(native, metric, caps)
    assert k.max() == sum(caps)   # random sites: no ties; (40, 24): exactly the LDS limit of 64
    if caps == (1, 1):
        assert k.min() == 2


@pytest.mark.parametrize("tile_min", [None, 0, 10 ** 6])
@pytest.mark.parametrize("metric,caps", [(HAV, (40, 25)), (HAV, (150, 100)), (EUC, (40, 25)), (EUC, (150, 100))])
def test_capped_predictions_beyond_the_lds_limit(native, metric, caps, tile_min):
    k = run_case(native, metric, caps, tile_min=tile_min)
    if caps == (40, 25):
        assert k.max() == 65      # the first system beyond the LDS limit
    else:
        assert k.max() > 128 and np.unique(k).size > 3   # capped and uncapped processes mixed


@pytest.mark.parametrize("caps", [(8, 5), (40, 25)])
def test_capped_cross_validation_at_data_sites(native, caps):
    k = run_case(native, HAV, caps, cv=True, at_data=True)
    assert k.max() == sum(caps)   # the withheld datum is no candidate: the cap is filled from the others


@pytest.mark.parametrize("caps", [(8, 5), (40, 25)])
def test_capped_target_process_1(native, caps):
    run_case(native, HAV, caps, i=1)
    run_case(native, EUC, caps, i=1, cv=True, at_data=True)


@pytest.mark.parametrize("caps", [(8,), (70,)])
def test_capped_univariate(native, caps):
    k = run_case(native, HAV, caps, univariate=True)
    assert k.max() == caps[0]


# ---------------------------------------------------------------------------------------------------------------------
# C. universal form and measurement-error variances
# ---------------------------------------------------------------------------------------------------------------------
def local_systems(pb, pc, sel, i, params, noise=None):
    """per point: (Sigma_loc [+ diag(s d)], c, z, n0) on the selected sites, in the library's order (process 0, then 1)"""
    op = orc.Params.from_flat(params)
    for s in range(len(pc)):
        ix = [np.flatnonzero(sel[q][0][s]) for q in range(2)]
        if min(len(x) for x in ix) == 0:
            yield None, None, None, len(ix[0])     # a process without neighbours: the callers settle these points by rule
            continue
        coords = [pb["coords"][q][ix[q]] for q in range(2)]
        S = orc.joint_cov(op, coords, pb["metric"])
        if noise is not None:
            S = S + np.diag(np.concatenate([noise[q][ix[q]] for q in range(2)]))
        c = orc.pred_cross_cov(op, coords, pc[s:s + 1], i, pb["metric"])
        z = np.concatenate([pb["values"][q][ix[q]] for q in range(2)])
        yield S, np.asarray(c).reshape(-1), z, len(ix[0])


def bordered_case():
    """(coords, values, pc, i, caps, max_dist, params, ref_pred, ref_var): ordinary cokriging, [[Sigma_loc, X], [X^T, 0]] in numpy
    on the selected neighbours; the last point has no site of process i (one of process 1): not estimable"""
    pb = random_problem(HAV)
    far = np.array([[45.0, -80.0]])                       # only process 1 has a site near here
    coords = [pb["coords"][0], np.vstack([pb["coords"][1], far + 0.2])]
    values = [pb["values"][0], np.append(pb["values"][1], 0.7)]
    pbx = dict(pb, coords=coords, values=values)
    i, caps, pick = 0, (12, 12), np.arange(0, 300, 10)
    pc = np.vstack([pb["pc"][pick], far])
    D = [orc.distance_matrix(pc, c, HAV) for c in coords]
    sel = [select(D[q], pb["max_dist"], caps[q], False) for q in range(2)]
    assert min(sel[0][3].min(), sel[1][3].min()) > 1e-9
    assert sel[0][0][-1].sum() == 0 and sel[1][0][-1].sum() == 1
    op = orc.Params.from_flat(pb["params"])
    c00 = op.sigma[i] ** 2 + op.nugget[i]
    ref_pred, ref_var = np.full(len(pc), np.nan), np.full(len(pc), np.nan)
    for s, (S, c, z, n0) in enumerate(local_systems(pbx, pc, sel, i, pb["params"])):
        if S is None:
            assert n0 == 0 and s == len(pc) - 1
            continue                                      # no site of process i for its regressor: rank deficient, NaN
        k = len(z)
        X = np.zeros((k, 2))
        X[:n0, 0], X[n0:, 1] = 1.0, 1.0
        K = np.block([[S, X], [X.T, np.zeros((2, 2))]])
        sol = np.linalg.solve(K, np.concatenate([c, [1.0, 0.0]]))
        w, lam = sol[:k], sol[k:]
        ref_pred[s], ref_var[s] = w @ z, c00 - w @ c - lam[0]
    return coords, values, pc, i, caps, pb["max_dist"], pb["params"], ref_pred, ref_var


def test_capped_ordinary_cokriging_against_the_bordered_system(native):
    """trend = "constant" with caps (12, 12) against the bordered system on the selected neighbours; one point whose
    neighbourhood has no site of process i for its regressor lands in n_rank_def"""
    coords, values, pc, i, caps, max_dist, params, ref_pred, ref_var = bordered_case()
    h = make_handle(native, params, HAV, coords, values)
    h.set_local_neighbours(*caps)
    for q in range(2):
        h.set_trend(q, np.ones((len(coords[q]), 1)))
    pred, err, info = h.predict_local_universal(i, pc, np.ones((len(pc), 1)), max_dist=max_dist)
    assert info["n_rank_def"] == 1 and np.isnan(pred[-1]) and np.isnan(err[-1])
    assert info["n_empty"] == 0 and info["n_not_pd"] == 0 and info["k_max"] == 24
    np.testing.assert_allclose(pred[:-1], ref_pred[:-1], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err[:-1] ** 2, ref_var[:-1], rtol=RTOL, atol=ATOL)
    assert h.timings()["local_n_capped"] == len(pc) - 1
    h.close()


def noisy_case():
    """(pb, d, scale, pc, i, caps, ref_pred, ref_var): Sigma_loc + diag(s d) on the selected neighbours"""
    pb = random_problem(HAV)
    rng = np.random.default_rng(5)
    d = [1e-2 * 10.0 ** rng.uniform(-1.0, 1.0, len(c)) for c in pb["coords"]]
    scale = (1.5, 0.7)
    i, caps, pick = 1, (12, 12), np.arange(0, 300, 10)
    pc = pb["pc"][pick]
    sel = [(s[0][pick], s[1][pick], s[2][pick]) for s in selection(pb, "grid", pb["pc"], i, caps, False)]
    op = orc.Params.from_flat(pb["params"])
    c00 = op.sigma[i] ** 2 + op.nugget[i]
    ref_pred, ref_var = np.zeros(len(pc)), np.zeros(len(pc))
    for s, (S, c, z, _) in enumerate(local_systems(pb, pc, sel, i, pb["params"], noise=[scale[q] * d[q] for q in range(2)])):
        w = np.linalg.solve(S, c)
        ref_pred[s], ref_var[s] = w @ z, c00 - w @ c
    return pb, d, scale, pc, i, caps, ref_pred, ref_var


def test_capped_prediction_with_measurement_error(native):
    """ck_set_noise with caps (12, 12) against the noisy local system in numpy"""
    pb, d, scale, pc, i, caps, ref_pred, ref_var = noisy_case()
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    for q in range(2):
        h.set_noise(q, d[q], scale[q])
    h.set_local_neighbours(*caps)
    pred, err, info = h.predict_local(i, pc, max_dist=pb["max_dist"])
    assert info["k_max"] == 24 and info["n_empty"] == 0 and info["n_not_pd"] == 0
    np.testing.assert_allclose(pred, ref_pred, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err ** 2, ref_var, rtol=RTOL, atol=ATOL)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("universal", [False, True])
def test_caps_that_do_not_bind_change_no_bit(native, universal):
    """(0, 0) and caps >= the data counts against a handle that never saw the call: array_equal outputs, equal info"""
    pb = random_problem(HAV)
    pc = pb["pc"][::3]

    def run(caps):
        h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
        if caps is not None:
            h.set_local_neighbours(*caps)
        if universal:
            for q in range(2):
                h.set_trend(q, np.ones((len(pb["coords"][q]), 1)))
            out = h.predict_local_universal(0, pc, np.ones((len(pc), 1)), max_dist=pb["max_dist"], want_beta=True)
            out[2]["beta"] = out[2]["beta"].tobytes()
        else:
            out = h.predict_local(0, pc, max_dist=pb["max_dist"])
        t = h.timings()
        h.close()
        return out, t

    (pred, err, info), t = run(None)
    assert info["k_max"] > 64 and t["local_select_ms"] == 0 and t["local_n_capped"] == 0
    for caps in ((0, 0), (700, 500), (10 ** 6, 10 ** 12), (0, 500)):
        (p2, e2, info2), t2 = run(caps)
        assert np.array_equal(pred, p2) and np.array_equal(err, e2) and info == info2, caps
        assert t2["local_n_capped"] == 0 and t2["local_n_rescan"] == 0
        assert (t2["local_select_ms"] > 0) == (caps != (0, 0))       # (0, 0): the select pass does not run at all
        assert t2["local_cand_max"] == (0 if caps == (0, 0) else info["k_max"])


def test_capped_call_is_repeatable_and_state_is_per_call(native):
    """the same bits on a repeated call; the cap acts on the next local call only and can be taken off again"""
    pb = random_problem(EUC)
    pc = pb["pc"][::4]
    h = make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    free = h.predict_local(0, pc, max_dist=pb["max_dist"])
    h.set_local_neighbours(40, 25)
    a = h.predict_local(0, pc, max_dist=pb["max_dist"])
    b = h.predict_local(0, pc, max_dist=pb["max_dist"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[2]["k_max"] == 65
    h.set_local_neighbours(0, 0)
    c = h.predict_local(0, pc, max_dist=pb["max_dist"])
    assert np.array_equal(free[0], c[0]) and np.array_equal(free[1], c[1]) and free[2] == c[2]
    with pytest.raises(native.NativeError, match="ck_set_local_neighbours"):
        h.set_local_neighbours(-1, 0)
    with pytest.raises(native.NativeError, match="ck_set_local_neighbours"):
        h.set_local_neighbours(3, -2)
    with pytest.raises(native.NativeError, match="local_select_cap"):
        h.set_option("local_select_cap", 10 ** 6)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_predictor_max_neighbours(native):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    pb = random_problem(HAV)
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(pb["params"]))
    mf = fields.MultiField([fields.Field(pb["coords"][k], pb["values"][k]) for k in range(2)])
    pc = pb["pc"][::6]
    h = make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    h.set_local_neighbours(8, 5)
    ref = h.predict_local(0, pc, max_dist=pb["max_dist"])
    ref_u = None
    for q in range(2):
        h.set_trend(q, np.ones((len(pb["coords"][q]), 1)))
    ref_u = h.predict_local_universal(0, pc, np.ones((len(pc), 1)), max_dist=pb["max_dist"])
    h.close()
    P = point_prediction.Predictor(mod, mf, max_neighbours=(8, 5))
    pred, err = P.predict_arrays(0, pc, max_dist=pb["max_dist"])
    assert np.array_equal(pred, ref[0]) and np.array_equal(err, ref[1])
    assert P.info["k_max"] == 13 and P.info["n_capped"] == len(pc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cv = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False)
    assert len(cv) == 700 and np.all(np.isfinite(cv["pred"])) and P.info["n_capped"] == 700 and P.info["k_max"] == 13
    P.close()
    Pu = point_prediction.Predictor(mod, mf, trend="constant", max_neighbours=(8, 5))
    pred, err = Pu.predict_arrays(0, pc, max_dist=pb["max_dist"])
    assert np.array_equal(pred, ref_u[0]) and np.array_equal(err, ref_u[1]) and Pu.info["n_capped"] == len(pc)
    Pu.close()
    P0 = point_prediction.Predictor(mod, mf)
    P0.predict_arrays(0, pc, max_dist=pb["max_dist"])
    assert P0.info["n_capped"] == 0 and P0.info["k_max"] > 64
    P0.close()
