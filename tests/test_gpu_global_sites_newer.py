"""GPU tests on whole-globe sites (tests/global_sites.py) of the local-solver entry points that came after
tests/test_gpu_global_sites.py: each reaches the haversine paths beyond the covariance tables (q >= 2, 10 007.5 km), the poles,
the antimeridian written both ways, lon -+ 360 copies and co-located data through a door the older calls do not have.

A. ck_predict_local_blocks: the table-or-exact decision per (member, neighbour) pair in the neighbourhood of the CENTRE, the
   tiled class's deferred list, sigma_BB over member pairs on opposite sides of the globe -- against the dense chain of
   tests/test_gpu_local_blocks.py on gs.globe_blocks, with noise, the singleton identity, and a centre written lon -+ 360;
B. ck_simulate_local: the internal copy of the data with the sites appended and its own tables over the whole sphere -- member
   lists, weights, means, variances and draws against tests/local_sim_ref.py;
C. ck_cv_local_folds: the lower cut d > buffer and the labels in the internal site order -- the selection against numpy
   (tests/test_gpu_local_cv_folds.py: withheld / select on the oracle's haversine distance), the predictions against a numpy chain
   on the selected sites alone (no second GPU handle), the special sites by name, the scores, the culling over 12 + 11 chunks;
D. ck_loglik_vecchia_fisher and ck_loglik_vecchia_trend / _trend_grad with set members beyond the table, against
   tests/vecchia_info_ref.py and tests/vecchia_trend_ref.py.

Data, parameters and handles are gs.GLOBE, gs.GLOBE_PARAMS["long"] (len_scale 2 000 km: an entry beyond the table is exp(-5) of
the variance) and make_handle of tests/test_gpu_global_sites.py.  No tolerance is new: rtol 1e-8 / atol 1e-10 on pred,
pred_err^2, beta, weights, mean and var (tests/test_gpu_local.py); draws at rtol 1e-8, atol 1e-8 sqrt(c0)
(tests/test_gpu_local_simulation.py); check_case / TOL_GRAD of tests/test_gpu_vecchia_trend.py; check_matrix of
tests/test_gpu_vecchia_info.py.  tests/test_global_sites_host.py pins without a GPU what the cases lean on: conditioning, gaps
at every cut, both size classes, the counts of pairs strictly outside the table, no reference block or site left out.  The only
data left out of a comparison are those whose neighbourhood the fold or the buffer empties: NaN in the reference, counted, and
the count asserted equal to the device's n_empty.

The numpy chain of section C takes the rows of the oracle's Sigma of GLOBE at the selected sites (orc.joint_cov, + diag(s d)
with ck_set_noise: the chain of tests/test_gpu_noise_local.py) and is tied, on every eighth datum, to orc.local_predict given
the selected sites only -- the construction of test_local_capped_neighbourhoods_on_the_globe.

Seen on an MI355X, every case passing.  Blocks: pred 1.4e-14, pred_err^2 4.0e-15, beta 3.6e-15 absolute over both reaches, kinds,
routes, site orders and the noise; k 24 .. 45 at 3 000 km (the LDS class), 380 .. 436 at 12 000 km (the tiled class); the singleton
blocks have the point calls' bits; the centre and its lon -+ 360 copy agree in every printed digit.  Simulation: weights 3.6e-14,
mean 2.4e-14, variance 4.9e-15, draws 2.5e-14; k_max 24 (caps) and 51 (3 000 km), 5 .. 9 levels, every member list identical.
Cross-validation: every count identical in both site orders; pred 2.2e-14 and pred_err^2 5.3e-15 against the chain (with noise
7.2e-15 / 1.2e-15; with a constant trend 1.0e-14 / 2.0e-15, beta 3.0e-15); k 0 .. 37 at 3 000 km with 28 neighbourhoods emptied by
their fold in each such call (NaN there and nowhere else), k = 65 for every datum under the caps, 268 .. 368 uncapped at 12 000
km; the scores 1.1e-15 relative.  Vecchia: information classes exact 2.3e-14, length scale 5.8e-12, nu 1.2e-10 (k_max 32, 572
capped sets); the trend's value 9.1e-13, beta 5.0e-16, gradient measure 2.2e-10, scores 3.8e-10, against central differences
9.5e-9; the p = 0 totals have ck_loglik_vecchia's bits.  The 82 cases of the module take 11 s together, the slowest 1.2 s."""
import time

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc
from tests import global_sites as gs
from tests import local_sim_ref as ls
from tests import test_gpu_local_blocks as tlb
from tests import test_gpu_local_cv_folds as tcv
from tests import test_gpu_local_universal as tlu
from tests import test_gpu_vecchia_info as tvi
from tests import test_gpu_vecchia_trend as tvt
from tests import vecchia_grad_ref as vgr
from tests import vecchia_info_ref as vir
from tests import vecchia_trend_ref as vtr
from tests.test_gpu_global_sites import local_sites, make_handle

pytestmark = pytest.mark.gpu

HAV = 0
RTOL, ATOL = 1e-8, 1e-10
PARAMS = gs.GLOBE_PARAMS["long"]
P = orc.Params.from_flat(PARAMS)
COORDS, VALUES = gs.GLOBE["coords"], gs.GLOBE["values"]
NOISE_SCALES = (1.5, 0.7)
OK, EMPTY, RANK_DEF = tlu.OK, tlu.EMPTY, tlu.RANK_DEF
_cache = {}
_seen = {}
_t0 = time.time()


def seen(key, value):
    _seen[key] = max(_seen.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    yield nat
    print("\nlargest deviations of tests/test_gpu_global_sites_newer.py:")
    for key in sorted(_seen):
        print(f"  {key}: {_seen[key]:.3g}")
    print(f"  wall time since import: {time.time() - _t0:.1f} s")


def data_noise():
    """variances as tests/test_gpu_local_lds_boundary.py draws them: two decades around 1e-2 sigma_k^2"""
    if "noise" not in _cache:
        rng = np.random.default_rng(43)
        _cache["noise"] = [1e-2 * P.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, len(COORDS[k])) for k in range(2)]
    return _cache["noise"]


def sigma(noise=False):
    """the oracle's Sigma of GLOBE, with s_k d on the diagonal"""
    key = ("S", noise)
    if key not in _cache:
        S = orc.joint_cov(P, COORDS, HAV)
        if noise:
            S = S + np.diag(np.concatenate([NOISE_SCALES[k] * data_noise()[k] for k in range(2)]))
        _cache[key] = S
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# A. block cokriging
# ---------------------------------------------------------------------------------------------------------------------
def block_case():
    if "blocks" not in _cache:
        _cache["blocks"] = gs.globe_blocks(np.random.default_rng(gs.BLOCK_SEED))
    return _cache["blocks"]


def block_trend(kind, lab, w, r):
    """(Fs, F0) of the constant trend: f0[b] = sum_a w_a"""
    if kind is None:
        return None, None
    return [np.ones((len(c), 1)) for c in COORDS], np.bincount(lab, weights=w, minlength=r)[:, None]


def block_chain(i, max_dist, kind, noise=False):
    """tests/test_gpu_local_blocks.py: block_reference on gs.globe_blocks, once per case"""
    key = ("block ref", i, max_dist, kind, noise)
    if key not in _cache:
        centres, pc, lab, w = block_case()
        Fs, F0 = block_trend(kind, lab, w, len(centres))
        d = [NOISE_SCALES[k] * data_noise()[k] for k in range(2)] if noise else None
        _cache[key] = tlb.block_reference(P, COORDS, VALUES, HAV, centres, pc, lab, w, i, max_dist, Fs, F0, noise=d)
    return _cache[key]


def run_blocks(native, i, max_dist, kind, tile_min, noise, label):
    centres, pc, lab, w = block_case()
    r = len(centres)
    Fs, F0 = block_trend(kind, lab, w, r)
    ref = block_chain(i, max_dist, kind, noise)
    assert np.all(ref["status"] == OK)                               # the chain leaves no block out
    opts = {} if tile_min is None else {"local_tile_min": tile_min}
    for site_order in (0, 1):
        h, _ = make_handle(native, PARAMS, COORDS, VALUES, noise=data_noise() if noise else None, scales=NOISE_SCALES,
                           site_order=site_order, **opts)
        tlb.set_trend(h, Fs)
        pred, err, info = h.predict_local_blocks(i, centres, pc, lab, w, f0=F0, max_dist=max_dist, want_beta=kind is not None)
        tm = h.local_blocks_timings()
        h.close()
        tlb.compare(pred, err, info, ref, beta=info["beta"] if kind is not None else None, label=f"{label} site_order {site_order}")
        print(f"{label} site_order {site_order}: per block |dpred| {np.abs(pred - ref['pred'])}, |dvar| {np.abs(err ** 2 - ref['var'])}")
        seen("A blocks |dpred|", np.max(np.abs(pred - ref["pred"])))
        seen("A blocks |dvar|", np.max(np.abs(err ** 2 - ref["var"])))
        if kind is not None:
            seen("A blocks |dbeta|", np.max(np.abs(info["beta"] - ref["beta"])))
        assert tm["cbar_evals"] == float(np.sum(np.bincount(lab, minlength=r) * ref["k"]))
        assert (tm["tiled_ms"] > 0.0) == (tile_min == 0 or ref["k"].max() > 64)
    return ref


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("tile_min", [None, 0])                     # the default classes | everything tiled
@pytest.mark.parametrize("kind", [None, "constant"])
@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_blocks_against_the_chain(native, max_dist, kind, tile_min, i):
    """Members up to 9 000 and 15 000 km from centres whose reach is 3 000 or 12 000 km: (member, neighbour) pairs beyond the
    table that the centre itself does not have; the cancelling weights of block 4; the hemisphere means of blocks 0 and 7."""
    ref = run_blocks(native, i, max_dist, kind, tile_min, False, f"blocks {max_dist:g} km {kind} tile_min {tile_min} i {i}")
    assert (ref["k"].max() <= 64) if max_dist == 3000.0 else (ref["k"].min() > 64)


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_blocks_with_noise(native, max_dist, i):
    run_blocks(native, i, max_dist, None, None, True, f"blocks with noise {max_dist:g} km i {i}")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("kind", [None, "constant"])
@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_singleton_blocks_are_the_point_call_on_the_globe(native, max_dist, kind, i):
    """the header's identity at the poles, either side of the antimeridian, on a datum and on its lon -+ 360 copy"""
    pc = local_sites()
    m = len(pc)
    h, _ = make_handle(native, PARAMS, COORDS, VALUES)
    F0 = None
    if kind is not None:
        tlb.set_trend(h, [np.ones((len(c), 1)) for c in COORDS])
        F0 = np.ones((m, 1))
        pp, pe, pinfo = h.predict_local_universal(i, pc, F0, max_dist=max_dist, want_beta=True)
    else:
        pp, pe, pinfo = h.predict_local(i, pc, max_dist=max_dist)
    bp, be, binfo = h.predict_local_blocks(i, pc, pc, np.arange(m), np.ones(m), f0=F0, max_dist=max_dist, want_beta=kind is not None)
    h.close()
    assert np.all(np.isfinite(pp)) and np.all(np.isfinite(pe))
    np.testing.assert_array_equal(bp, pp)
    np.testing.assert_array_equal(be, pe)
    for key in ("n_empty", "n_not_pd", "k_max"):
        assert binfo[key] == pinfo[key], key
    assert (pinfo["k_max"] <= 64) if max_dist == 3000.0 else (pinfo["k_max"] > 64)
    if kind is not None:
        assert binfo["n_rank_def"] == pinfo["n_rank_def"] == 0
        np.testing.assert_array_equal(binfo["beta"], pinfo["beta"])


@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_a_centre_and_its_periodic_copy_give_the_same_block(native, max_dist):
    """rows 4 and 5 of the centres -- a datum and its lon -+ 360 copy -- given the same members, once with block 4's cancelling
    weights and once with positive ones: equal neighbour counts, results within the tolerance of each other and of the chain
    (sin / cos of the two longitudes differ in the last bits, so no bit equality)"""
    centres, pc, lab, w = block_case()
    mem = np.flatnonzero(lab == gs.BLOCK_CANCELLING)
    q = len(mem)
    c4 = centres[[4, 5, 4, 5]]
    assert c4[0][0] == c4[1][0] and abs(c4[0][1] - c4[1][1]) == 360.0
    wpos = np.abs(w[mem]) / np.abs(w[mem]).sum()
    pc4, lab4, w4 = np.tile(pc[mem], (4, 1)), np.repeat(np.arange(4), q), np.concatenate([w[mem], w[mem], wpos, wpos])
    ref = tlb.block_reference(P, COORDS, VALUES, HAV, c4, pc4, lab4, w4, 0, max_dist)
    assert np.all(ref["status"] == OK) and ref["k"][0] == ref["k"][1]
    h, _ = make_handle(native, PARAMS, COORDS, VALUES)
    count, _ = h.local_neighbours(0, c4, max_dist)
    pred, err, info = h.predict_local_blocks(0, c4, pc4, lab4, w4, max_dist=max_dist)
    h.close()
    assert np.array_equal(count[0], count[1]) and count[0].sum() == ref["k"][0]
    tlb.compare(pred, err, info, ref, label=f"periodic centre {max_dist:g} km")
    print(f"periodic centre {max_dist:g} km: pred {pred}, pred_err^2 {err ** 2}")
    for a, b in ((0, 1), (2, 3)):
        np.testing.assert_allclose(pred[a], pred[b], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(err[a] ** 2, err[b] ** 2, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# B. conditional simulation
# ---------------------------------------------------------------------------------------------------------------------
def sim_case(i, which, on_data=False):
    """(pb, ref): the sites, ranks and tests/local_sim_ref.py's reference of one case, once.  on_data: every row of
    globe_pred_sites, the pole and the datum included, with SIM_DATA_NOISE on every datum"""
    key = ("sim", i, which, on_data)
    if key not in _cache:
        max_dist, caps = gs.SIM_CASES[which]
        rng = np.random.default_rng(gs.SIM_SITE_SEED)
        sites = gs.globe_pred_sites(rng, gs.SIM_M) if on_data else gs.sim_sites(rng, gs.SIM_M, i)
        ranks = np.random.default_rng(gs.SIM_RANK_SEED).permutation(len(sites)).astype(np.int64)
        noise = [np.full(len(c), gs.SIM_DATA_NOISE) for c in COORDS] if on_data else None
        ref = ls.local_sim_reference(PARAMS, COORDS, VALUES, HAV, i, sites, ranks, max_dist, caps, noise=noise)
        pb = dict(sites=sites, ranks=ranks, max_dist=max_dist, caps=caps, noise=noise, i=i,
                  c0=float(P.sigma[i] ** 2 + P.nugget[i]), label=f"sim i {i} {max_dist:g} km caps {caps} on_data {on_data}")
        _cache[key] = (pb, ref)
    return _cache[key]


def check_simulation(native, pb, ref, site_order=1):
    from tests.test_gpu_local_simulation import padded
    assert ref["info"] == 0 and ref["gap"] > 1e-9 and ref["n_empty"] == 0          # the reference leaves no site out
    i, sites, ranks, md = pb["i"], pb["sites"], pb["ranks"], pb["max_dist"]
    h, _ = make_handle(native, PARAMS, COORDS, VALUES, noise=pb["noise"], site_order=site_order)
    h.set_local_neighbours(*pb["caps"])
    idx, w = h.simulate_local_weights(i, sites, ranks, md)
    eps = np.random.default_rng(5).standard_normal((4, len(sites)))
    Y, info, st = h.simulate_local(i, sites, ranks, md, 4, noise=eps)
    h.close()
    assert np.array_equal(idx, padded(ref["members"], -1, np.int64)), pb["label"]           # the member lists, exactly
    wr = padded(ref["weights"], 0.0, np.float64)
    want = ref["draws"](eps)
    print(f"{pb['label']} site_order {site_order}: max |dw| {np.max(np.abs(w - wr)):.2e}, max |dmean| {np.max(np.abs(st['mean'] - ref['mean'])):.2e}, "
          f"max rel dvar {np.max(np.abs(st['var'] - ref['var']) / ref['var']):.2e}, max |dY| {np.max(np.abs(Y - want)):.2e}, k_max {st['k_max']}, "
          f"levels {st['n_levels']}")
    seen("B simulation |dw|", np.max(np.abs(w - wr)))
    seen("B simulation |dmean|", np.max(np.abs(st["mean"] - ref["mean"])))
    seen("B simulation |dvar|", np.max(np.abs(st["var"] - ref["var"])))
    seen("B simulation |dY|", np.max(np.abs(Y - want)))
    np.testing.assert_allclose(w, wr, rtol=RTOL, atol=ATOL)
    assert info == 0
    np.testing.assert_allclose(st["mean"], ref["mean"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"], ref["var"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(st["count"], ref["count"])
    assert (st["n_empty"], st["k_max"], st["n_capped"], st["n_levels"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"], ref["n_levels"])
    np.testing.assert_allclose(Y, want, rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("i", [0, 1])
def test_simulation_on_the_globe(native, i, which):
    """the sets mix data and earlier sites across the antimeridian; the internal tables span the whole sphere, and thousands of
    the candidates inside 12 000 km lie beyond them"""
    check_simulation(native, *sim_case(i, which))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("i", [0, 1])
def test_simulation_with_sites_on_noisy_data(native, i, which):
    """every row of globe_pred_sites: the pole that is a datum, the datum verbatim and its lon -+ 360 copy -- regular under
    measurement-error variances on the data"""
    check_simulation(native, *sim_case(i, which, on_data=True))


def test_simulation_in_the_callers_site_order(native):
    check_simulation(native, *sim_case(0, 0), site_order=0)


# ---------------------------------------------------------------------------------------------------------------------
# C. fold and buffer cross-validation
# ---------------------------------------------------------------------------------------------------------------------
def cv_distances(i):
    if ("cvD", i) not in _cache:
        _cache["cvD", i] = [orc.haversine_km(COORDS[i], COORDS[q]) for q in range(2)]
    return _cache["cvD", i]


def cv_labels(case):
    return [gs.lon_folds(c) for c in COORDS] if case[3] else [None, None]


def cv_selection(i, case):
    """numpy's selection for the data of process i: per process (keep (n_i, n_q), rcut, candidates, gap) of
    tests/test_gpu_local_cv_folds.py: withheld + select on the oracle's haversine distance"""
    key = ("cvsel", i, case)
    if key not in _cache:
        max_dist, caps, buf, _ = case
        D, fold = cv_distances(i), cv_labels(case)
        wb = (None, None) if buf is None else buf
        _cache[key] = [tcv.select(D[q], tcv.withheld(fold[i], fold[q], D[q], wb[q]), max_dist, caps[q]) for q in range(2)]
    return _cache[key]


def cv_handle(native, case, noise=False, trend=False, **options):
    h, _ = make_handle(native, PARAMS, COORDS, VALUES, noise=data_noise() if noise else None, scales=NOISE_SCALES, **options)
    h.set_local_neighbours(*case[1])
    if trend:
        tlb.set_trend(h, [np.ones((len(c), 1)) for c in COORDS])
    return h


def cv_call(case, i):
    """the arguments of cv_local_folds / local_cv_neighbours of a case"""
    fold = cv_labels(case)
    return dict(folds_i=fold[i], folds_other=fold[1 - i], n_folds=6 if case[3] else 0, buffer=case[2], max_dist=case[0])


def restricted(i, a, sel):
    """the selected sites of datum a of process i as a data set of their own, for a reference that takes a radius: a process
    without a selected site is given the antipode of the datum, which the radius 19 000 km leaves out and every selected site
    (at most 12 000 km away) is inside of"""
    x = COORDS[i][a]
    anti = np.array([[-x[0], x[1] - 180.0 if x[1] > 0 else x[1] + 180.0]])
    cs, vs, ix = [], [], []
    for q in range(2):
        s = np.flatnonzero(sel[q][0][a])
        ix.append(s)
        cs.append(COORDS[q][s] if s.size else anti)
        vs.append(VALUES[q][s] if s.size else np.zeros(1))
    return cs, vs, ix, 19000.0


def cv_chain(i, case, noise=False):
    """(pred, var, k, status) per datum of process i: Cholesky of the rows of the oracle's Sigma (+ diag(s d)) at the selected sites"""
    key = ("cvchain", i, case, noise)
    if key not in _cache:
        sel = cv_selection(i, case)
        S, z = sigma(noise), np.concatenate(VALUES)
        n_i, off = len(COORDS[i]), (0, gs.N0)
        pred, var = np.full(n_i, np.nan), np.full(n_i, np.nan)
        k, st = np.zeros(n_i, int), np.zeros(n_i, int)
        c00 = P.sigma[i] ** 2 + P.nugget[i]
        for a in range(n_i):
            idx = np.concatenate([off[q] + np.flatnonzero(sel[q][0][a]) for q in range(2)])
            k[a] = idx.size
            if idx.size == 0:
                st[a] = EMPTY
                continue
            assert off[i] + a not in idx                              # no datum predicts itself
            L = np.linalg.cholesky(S[np.ix_(idx, idx)])
            v, y = solve_triangular(L, S[idx, off[i] + a], lower=True), solve_triangular(L, z[idx], lower=True)
            pred[a], var[a] = v @ y, c00 - v @ v
        if not noise:       # the chain is orc.local_predict given the selected sites alone: tied to it on every eighth datum
            for a in range(0, n_i, 8):
                cs, vs, _, md = restricted(i, a, sel)
                op, oe = orc.local_predict(P, cs, vs, COORDS[i][a:a + 1], i, HAV, md)
                if st[a] == EMPTY:
                    assert np.isnan(op[0]) and np.isnan(oe[0])
                else:
                    np.testing.assert_allclose([op[0], oe[0] ** 2], [pred[a], max(var[a], 0.0)], rtol=1e-11, atol=1e-13)
        _cache[key] = (pred, var, k, st)
    return _cache[key]


def cv_compare(pred, err, info, ref, label, what):
    rp, rv, k, st = ref[:4]
    ok = st == OK
    dp = np.max(np.abs(pred[ok] - rp[ok]), initial=0.0)
    dv = np.max(np.abs(err[ok] ** 2 - np.maximum(rv[ok], 0.0)), initial=0.0)
    print(f"{label}: data {len(st)} finite {int(ok.sum())} emptied {int((st == EMPTY).sum())} k {int(k.min())}..{int(k.max())}, "
          f"max |dpred| {dp:.2e}, max |dvar| {dv:.2e}")
    seen(f"C {what} |dpred|", dp)
    seen(f"C {what} |dvar|", dv)
    seen("C emptied neighbourhoods in one call", int((st == EMPTY).sum()))
    assert np.array_equal(np.isnan(pred), ~ok) and np.array_equal(np.isnan(err), ~ok), label      # NaN in no other place
    assert info["n_empty"] == int((st == EMPTY).sum()) and info["n_not_pd"] == 0, label
    assert info["n_rank_def"] == int((st == RANK_DEF).sum()) and info["k_max"] == int(k.max()), label
    np.testing.assert_allclose(pred[ok], rp[ok], rtol=RTOL, atol=ATOL, err_msg=label)
    np.testing.assert_allclose(err[ok] ** 2, np.maximum(rv[ok], 0.0), rtol=RTOL, atol=ATOL, err_msg=label)


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("case", range(len(gs.CV_CASES)))
def test_cv_selection_against_numpy(native, case, i):
    case = gs.CV_CASES[case]
    sel = cv_selection(i, case)
    assert min(s[3].min() for s in sel) > 1e-9                        # every cut lies in a gap of the distances
    count = np.column_stack([s[0].sum(axis=1) for s in sel])
    rcut = np.column_stack([s[1] for s in sel])
    for site_order in (0, 1):
        h = cv_handle(native, case, site_order=site_order)
        got, gcut = h.local_cv_neighbours(i, **cv_call(case, i))
        h.close()
        assert np.array_equal(got, count), (site_order, np.flatnonzero((got != count).any(axis=1)))
        # the cut distance to the last bits only: the device's sin / cos are not libm's
        np.testing.assert_allclose(gcut, rcut, rtol=1e-12, atol=0)
    k = count.sum(axis=1)
    print(f"cv selection {case} i {i}: k {k.min()} .. {k.max()}, {np.count_nonzero(k == 65)} at 65, {np.count_nonzero(k == 0)} emptied")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("case", range(len(gs.CV_CASES)))
def test_cv_predictions_against_numpy(native, case, i):
    case = gs.CV_CASES[case]
    ref = cv_chain(i, case)
    for site_order in (0, 1):
        h = cv_handle(native, case, site_order=site_order)
        pred, err, info = h.cv_local_folds(i, **cv_call(case, i))
        h.close()
        cv_compare(pred, err, info, ref, f"cv {case} i {i} site_order {site_order}", "plain")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("case", [0, 2])                            # the LDS class with emptied neighbourhoods | k = 65
def test_cv_predictions_with_noise(native, case, i):
    case = gs.CV_CASES[case]
    ref, plain = cv_chain(i, case, noise=True), cv_chain(i, case)
    ok = ref[3] == OK
    assert np.max(np.abs(ref[0][ok] - plain[0][ok])) > 1e-3           # the noise moves the predictions: the case tests something
    h = cv_handle(native, case, noise=True)
    pred, err, info = h.cv_local_folds(i, **cv_call(case, i))
    h.close()
    cv_compare(pred, err, info, ref, f"cv with noise {case} i {i}", "noise")


def cv_trend_reference(i, case):
    """tests/test_gpu_local_universal.py: Reference given the selected sites only, a constant per process"""
    key = ("cvtrend", i, case)
    if key not in _cache:
        sel = cv_selection(i, case)
        n_i = len(COORDS[i])
        out = dict(pred=np.full(n_i, np.nan), var=np.full(n_i, np.nan), beta=np.full((n_i, 2), np.nan), status=np.zeros(n_i, int),
                   k=np.zeros(n_i, int))
        for a in range(n_i):
            cs, vs, ix, md = restricted(i, a, sel)
            r = tlu.Reference(P, cs, vs, HAV, [np.ones((len(c), 1)) for c in cs])(COORDS[i][a:a + 1], i, md, np.ones((1, 1)))
            assert r["k"][0] == ix[0].size + ix[1].size
            for name in ("pred", "var", "beta", "status", "k"):
                out[name][a] = r[name][0]
            if r["status"][0] == OK:                                  # the bordered Lagrange form agrees: the chain's own digits
                assert abs(r["pred"][0] - r["pred2"][0]) <= 0.1 * (RTOL * abs(r["pred"][0]) + ATOL)
                assert abs(r["var"][0] - r["var2"][0]) <= 0.1 * (RTOL * abs(r["var"][0]) + ATOL)
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("case", [0, 1])                            # the LDS class | the tiled class at k = 65
def test_cv_predictions_with_a_constant_trend(native, case, i):
    case = gs.CV_CASES[case]
    ref = cv_trend_reference(i, case)
    h = cv_handle(native, case, trend=True)
    pred, err, info = h.cv_local_folds(i, f0=np.ones((len(COORDS[i]), 1)), want_beta=True, **cv_call(case, i))
    h.close()
    st = ref["status"]
    cv_compare(pred, err, info, (ref["pred"], ref["var"], ref["k"], st), f"cv with a trend {case} i {i}", "trend")
    beta = info["beta"]
    assert np.array_equal(np.isnan(beta), np.isnan(ref["beta"]))
    fin = ~np.isnan(ref["beta"])
    seen("C trend |dbeta|", np.max(np.abs(beta[fin] - ref["beta"][fin])))
    np.testing.assert_allclose(beta[fin], ref["beta"][fin], rtol=RTOL, atol=ATOL)


def test_cv_special_sites_by_name(native):
    """what the buffer does at d = 0 across the processes, at the two spellings of (10, +-180) and around the pole"""
    c0 = COORDS[0]
    D = cv_distances(0)
    co = np.arange(100, 100 + gs.N_CO)                                # c1[50 + a] == c0[100 + a]
    assert np.all(D[1][co, 50 + np.arange(gs.N_CO)] == 0.0)
    assert tuple(c0[2]) == (10.0, 180.0) and tuple(c0[3]) == (10.0, -180.0) and 0.0 < D[0][2, 3] < 1e-9
    zero, wide = gs.CV_CASES[5], gs.CV_CASES[6]                       # buffer (0, 0) and (500, 500), no labels
    s0, s5 = cv_selection(0, zero), cv_selection(0, wide)
    h = cv_handle(native, zero)
    n0, _ = h.local_cv_neighbours(0, **cv_call(zero, 0))
    n5, _ = h.local_cv_neighbours(0, **cv_call(wide, 0))
    h.set_local_neighbours(0, 0)                                      # without a cap the counts show every withheld site
    both, _ = h.local_cv_neighbours(0, **cv_call(zero, 0))
    half, _ = h.local_cv_neighbours(0, **dict(cv_call(zero, 0), buffer=(0.0, None)))
    h.close()
    for got, sel in ((n0, s0), (n5, s5)):
        assert np.array_equal(got, np.column_stack([s[0].sum(axis=1) for s in sel]))
    # d = 0 across the processes: withheld under buffer (0, 0), a neighbour again once the other process's buffer is off
    assert not s0[1][0][co, 50 + np.arange(gs.N_CO)].any()
    at_zero = np.count_nonzero(D[1] == 0.0, axis=1)
    assert np.all(at_zero[co] == 1) and at_zero.sum() == gs.N_CO + 2
    assert np.array_equal(half[:, 1] - both[:, 1], at_zero) and np.array_equal(half[:, 0], both[:, 0])
    assert np.array_equal(both[:, 0], np.count_nonzero((D[0] > 0) & (D[0] <= zero[0]), axis=1))
    # the twin spelling at 1.5e-12 km is no duplicate: it stays under buffer 0 and is the nearest neighbour ...
    assert s0[0][0][2, 3] and s0[0][0][3, 2] and not s0[0][0][2, 2] and not s0[0][0][3, 3]
    # ... and both spellings go under buffer 500, with everything else within 500 km
    assert not s5[0][0][2, 3] and not s5[0][0][3, 2]
    for a in (2, 3):
        assert n5[a, 0] == np.count_nonzero(s5[0][0][a]) and not s5[0][0][a][D[0][a] <= 500.0].any()
    # the pole: everything within 500 km goes, at every longitude
    for q in range(2):
        gone = D[q][0] <= 500.0
        assert not s5[q][0][0][gone].any() and s5[q][1][0] > 500.0
    assert np.array_equal(n5[0], [np.count_nonzero(s5[q][0][0]) for q in range(2)])


def test_cv_scores_against_numpy(native):
    """fold_stats and score5 from the device's own pred / pred_err and the datum's noise term (test_scores_against_numpy)"""
    case = gs.CV_CASES[0]
    fold = cv_labels(case)
    h = cv_handle(native, case, noise=True)
    pred, err, info = h.cv_local_folds(0, **cv_call(case, 0))
    h.close()
    e, v = VALUES[0] - pred, err ** 2 + NOISE_SCALES[0] * data_noise()[0]
    ok = np.isfinite(pred) & (v > 0)
    assert info["n_empty"] == np.count_nonzero(~ok) > 0               # emptied neighbourhoods are skipped and not counted
    ref = np.zeros((6, 6))
    for f in range(6):
        s = ok & (fold[0] == f)
        ref[f] = [(fold[0] == f).sum() + (fold[1] == f).sum(), s.sum(), e[s].sum(), (e[s] ** 2).sum(), (e[s] ** 2 / v[s]).sum(), np.log(v[s]).sum()]
    fs = info["fold_stats"]
    dev = np.abs(fs[:, 2:] / ref[:, 2:] - 1).max()
    print(f"fold_stats relative deviations: {dev:.2e}")
    seen("C scores relative", dev)
    assert np.array_equal(fs[:, :2], ref[:, :2])
    np.testing.assert_allclose(fs[:, 2:], ref[:, 2:], rtol=1e-12)
    assert info["score5"][0] == ok.sum()
    np.testing.assert_allclose(info["score5"], ref[:, 1:].sum(axis=0), rtol=1e-12)


def test_cv_culling_with_many_chunks(native):
    """12 + 11 chunks of 256 sites, lon_folds labels, buffer (300, 300): the counts of the first 60 data of process 0 are
    numpy's from 1 500 km (most chunks skipped) to the `no culling` switch, in both site orders"""
    coords = gs.culling_sites()
    fold = [gs.lon_folds(c) for c in coords]
    D = [orc.haversine_km(coords[0][:60], c) for c in coords]
    W = [tcv.withheld(fold[0][:60], fold[q], D[q], gs.CV_CULL_BUFFER[q]) for q in range(2)]
    for md in gs.CV_CULL_REACHES + gs.CV_CULL_BUFFER:                 # no distance within rounding of a reach or of the buffer
        assert min(np.min(np.abs(d[d > 0] - md)) for d in D) > 1e-9 * md
    for site_order in (0, 1):
        h, _ = make_handle(native, PARAMS, coords, [np.zeros(len(c)) for c in coords], site_order=site_order)
        for md in gs.CV_CULL_REACHES:
            want = np.column_stack([tcv.select(D[q], W[q], md, 0)[0].sum(axis=1) for q in range(2)])
            count, _ = h.local_cv_neighbours(0, fold[0], fold[1], n_folds=6, buffer=gs.CV_CULL_BUFFER, max_dist=md)
            assert np.array_equal(count[:60], want), (site_order, md, np.flatnonzero((count[:60] != want).any(axis=1)))
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. Vecchia: the Fisher information and the GLS trend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,live", [("globe16/long", 11), ("globe16noise/long", 13)])
def test_vecchia_information_on_the_globe(native, label, live):
    f, ref = vir.fixture(label), vir.sets_of(label)
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0 and ref["k_max"] == 32 and ref["n_capped"] > 500
    h = tvi.handle_of(native, label)
    I, info, st = h.loglik_vecchia_fisher(f["ranks"], f["max_dist"])
    h.close()
    assert info == 0 and (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"])
    want = vir.reference(label)
    from tests import dense_chains as dc
    for cls, e in dc.class_errors(dc.normalised(I, want), 11).items():
        seen(f"D information class {cls}", e)
    tvi.check_matrix(I, want, label)
    tvi.check_shape(I, np.arange(live))


def trend_problem():
    """GLOBE with 0.3 added to the values and one constant per process"""
    if "trend pb" not in _cache:
        f = vir.fixture("globe16/long")
        _cache["trend pb"] = dict(coords=COORDS, values=[v + 0.3 for v in VALUES], params=list(PARAMS), metric=HAV, ranks=f["ranks"])
    pb = _cache["trend pb"]
    return pb, tvt.reference(pb, "constant", gs.VECCHIA_REACH, gs.VECCHIA_CAPS)


def test_vecchia_trend_on_the_globe(native):
    """profile and REML values, beta and its covariance, mu, v . v and g per datum (check_case), then the gradient against
    vecchia_grad_ref on the residual and against central differences of the numpy profile value on the fixed sets"""
    pb, ref = trend_problem()
    assert ref["k_max"] == 32 and ref["p"] == 2 and ref["n_capped"] > 500
    h = tvt.make_handle(native, pb["params"], HAV, pb["coords"], pb["values"], ref["F"])
    h.set_local_neighbours(*gs.VECCHIA_CAPS)
    value = tvt.check_case(h, pb, ref, gs.VECCHIA_REACH, "globe constant")
    out5, beta, cov, grad, info, st = h.loglik_vecchia_trend_grad(pb["ranks"], gs.VECCHIA_REACH, scores=True)
    h.close()
    seen("D trend |dl|", abs(value[0][0] - ref["out5"][0]))
    seen("D trend |dbeta|", np.linalg.norm(beta - ref["beta"]))
    assert info == 0 and np.array_equal(out5, value[0]) and np.array_equal(beta, value[1]) and np.array_equal(cov, value[2])
    want = tvt.grad_reference(pb, ref)
    eg = vgr.measure(grad[:11], want["grad13"][:11])
    es = vgr.measure(st["score"][:, :11], want["score"][:, :11])
    print(f"globe constant: gradient measure max {eg.max():.2e}, score measure max {es.max():.2e}")
    seen("D trend gradient measure", eg.max())
    seen("D trend score measure", es.max())
    assert eg.max() < tvt.TOL_GRAD and es.max() < tvt.TOL_GRAD, (grad, want["grad13"])
    assert np.all(grad[11:] == 0.0)
    x0 = np.array(pb["params"], dtype=float)
    for k in (0, 3, 6, 9, 10):
        e = 1e-5 * max(abs(x0[k]), 1.0)
        f = []
        for sgn in (1.0, -1.0):
            x = x0.copy()
            x[k] += sgn * e
            f.append(vtr.profile_value(x, pb["coords"], pb["values"], ref["X"], HAV, ref["keep"]))
        fd = (f[0] - f[1]) / (2 * e)
        seen("D trend gradient against central differences", vgr.measure(grad[k], fd))
        assert vgr.measure(grad[k], fd) < tvt.TOL_GRAD, (k, grad[k], fd)


def test_vecchia_trend_without_a_trend_is_the_plain_likelihood_on_the_globe(native):
    """p = 0: the totals of the trend call are ck_loglik_vecchia's, bit for bit, with sets beyond the table"""
    ranks = vir.fixture("globe16/long")["ranks"]
    h, _ = make_handle(native, PARAMS, COORDS, VALUES)
    h.set_local_neighbours(*gs.VECCHIA_CAPS)
    out3, info, st = h.loglik_vecchia(ranks, gs.VECCHIA_REACH, terms=True)
    assert info == 0 and st["k_max"] == 32
    for reml in (False, True):
        out5, beta, cov, info5, st5 = h.loglik_vecchia_trend(ranks, gs.VECCHIA_REACH, reml=reml, terms=True)
        assert info5 == 0 and beta.size == 0 and cov.size == 0
        assert np.array_equal(out5, [out3[0], out3[1], 0.0, out3[2], out3[2]])
        for key in ("mean", "var", "count"):
            assert np.array_equal(st5[key], st[key])
    h.close()
