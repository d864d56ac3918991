"""GPU tests of leave-group-out and buffer cross-validation in the moving neighbourhood: include/cokrige.h ck_cv_local_folds /
ck_debug_local_cv_neighbours, native.Handle.cv_local_folds / local_cv_neighbours and
point_prediction.Predictor.cross_validation(folds=..., also_withhold=..., buffer=...).

A. the selection, bit for bit, on the lattice of tests/test_gpu_local_nmax.py (coordinates on multiples of 1/8: the device distance
   equals numpy's to the bit, ties included): folds as strips and as 2 x 2 blocks, buffers, caps, the re-scan path, the caller's
   site order, a fold that withholds a whole chunk of 256 internal sites;
B. predictions against a handle that never saw the fold: the fold's data of both processes removed, the existing prediction
   calls at the withheld coordinates (rtol 1e-8, atol 1e-10 on pred and pred_err^2 as in that file -- the covariance tables of the
   two handles differ in the last digits); every cut asserted to lie in a gap of the distances;
C. identities, bit for bit: singleton folds and the zero buffer against ck_predict_local(cv = 1); ck_predict_local unchanged by
   a cross-validation call on the same handle;
D. full conditioning against the dense ck_cv_folds;
E. edges;  F. the scores against numpy;  G. refusals;  H. the Python layer.

Largest deviations seen on an MI355X: B. |d pred| 1.1e-13 and |d pred_err^2| 7.8e-16 (most folds: the same bits, the two handles'
tables being built over the same bounding box); F. the sums 6.7e-16 relative.  Every case takes well under a second."""
import warnings

import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import test_gpu_local_nmax as tln

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def withheld(fold_p, fold_s, D, wb):
    """(m, n) mask of the rule of include/cokrige.h for one process: fold_p the points' labels (None: none), fold_s the sites'"""
    w = np.zeros(D.shape, dtype=bool)
    if fold_p is not None and fold_s is not None:
        w |= (fold_s[None, :] >= 0) & (fold_s[None, :] == fold_p[:, None])
    if wb is not None and wb >= 0:
        w |= D <= wb
    return w


def select(D, w, max_dist, cap):
    """tln.select on the candidates that are left after withholding"""
    return tln.select(np.where(w, np.inf, D), max_dist, cap, False)


# ---------------------------------------------------------------------------------------------------------------------
# A. selection, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def lattice_cv():
    """the lattice's data as the points: D[i][q] = distances from the data of process i to the sites of process q; labels by
    strips of three lattice columns (8 folds) and by 2 x 2 blocks of nodes (144 folds), the same rule for both processes"""
    if "lat" not in _cache:
        coords, values, _, _ = tln.lattice()
        D = [[orc.distance_matrix(coords[i], coords[q], EUC) for q in range(2)] for i in range(2)]
        strips = [np.floor(c[:, 0] / 0.75).astype(np.int32) for c in coords]
        blocks = [(np.floor(c[:, 0] / 0.5) * 12 + np.floor(c[:, 1] / 0.5)).astype(np.int32) for c in coords]
        _cache["lat"] = (coords, values, D, {"strips": (strips, 8), "blocks": (blocks, 144)})
    return _cache["lat"]


@pytest.fixture(scope="module")
def lattice_handles(native):
    from sif_xco2_cokriging_amd import synth
    coords, values, _, _ = lattice_cv()
    hs = {"default": tln.make_handle(native, synth.SET_B_UNIT, EUC, coords, values),
          "rescan": tln.make_handle(native, synth.SET_B_UNIT, EUC, coords, values, local_select_cap=16),
          "caller_order": tln.make_handle(native, synth.SET_B_UNIT, EUC, coords, values, site_order=0)}
    yield hs
    for h in hs.values():
        h.close()


CAPS_A = [(1, 1), (4, 4), (5, 9), (0, 0)]


def check_selection(handles, i, fold, n_folds, buffer, max_dist):
    """ck_debug_local_cv_neighbours against numpy for every cap of CAPS_A on every handle -> (ties, re-scans, withheld pairs)"""
    _, _, D, _ = lattice_cv()
    wb = (None, None) if buffer is None else buffer
    fi, fo = (None, None) if fold is None else (fold[i], fold[1 - i])
    W = [withheld(None if fold is None else fold[i], None if fold is None else fold[q], D[i][q], wb[q]) for q in range(2)]
    n_ties = n_rescan = 0
    for caps in CAPS_A:
        ref = [select(D[i][q], W[q], max_dist, caps[q]) for q in range(2)]
        ref_count = np.column_stack([r[0].sum(axis=1) for r in ref])
        ref_rcut = np.column_stack([r[1] for r in ref])
        if caps != (0, 0):
            n_ties += int(np.count_nonzero(ref_count > np.array(caps)))
        for name, h in handles.items():
            h.set_local_neighbours(*caps)
            count, rcut = h.local_cv_neighbours(i, fi, fo, n_folds=n_folds, buffer=buffer, max_dist=max_dist)
            assert np.array_equal(rcut, ref_rcut), (name, caps)
            assert np.array_equal(count, ref_count), (name, caps)
            if name == "rescan":
                n_rescan += h.timings()["local_n_rescan"]
        for h in handles.values():
            h.set_local_neighbours(0, 0)
    return n_ties, n_rescan, int(W[0].sum() + W[1].sum())


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("kind", ["strips", "blocks"])
@pytest.mark.parametrize("buffer", [None, (0.0, 0.0), (0.25, 0.25), (0.5, None), (None, 0.5)])
@pytest.mark.parametrize("max_dist", [0.3, 1.0])
def test_selection_bit_for_bit(lattice_handles, max_dist, buffer, kind, i):
    fold, n_folds = lattice_cv()[3][kind]
    n_ties, n_rescan, n_withheld = check_selection(lattice_handles, i, fold, n_folds, buffer, max_dist)
    assert n_withheld > 0
    assert n_ties > 0 or max_dist < 1.0       # the lattice ties at every cut
    assert n_rescan > 0 or max_dist < 1.0     # 16 keys per process: the 1.0 radius goes through the re-scan path


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("buffer", [(0.0, None), (0.25, 0.0), (0.5, 0.5)])
def test_selection_with_a_buffer_alone(lattice_handles, buffer, i):
    if buffer[i] is None:
        buffer = buffer[::-1]
    check_selection(lattice_handles, i, None, 0, buffer, 1.0)


def test_selection_with_a_whole_chunk_withheld(lattice_handles):
    """the first 300 data of process 0 in one fold: with site_order = 0 they are the internal sites 0 .. 299, so all of the first
    chunk of 256 is withheld from each of them; labels -1 on part of process 1 (never withheld, no point)"""
    coords, _, D, _ = lattice_cv()
    fold = [np.where(np.arange(576) < 300, 0, 1).astype(np.int32), np.where(np.arange(144) < 70, 0, np.where(np.arange(144) < 100, 1, -1)).astype(np.int32)]
    check_selection(lattice_handles, 0, fold, 2, None, 1.0)
    check_selection(lattice_handles, 0, fold, 2, (0.25, None), 0.3)
    h = lattice_handles["caller_order"]
    count, rcut = h.local_cv_neighbours(1, fold[1], fold[0], n_folds=2, max_dist=1.0)
    assert np.all(count[100:] == 0) and np.all(np.isnan(rcut[100:]))        # never withheld: no row
    W = [withheld(fold[1], fold[q], D[1][q], None) for q in range(2)]
    ref = np.column_stack([select(D[1][q], W[q], 1.0, 0)[0].sum(axis=1) for q in range(2)])
    assert np.array_equal(count[:100], ref[:100]) and np.all(rcut[:100] == 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# B. against a handle that never saw the fold
# ---------------------------------------------------------------------------------------------------------------------
def fold_problem(metric, univariate=False):
    """tln.random_problem with labels: four folds over about half of the data of either process, the rest never withheld; d: raw
    measurement-error variances"""
    key = ("fold", metric, univariate)
    if key not in _cache:
        pb = tln.random_problem(metric)
        params = pb["params"]
        if univariate:
            pb = dict(pb, coords=pb["coords"][:1], values=pb["values"][:1])
            params = [params[0], params[2], params[5], params[8]]
        rng = np.random.default_rng(77 + metric)
        fold = [np.where(rng.random(len(c)) < 0.5, rng.integers(0, 4, len(c)), -1).astype(np.int32) for c in pb["coords"]]
        d = [1e-2 * 10.0 ** rng.uniform(-1.0, 1.0, len(c)) for c in pb["coords"]]
        _cache[key] = dict(pb, params=list(params), fold=fold, d=d)
    return _cache[key]


def assert_gaps(pb, i, caps, sel_points, fold_code):
    """numpy's selection of the points sel_points (data of process i in fold fold_code) has a relative gap > 1e-9 at every cut"""
    for q in range(len(pb["coords"])):
        D = orc.distance_matrix(pb["coords"][i][sel_points], pb["coords"][q], pb["metric"])
        W = withheld(np.full(len(sel_points), fold_code), pb["fold"][q], D, None)
        gap = select(D, W, pb["max_dist"], caps[q])[3]
        assert gap.min() > 1e-9, (caps, q, gap.min())


def run_fresh(native, metric, caps=None, i=0, trend=False, noise=False, tile_min=None, univariate=False, folds=(0, 1, 2)):
    pb = fold_problem(metric, univariate)
    nproc = len(pb["coords"])
    opts = {} if tile_min is None else {"local_tile_min": tile_min}
    scale = (1.5, 0.7)

    def handle(keep):
        h = tln.make_handle(native, pb["params"], metric, [pb["coords"][q][keep[q]] for q in range(nproc)],
                            [pb["values"][q][keep[q]] for q in range(nproc)], **opts)
        if caps is not None:
            h.set_local_neighbours(*caps)
        for q in range(nproc):
            if trend:
                h.set_trend(q, np.ones((int(np.count_nonzero(keep[q])), 1)))
            if noise:
                h.set_noise(q, pb["d"][q][keep[q]], scale[q])
        return h

    everything = [np.ones(len(c), bool) for c in pb["coords"]]
    h = handle(everything)
    fi, fo = pb["fold"][i], (pb["fold"][1 - i] if nproc == 2 else None)
    n_i = len(fi)
    pred, err, info = h.cv_local_folds(i, fi, fo, n_folds=4, f0=np.ones((n_i, 1)) if trend else None, max_dist=pb["max_dist"])
    h.close()
    assert np.array_equal(np.isnan(pred), fi < 0) and np.array_equal(np.isnan(err), fi < 0)
    assert info["n_empty"] == 0 and info["n_not_pd"] == 0 and info["n_rank_def"] == 0
    k_max = 0
    for f in folds:
        pts = np.flatnonzero(fi == f)
        if caps is not None:
            assert_gaps(pb, i, caps, pts, f)
        hf = handle([pb["fold"][q] != f for q in range(nproc)])
        pc = pb["coords"][i][pts]
        if trend:
            rp, re, rinfo = hf.predict_local_universal(i, pc, np.ones((len(pc), 1)), max_dist=pb["max_dist"])
        else:
            rp, re, rinfo = hf.predict_local(i, pc, max_dist=pb["max_dist"])
        hf.close()
        k_max = max(k_max, rinfo["k_max"])
        print(f"fold {f}: max |d pred| = {np.max(np.abs(pred[pts] - rp)):.3e}, max |d err^2| = {np.max(np.abs(err[pts] ** 2 - re ** 2)):.3e}")
        np.testing.assert_allclose(pred[pts], rp, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(err[pts] ** 2, re ** 2, rtol=RTOL, atol=ATOL)
    assert info["k_max"] >= k_max
    return info["k_max"]


@pytest.mark.parametrize("metric,caps,i", [(HAV, None, 0), (EUC, None, 1), (HAV, (8, 5), 1), (EUC, (8, 5), 0), (HAV, (40, 24), 0),
                                           (EUC, (40, 24), 1)])
def test_against_a_handle_without_the_fold(native, metric, caps, i):
    k = run_fresh(native, metric, caps=caps, i=i)
    if caps is not None:
        assert k == sum(caps)
    else:
        assert k > 64


@pytest.mark.parametrize("metric,caps,i", [(HAV, (8, 5), 0), (EUC, None, 1)])
def test_against_a_handle_without_the_fold_constant_trend(native, metric, caps, i):
    run_fresh(native, metric, caps=caps, i=i, trend=True, folds=(0, 3))


@pytest.mark.parametrize("metric,caps,i", [(HAV, (40, 24), 1), (EUC, None, 0)])
def test_against_a_handle_without_the_fold_noise(native, metric, caps, i):
    run_fresh(native, metric, caps=caps, i=i, noise=True, folds=(1, 2))


@pytest.mark.parametrize("tile_min", [16, 10 ** 6])
def test_against_a_handle_without_the_fold_size_classes(native, tile_min):
    """local_tile_min = 16: everything beyond 16 neighbours on the tiled path; 10^6: everything beyond 64 on the slab kernel"""
    assert run_fresh(native, HAV, i=0, tile_min=tile_min, folds=(0, 2)) > 64
    assert run_fresh(native, EUC, caps=(40, 25), i=1, tile_min=tile_min, folds=(3,)) == 65


@pytest.mark.parametrize("caps", [None, (8,)])
def test_against_a_handle_without_the_fold_univariate(native, caps):
    run_fresh(native, HAV, caps=caps, univariate=True, folds=(0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# C. identities, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [None, (8, 5), (40, 25)])
@pytest.mark.parametrize("i", [0, 1])
def test_singleton_folds_are_the_cv_flag(native, caps, i):
    """duplicate-free data: the only site with a datum's own label is the datum, the only site at distance 0 too"""
    pb = tln.random_problem(HAV)
    h = tln.make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    if caps is not None:
        h.set_local_neighbours(*caps)
    n_i = len(pb["coords"][i])
    before = h.predict_local(0, pb["pc"][:50], max_dist=pb["max_dist"])
    ref = h.predict_local(i, pb["coords"][i], max_dist=pb["max_dist"], cv=True)
    pred, err, info = h.cv_local_folds(i, np.arange(n_i), None, max_dist=pb["max_dist"])
    assert np.array_equal(pred, ref[0]) and np.array_equal(err, ref[1]) and not np.isnan(pred).any()
    assert info["k_max"] == ref[2]["k_max"] and info["n_empty"] == ref[2]["n_empty"] == 0 and info["n_not_pd"] == 0
    assert np.array_equal(info["fold_stats"][:, :2], np.ones((n_i, 2)))
    # and the cross-validation call left the handle as it was: the same bits at fixed points
    after = h.predict_local(0, pb["pc"][:50], max_dist=pb["max_dist"])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    h.close()


@pytest.mark.parametrize("caps", [None, (8, 5)])
def test_zero_buffer_is_the_cv_flag_on_coincident_sites(native, caps):
    """data with coincident sites: buffer (0, off) without labels withholds what cv = 1 withholds, copies included.  Two data of a
    process at one place share the nugget (their rows of Sigma are equal), so measurement-error variances keep the systems of
    their neighbours positive definite"""
    pb = tln.random_problem(EUC)
    coords = [np.vstack([pb["coords"][0], pb["coords"][0][:40], pb["coords"][1][:10]]), pb["coords"][1]]
    values = [np.concatenate([pb["values"][0], pb["values"][0][:40] + 0.1, np.zeros(10)]), pb["values"][1]]
    h = tln.make_handle(native, pb["params"], EUC, coords, values)
    h.set_noise(0, np.full(len(coords[0]), 0.01), 1.0)
    if caps is not None:
        h.set_local_neighbours(*caps)
    ref = h.predict_local(0, coords[0], max_dist=pb["max_dist"], cv=True)
    pred, err, info = h.cv_local_folds(0, buffer=(0.0, None), max_dist=pb["max_dist"])
    assert ref[2]["n_not_pd"] == 0 and info["n_not_pd"] == 0
    assert np.array_equal(pred, ref[0]) and np.array_equal(err, ref[1]) and not np.isnan(pred).any()
    assert info["k_max"] == ref[2]["k_max"] and info["fold_stats"].shape == (0, 6) and info["score5"][0] == len(pred)
    # singleton folds do NOT: the coincident copy stays a neighbour
    p2, _, _ = h.cv_local_folds(0, np.arange(len(coords[0])), None, max_dist=pb["max_dist"])
    assert not np.array_equal(p2[:40], pred[:40]) and np.array_equal(p2[100:700], pred[100:700])
    h.close()


def test_dense_calls_are_unchanged_by_a_cross_validation_call(native):
    """a resident factor survives: ck_predict gives the same bits before and after"""
    pb = tln.random_problem(EUC)
    h = tln.make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    h.assemble_joint()
    assert h.factor() == 0
    before = h.predict(0, pb["pc"][:40])
    h.cv_local_folds(0, np.arange(700) % 7, np.arange(500) % 7, max_dist=pb["max_dist"])
    after = h.predict(0, pb["pc"][:40])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. full conditioning against the dense call
# ---------------------------------------------------------------------------------------------------------------------
def dense_case():
    if "dense" not in _cache:
        rng = np.random.default_rng(31)
        params = [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.02, 0.025, -0.19]
        p = orc.Params.from_flat(params)
        pts = np.column_stack([rng.uniform(0, 10, 225), rng.uniform(0, 10, 225)])
        coords = [pts[:150].copy(), pts[75:].copy()]               # process 1 datum a sits on process 0 datum 75 + a for a < 75
        S = orc.joint_cov(p, coords, EUC)
        z = np.linalg.cholesky(S) @ rng.standard_normal(300)
        d = [1e-2 * 10.0 ** rng.uniform(-1.0, 1.0, 150) for _ in range(2)]
        _cache["dense"] = (params, coords, [z[:150].copy(), z[150:].copy()], d)
    return _cache["dense"]


@pytest.mark.parametrize("i", [0, 1])
def test_full_conditioning_equals_the_dense_folds(native, i):
    params, coords, values, d = dense_case()
    scale = (1.3, 0.6)
    rng = np.random.default_rng(5 + i)
    sizes = [1, 2, 17, 64, 30]
    fi = np.repeat(np.arange(6), sizes + [150 - sum(sizes)])[rng.permutation(150)].astype(np.int32)
    fi[fi == 5] = -1
    fo = np.full(150, -1, dtype=np.int32)
    if i == 0:
        fo[:75] = fi[75:]             # the co-located partner leaves with the fold
    else:
        fo[75:] = fi[:75]
    h = tln.make_handle(native, params, EUC, coords, values)
    for q in range(2):
        h.set_noise(q, d[q], scale[q])
    h.assemble_joint()
    assert h.factor() == 0
    info, dp, de = h.cv_folds(i, fi, fo, n_folds=5)
    assert info == 0
    pred, err, linfo = h.cv_local_folds(i, fi, fo, n_folds=5, max_dist=100.0)
    sel = fi >= 0
    assert np.array_equal(np.isnan(pred), ~sel) and linfo["k_max"] >= 300 - 64 - 64
    own = scale[i] * d[i]
    np.testing.assert_allclose(pred[sel], dp[sel], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err[sel] ** 2 + own[sel], de[sel] ** 2, rtol=RTOL, atol=ATOL)
    # singleton folds: the marginal density of a single datum is its joint density
    single = np.arange(150, dtype=np.int32)
    info, _, _, stats = h.cv_folds(i, single, None, n_folds=150, want_stats=True)
    assert info == 0
    dense_nlpd = 0.5 * (stats[:, 0] * np.log(2.0 * np.pi) - stats[:, 1] + stats[:, 2])
    _, _, linfo = h.cv_local_folds(i, single, None, max_dist=100.0)
    fs = linfo["fold_stats"]
    local_nlpd = 0.5 * (fs[:, 1] * np.log(2.0 * np.pi) + fs[:, 5] + fs[:, 4])
    np.testing.assert_allclose(local_nlpd.sum(), dense_nlpd.sum(), rtol=RTOL)
    np.testing.assert_allclose(local_nlpd, dense_nlpd, rtol=1e-7, atol=1e-9)
    s5 = linfo["score5"]
    np.testing.assert_allclose(0.5 * (s5[0] * np.log(2.0 * np.pi) + s5[4] + s5[3]), dense_nlpd.sum(), rtol=RTOL)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_i", [1, 65])
def test_edge_sizes(native, n_i):
    pb = tln.random_problem(HAV)
    coords, values = [pb["coords"][0][:n_i], pb["coords"][1][:130]], [pb["values"][0][:n_i], pb["values"][1][:130]]
    h = tln.make_handle(native, pb["params"], HAV, coords, values)
    ref = h.predict_local(0, coords[0], max_dist=600.0, cv=True)
    pred, err, info = h.cv_local_folds(0, np.arange(n_i), None, max_dist=600.0)
    assert np.array_equal(pred, ref[0]) and np.array_equal(err, ref[1]) and np.isfinite(pred).all() and info["k_max"] == ref[2]["k_max"]
    count, _ = h.local_cv_neighbours(0, np.zeros(n_i, np.int32), None, max_dist=1e5)
    assert np.all(count[:, 0] == 0) and np.all(count[:, 1] == 130)
    h.close()


def test_one_fold_of_everything_empties_every_neighbourhood(native):
    pb = tln.random_problem(EUC)
    h = tln.make_handle(native, pb["params"], EUC, pb["coords"], pb["values"])
    pred, err, info = h.cv_local_folds(0, np.zeros(700, np.int32), np.zeros(500, np.int32), max_dist=pb["max_dist"])
    assert np.isnan(pred).all() and np.isnan(err).all()
    assert info["n_empty"] == 700 and info["n_not_pd"] == 0 and info["k_max"] == 0
    assert info["fold_stats"].tolist() == [[1200.0, 0.0, 0.0, 0.0, 0.0, 0.0]] and np.all(info["score5"] == 0)
    h.close()


def test_unlabelled_data_are_not_predicted_but_remain_neighbours(native):
    pb = fold_problem(HAV)
    fi, fo = pb["fold"]
    h = tln.make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    pred, err, info = h.cv_local_folds(0, fi, fo, n_folds=4, max_dist=pb["max_dist"])
    h.close()
    assert np.array_equal(np.isnan(pred), fi < 0) and (fi < 0).sum() > 100
    keep = [fi >= 0, fo >= 0]                                  # the same call on the labelled data alone
    h = tln.make_handle(native, pb["params"], HAV, [pb["coords"][q][keep[q]] for q in range(2)], [pb["values"][q][keep[q]] for q in range(2)])
    p2, _, info2 = h.cv_local_folds(0, fi[keep[0]], fo[keep[1]], n_folds=4, max_dist=pb["max_dist"])
    h.close()
    assert info2["k_max"] < info["k_max"]
    assert np.median(np.abs(p2 - pred[keep[0]])) > 1e-4         # they were neighbours: without them the predictions move


def test_a_trend_the_remaining_neighbours_cannot_carry(native):
    """fold 0 = all of process 0, nothing of process 1: every neighbourhood is left without a site of process 0 for its regressor"""
    pb = tln.random_problem(HAV)
    h = tln.make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    for q in range(2):
        h.set_trend(q, np.ones((len(pb["coords"][q]), 1)))
    pred, err, info = h.cv_local_folds(0, np.zeros(700, np.int32), None, f0=np.ones((700, 1)), max_dist=pb["max_dist"], want_beta=True)
    assert info["n_rank_def"] == 700 and info["n_empty"] == 0 and np.isnan(pred).all() and np.isnan(info["beta"]).all()
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# F. scores
# ---------------------------------------------------------------------------------------------------------------------
def test_scores_against_numpy(native):
    """fold_stats and score5 recomputed from the returned pred / pred_err and the noise; two isolated data have an empty
    neighbourhood: NaN rows, skipped and not counted"""
    pb = fold_problem(HAV)
    far = np.array([[70.0, 40.0], [-40.0, 100.0]])
    coords = [np.vstack([pb["coords"][0], far]), pb["coords"][1]]
    values = [np.concatenate([pb["values"][0], [0.3, -0.2]]), pb["values"][1]]
    d = [np.concatenate([pb["d"][0], [0.01, 0.02]]), pb["d"][1]]
    fi, fo = np.concatenate([pb["fold"][0], [1, 3]]).astype(np.int32), pb["fold"][1]
    h = tln.make_handle(native, pb["params"], HAV, coords, values)
    for q in range(2):
        h.set_noise(q, d[q], (1.5, 0.7)[q])
    h.set_local_neighbours(12, 12)
    pred, err, info = h.cv_local_folds(0, fi, fo, n_folds=4, max_dist=pb["max_dist"])
    again = h.cv_local_folds(0, fi, fo, n_folds=4, max_dist=pb["max_dist"])
    h.close()
    assert info["n_empty"] == 2 and np.isnan(pred[-2:]).all()
    assert np.array_equal(pred, again[0], equal_nan=True) and np.array_equal(err, again[1], equal_nan=True)
    assert info["fold_stats"].tobytes() == again[2]["fold_stats"].tobytes() and info["score5"].tobytes() == again[2]["score5"].tobytes()
    e, v = values[0] - pred, err ** 2 + 1.5 * d[0]
    ok = np.isfinite(pred) & (v > 0)
    ref = np.zeros((4, 6))
    for f in range(4):
        s = ok & (fi == f)
        ref[f] = [(fi == f).sum() + (fo == f).sum(), s.sum(), e[s].sum(), (e[s] ** 2).sum(), (e[s] ** 2 / v[s]).sum(), np.log(v[s]).sum()]
    fs = info["fold_stats"]
    print("fold_stats relative deviations:", np.abs(fs[:, 2:] / ref[:, 2:] - 1).max(axis=0))
    assert np.array_equal(fs[:, :2], ref[:, :2]) and fs[1, 1] == (fi == 1).sum() - 1 and fs[3, 1] == (fi == 3).sum() - 1
    np.testing.assert_allclose(fs[:, 2:], ref[:, 2:], rtol=1e-12)
    assert info["score5"][0] == ok.sum()
    np.testing.assert_allclose(info["score5"], ref[:, 1:].sum(axis=0), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# G. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    pb = tln.random_problem(EUC)
    coords, values = [pb["coords"][0][:40], pb["coords"][1][:30]], [pb["values"][0][:40], pb["values"][1][:30]]
    h = tln.make_handle(native, pb["params"], EUC, coords, values)
    ok = (np.arange(40) % 3).astype(np.int32)
    for call in (h.cv_local_folds, h.local_cv_neighbours):
        name = "ck_cv_local_folds" if call == h.cv_local_folds else "ck_debug_local_cv_neighbours"
        bad = ok.copy()
        bad[17] = 3
        with pytest.raises(native.NativeError, match=name + r": label 3 of datum 17 of process 0 is outside \[-1, n_folds = 3\)"):
            call(0, bad, None, n_folds=3, max_dist=0.2)
        other = np.full(30, -1, np.int32)
        other[9] = -5
        with pytest.raises(native.NativeError, match=name + r": label -5 of datum 9 of process 1 is outside"):
            call(0, ok, other, n_folds=3, max_dist=0.2)
        with pytest.raises(native.NativeError, match=name + r": fold 3 is empty: it holds no datum of process 0 \(and 2 of the other"):
            call(0, ok, np.where(np.arange(30) < 2, 3, -1), n_folds=4, max_dist=0.2)
        with pytest.raises(native.NativeError, match=name + r": n_folds = -2 is negative"):
            call(0, ok, None, n_folds=-2, max_dist=0.2)
        for b in ((np.nan, 0.1), (0.1, np.inf)):
            with pytest.raises(native.NativeError, match=name + r": buffer2\[%d\] = .* is not finite" % (0 if b[0] != b[0] else 1)):
                call(0, ok, None, n_folds=3, buffer=b, max_dist=0.2)
        for b in (None, (None, 0.1), (-1.0, 0.0)):
            with pytest.raises(native.NativeError, match=name + r": the fold labels of the predicted process 0 are null and its buffer is off"):
                call(0, None, None, n_folds=0, buffer=b, max_dist=0.2)
        for md in (-1.0, np.nan, np.inf):
            with pytest.raises(native.NativeError, match=name + r": max_dist must be finite and >= 0"):
                call(0, ok, None, n_folds=3, max_dist=md)
        with pytest.raises(native.NativeError, match=name + r": process index 2 out of range"):
            call(2, None, None, n_folds=0, buffer=0.1, max_dist=0.2)
    for q in range(2):
        h.set_trend(q, np.ones((len(coords[q]), 1)))
    with pytest.raises(ValueError, match=r"f0 has shape \(40, 0\), expected \(40, 1\)"):
        h.cv_local_folds(0, ok, None, n_folds=3, max_dist=0.2)
    import ctypes
    out = np.zeros((2, 40))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rc = native.lib().ck_cv_local_folds(h._h, 0, ok.ctypes.data_as(ip), None, 3, None, None, 0.2, out[0].ctypes.data_as(dp),
                                        out[1].ctypes.data_as(dp), None, None, None, None)
    assert rc != 0 and "ck_cv_local_folds: null regressors f0 with a trend of p_i = 1 columns of process 0" in native.lib().ck_last_error().decode()
    pred, _, info = h.cv_local_folds(0, ok, None, n_folds=3, f0=np.ones((40, 1)), max_dist=0.5)     # the handle still works
    assert np.isfinite(pred).any()
    h.close()
    h = tln.make_handle(native, pb["params"], EUC, coords, values)
    h.set_partition(0, 2)
    with pytest.raises(native.NativeError, match=r"ck_cv_local_folds is the single-process form.*world = 2"):
        h.cv_local_folds(0, ok, None, n_folds=3, max_dist=0.2)
    with pytest.raises(native.NativeError, match=r"ck_debug_local_cv_neighbours is the single-process form.*world = 2"):
        h.local_cv_neighbours(0, ok, None, n_folds=3, max_dist=0.2)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# H. Python layer
# ---------------------------------------------------------------------------------------------------------------------
def predictor(**kw):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    pb = fold_problem(HAV)
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(pb["params"]))
    mf = fields.MultiField([fields.Field(pb["coords"][k], pb["values"][k]) for k in range(2)])
    return point_prediction.Predictor(mod, mf, **kw), pb


def test_predictor_cross_validation_folds(native):
    P, pb = predictor(max_neighbours=(8, 5), measurement_error=[pb_d for pb_d in fold_problem(HAV)["d"]], noise_scale=(1.5, 0.7))
    fi, fo = pb["fold"]
    lab = [None if c < 0 else "track%d" % c for c in fi]
    lab_o = [None if c < 0 else "track%d" % c for c in fo]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        df = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, folds=lab, also_withhold=lab_o)
    labels = P.cv_folds_["label"].tolist()
    codes = np.array([labels.index(x) if x is not None else -1 for x in lab], dtype=np.int32)
    codes_o = np.array([labels.index(x) if x is not None else -1 for x in lab_o], dtype=np.int32)
    h = tln.make_handle(native, pb["params"], HAV, pb["coords"], pb["values"])
    for q in range(2):
        h.set_noise(q, pb["d"][q], (1.5, 0.7)[q])
    h.set_local_neighbours(8, 5)
    pred, err, info = h.cv_local_folds(0, codes, codes_o, n_folds=4, max_dist=pb["max_dist"])
    h.close()
    keep = codes >= 0
    order = np.lexsort((pb["coords"][0][keep][:, 1], pb["coords"][0][keep][:, 0]))     # the frame is sorted by the coordinates
    assert list(df.columns) == ["d1", "d2", "data", "pred", "residual", "pred_err", "fold"] and len(df) == keep.sum()
    assert np.array_equal(df["pred"].values, pred[keep][order]) and np.array_equal(df["pred_err"].values, err[keep][order])
    assert df["fold"].tolist() == [lab[a] for a in np.flatnonzero(keep)[order]]
    assert np.array_equal(df["residual"].values, (pb["values"][0] - pred)[keep][order])
    fs = info["fold_stats"]
    cf = P.cv_folds_
    assert list(cf.columns) == ["label", "n_withheld", "n_scored", "me", "rmse", "msdr", "nlpd_marginal"]
    assert np.array_equal(cf["n_withheld"].values, fs[:, 0]) and np.array_equal(cf["n_scored"].values, fs[:, 1])
    assert np.array_equal(cf["me"].values, fs[:, 2] / fs[:, 1]) and np.array_equal(cf["rmse"].values, np.sqrt(fs[:, 3] / fs[:, 1]))
    assert np.array_equal(cf["msdr"].values, fs[:, 4] / fs[:, 1])
    assert np.array_equal(cf["nlpd_marginal"].values, 0.5 * (fs[:, 1] * np.log(2.0 * np.pi) + fs[:, 5] + fs[:, 4]))
    s5 = info["score5"]
    assert P.cv_scores_["n_scored"] == keep.sum() and P.cv_scores_["rmse"] == np.sqrt(s5[2] / s5[0])
    assert P.cv_scores_["msdr"] == s5[3] / s5[0] and P.cv_scores_["nlpd_marginal"] == 0.5 * (s5[0] * np.log(2.0 * np.pi) + s5[4] + s5[3])
    assert P.info["k_max"] == 13 and P.info["n_capped"] == keep.sum() and P.timings["n_predicted"] == keep.sum()
    P.close()


def test_predictor_cross_validation_kfold_buffer_and_today(native):
    P, pb = predictor()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, folds=5, seed=3)
        fa = P.cv_folds_.copy()
        b = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, folds=5, seed=3)
        assert a.equals(b) and fa.equals(P.cv_folds_)
        c = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, folds=5, seed=4)
        assert not a["pred"].equals(c["pred"])
        assert len(a) == 700 and fa["n_withheld"].tolist() == [140] * 5 and sorted(a["fold"].unique()) == [0, 1, 2, 3, 4]
        # buffer alone: every datum predicted, and (0, off) is the leave-one-out of today
        today = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False)
        assert P.cv is True
        P.cv = False
        d = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, buffer=(0.0, None))
        assert P.cv is False and len(P.cv_folds_) == 0 and P.cv_scores_["n_scored"] == 700
        assert list(today.columns) == ["d1", "d2", "data", "pred", "residual", "pred_err"]
        assert d[list(today.columns)].equals(today) and d["fold"].isna().all()
        wide = P.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, buffer=40.0)
        assert np.mean(wide["pred_err"]) > np.mean(d["pred_err"])         # the near neighbours are gone
        # the method without a new argument: exactly today's code path
        P.cv = True
        f = P.mf.fields[0]
        import pandas as pd
        data = pd.DataFrame(np.hstack((f.coords_main, np.atleast_2d(f.values_main).T)), columns=["d1", "d2", "data"])
        out = P(0, data[["d1", "d2"]], max_dist=pb["max_dist"], postprocess=False)
        df = out.to_dataframe().reset_index() if hasattr(out, "to_dataframe") else out.reset_index()
        df = df.dropna(subset=["pred"]).merge(data, on=["d1", "d2"], how="outer")
        df["residual"] = df["data"] - df["pred"]
        assert today.equals(df[["d1", "d2", "data", "pred", "residual", "pred_err"]])
    P.close()
    Pu, _ = predictor(trend="constant", max_neighbours=(12, 12))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        u = Pu.cross_validation(0, max_dist=pb["max_dist"], postprocess=False, folds=4, seed=1)
    assert np.isfinite(u["pred"]).all() and Pu.trend_coef.shape == (700, 2) and Pu.info["n_rank_def"] == 0
    Pu.close()
