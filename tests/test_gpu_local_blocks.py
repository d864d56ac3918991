"""GPU tests of block cokriging in the moving neighbourhood: include/cokrige.h ck_predict_local_blocks,
native.Handle.predict_local_blocks and point_prediction.Predictor.predict_blocks.

  1. blocks of one site with weight 1 are the point call, bit for bit (trend or none, neighbour cap, noise);
  2. with max_dist beyond the domain the block is the joint predictor's ck_predict_blocks on the same data;
  3. a dense float64 chain written here (the neighbours of the centre by the oracle's distance, Sigma_loc, cbar and sigma_BB from
     the oracle's covariances, numpy Cholesky, the GLS step of tests/test_gpu_local_universal.py) at the sizes around the LDS
     limit, on both size classes, for q = 1, 3, 64 and 300 members, both metrics, simple / constant / linear;
  4. the degenerate blocks; 5. determinism and order; 6. refusals; 7. the Python layer.

Tolerances are the local path's own (tests/test_gpu_local.py): rtol 1e-8, atol 1e-10 on pred and on pred_err^2, beta at the
same against the chain.  The chain's systems are seeded random sites with a nugget: their condition numbers stay below 2e3
(printed by reference_conditioning(), run on the CPU when the seeds were chosen), five orders of magnitude inside what the
tolerance leaves to float64, so no block is left out of a comparison except those the chain itself marks NaN."""
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc
from tests import test_gpu_local_universal as tlu

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV, BIV_EUC = tlu.BIV, tlu.BIV_EUC
OK, EMPTY, NOT_PD, RANK_DEF = tlu.OK, tlu.EMPTY, tlu.NOT_PD, tlu.RANK_DEF
RTOL, ATOL = 1e-8, 1e-10
QS = (1, 3, 64, 300)   # fewer members than slices, still fewer, exactly one per slice at k = 64, many per slice
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


# ---- the dense chain ---------------------------------------------------------------------------------------------------
def block_reference(p, coords, values, metric, centres, pc, lab, w, i, max_dist, Fs=None, F0=None, noise=None):
    """per block: the neighbours of the centre, Sigma_loc (+ noise[k] on the diagonal of process k), cbar, sigma_BB, Cholesky,
    the GLS step under the rules of include/cokrige.h.  Members are taken in the caller's order."""
    n, r = p.n_procs, len(centres)
    pk = [F.shape[1] for F in Fs] if Fs is not None else [0] * n
    P, off = sum(pk), [0, pk[0]]
    Sig = {}
    for a in range(n):
        for b in range(a, n):
            d = orc.distance_matrix(coords[a], coords[b], metric)
            Sig[a, b] = orc.covariance(p, a, d) if a == b else orc.cross_covariance(p, a, b, d)
            if a == b and noise is not None:
                Sig[a, b] = Sig[a, b] + np.diag(noise[a])
    out = dict(pred=np.full(r, np.nan), var=np.full(r, np.nan), beta=np.full((r, P), np.nan), status=np.zeros(r, int),
               k=np.zeros(r, int), cond=np.zeros(r), sbb=np.zeros(r))
    for b in range(r):
        if P and not np.all(np.isfinite(F0[b])):
            out["status"][b] = -1   # rule 5
            dists = [orc.distance_matrix(centres[b], c, metric)[0] for c in coords]
            out["k"][b] = sum(int((d <= max_dist).sum()) for d in dists)
            continue
        dists = [orc.distance_matrix(centres[b], c, metric)[0] for c in coords]
        ix = [d <= max_dist for d in dists]
        nk = [int(x.sum()) for x in ix]
        k = out["k"][b] = sum(nk)
        if k == 0:
            out["status"][b] = EMPTY
            continue
        mem = np.flatnonzero(lab == b)
        xm, wm = pc[mem], w[mem]
        cbar = np.hstack([wm @ (orc.covariance(p, i, orc.distance_matrix(xm, coords[a][ix[a]], metric), use_nugget=True) if a == i
                                else orc.cross_covariance(p, i, a, orc.distance_matrix(xm, coords[a][ix[a]], metric)))
                          for a in range(n) if nk[a] > 0])
        sbb = out["sbb"][b] = wm @ orc.covariance(p, i, orc.distance_matrix(xm, xm, metric), use_nugget=True) @ wm
        z = np.hstack([np.asarray(values[a])[ix[a]] for a in range(n)])
        blk = {}
        for a in range(n):
            for c in range(n):
                blk[a, c] = Sig[a, c][np.ix_(ix[a], ix[c])] if a <= c else Sig[c, a][np.ix_(ix[c], ix[a])].T
        S = np.block([[blk[a, c] for c in range(n)] for a in range(n)])
        out["cond"][b] = np.linalg.cond(S)
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            out["status"][b] = NOT_PD
            continue
        v, y = solve_triangular(L, cbar, lower=True), solve_triangular(L, z, lower=True)
        if P == 0:
            out["pred"][b], out["var"][b] = v @ y, sbb - v @ v
            continue
        X, x0, r0 = np.zeros((k, P)), np.zeros(P), 0
        for a in range(n):
            X[r0:r0 + nk[a], off[a]:off[a] + pk[a]] = Fs[a][ix[a]]
            r0 += nk[a]
        x0[off[i]:off[i] + pk[i]] = F0[b]
        gone = [a for a in range(n) if pk[a] > 0 and nk[a] == 0]
        if i in gone:
            out["status"][b] = RANK_DEF
            continue
        keep = np.array([j for a in range(n) if a not in gone for j in range(off[a], off[a] + pk[a])], dtype=int)
        U = solve_triangular(L, X[:, keep], lower=True)
        A, bb = U.T @ U, U.T @ y
        if tlu.chol_threshold(A) is None:
            out["status"][b] = RANK_DEF
            continue
        out["cond"][b] = max(out["cond"][b], np.linalg.cond(A))
        rr = x0[keep] - U.T @ v
        beta = np.linalg.solve(A, bb)
        out["pred"][b] = v @ y + rr @ beta
        out["var"][b] = sbb - v @ v + rr @ np.linalg.solve(A, rr)
        out["beta"][b, keep] = beta
    return out


def compare(pred, err, info, ref, beta=None, label=""):
    st = ref["status"]
    ok = st == OK
    print(f"{label}: blocks {len(st)} finite {int(ok.sum())} k {int(ref['k'].min())}..{int(ref['k'].max())} cond max "
          f"{ref['cond'].max():.1e} max |dpred| {np.max(np.abs(pred[ok] - ref['pred'][ok]), initial=0):.2e} "
          f"max |dvar| {np.max(np.abs(err[ok] ** 2 - np.maximum(ref['var'][ok], 0)), initial=0):.2e}")
    assert np.array_equal(np.isnan(pred), ~ok) and np.array_equal(np.isnan(err), ~ok)
    assert info["n_empty"] == int((st == EMPTY).sum())
    assert info["n_not_pd"] == int((st == NOT_PD).sum())
    assert info["n_rank_def"] == int((st == RANK_DEF).sum())
    assert info["k_max"] == int(ref["k"].max())
    np.testing.assert_allclose(pred[ok], ref["pred"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(err[ok] ** 2, np.maximum(ref["var"][ok], 0.0), rtol=RTOL, atol=ATOL)
    if beta is not None:
        assert np.array_equal(np.isnan(beta), np.isnan(ref["beta"]))
        fin = ~np.isnan(ref["beta"])
        np.testing.assert_allclose(beta[fin], ref["beta"][fin], rtol=RTOL, atol=ATOL)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def big_data(metric):
    """700 + 650 sites (tests/test_gpu_local_universal.py's)"""
    if ("big", metric) not in _cache:
        _cache["big", metric] = tlu.make_data(3, BIV if metric == HAV else BIV_EUC, metric)
    return _cache["big", metric]


def small_data():
    """70 + 40 seeded sites, the generator of tests/test_gpu_local_lds_boundary.py"""
    if "small" not in _cache:
        _cache["small"] = tlu.make_data(41, BIV, HAV, n0=70, n1=40)
    return _cache["small"]


FAR = (np.array([[-40.0, 100.0], [-41.0, 101.0], [-42.0, 99.0]]), np.array([0.1, -0.2, 0.3]))   # data, but never a neighbour
WHOLE = 8000.0   # km: every datum of the CONUS box, none of FAR


def subset(n0, n1):
    p, coords, values = small_data()
    return p, [coords[k][:n] if n else FAR[0] for k, n in enumerate((n0, n1))], [values[k][:n] if n else FAR[1] for k, n in enumerate((n0, n1))]


def make_blocks(rng, centres, sizes, metric, spread=None):
    """members scattered around every centre (about a degree | 0.3 units), weights that are no mean: non-uniform, their sum
    not 1; the members of all blocks interleaved"""
    spread = spread if spread is not None else (0.6 if metric == HAV else 0.3)
    lab = np.repeat(np.arange(len(centres)), sizes)
    pc = centres[lab] + rng.uniform(-spread, spread, (len(lab), 2))
    w = rng.uniform(0.2, 2.0, len(lab)) / np.asarray(sizes)[lab]
    perm = rng.permutation(len(lab))
    return pc[perm], lab[perm], w[perm]


def block_f0(kind, coords_i, pc, lab, w, r):
    F = tlu.design(kind, coords_i, pc)
    return np.column_stack([np.bincount(lab, weights=w * F[:, j], minlength=r) for j in range(F.shape[1])])


def boundary_case(n0, n1, kind, seed=5):
    """four blocks of 1, 3, 64 and 300 members over the first n0 + n1 data: k = n0 + n1 for every block"""
    p, coords, values = subset(n0, n1)
    rng = np.random.default_rng(seed + 7 * n0 + n1)
    centres = tlu.pred_sites(rng, HAV, len(QS))
    pc, lab, w = make_blocks(rng, centres, QS, HAV)
    w[np.flatnonzero(lab == 2)[0]] *= -1.0   # one negative weight
    Fs = None if kind is None else [tlu.design(kind, c, c) for c in coords]
    return p, coords, values, centres, pc, lab, w, Fs


def general_case(metric, kind, seed=17, r=24):
    """blocks of 1, 3, 64, 300 members in turn over the 700 + 650 sites; a radius that puts blocks into both size classes"""
    p, coords, values = big_data(metric)
    rng = np.random.default_rng(seed)
    centres = tlu.pred_sites(rng, metric, r)
    sizes = np.array([QS[b % 4] for b in range(r)])
    pc, lab, w = make_blocks(rng, centres, sizes, metric)
    Fs = None if kind is None else [tlu.design(kind, c, c) for c in coords]
    return p, coords, values, centres, pc, lab, w, Fs


def set_trend(h, Fs):
    if Fs is not None:
        for k, F in enumerate(Fs):
            h.set_trend(k, F)


def run_blocks(native, case, i, max_dist, kind, tile_min=None, metric=HAV, label="", key=None):
    """key: names (case, i, max_dist) -- the chain is computed once and shared by the routes that are compared with it"""
    p, coords, values, centres, pc, lab, w, Fs = case
    r = len(centres)
    F0 = None if kind is None else block_f0(kind, coords[i], pc, lab, w, r)
    h = tlu.handle(native, p, coords, values, metric)
    if tile_min is not None:
        h.set_option("local_tile_min", tile_min)
    set_trend(h, Fs)
    pred, err, info = h.predict_local_blocks(i, centres, pc, lab, w, f0=F0, max_dist=max_dist, want_beta=True)
    tm = h.local_blocks_timings()
    h.close()
    if ("ref", key) not in _cache or key is None:
        _cache["ref", key] = block_reference(p, coords, values, metric, centres, pc, lab, w, i, max_dist, Fs, F0)
    ref = _cache["ref", key]
    compare(pred, err, info, ref, beta=info["beta"] if kind is not None else None, label=label)
    assert tm["cbar_evals"] == float(np.sum(np.bincount(lab, minlength=r) * ref["k"]))
    return ref, tm


def reference_conditioning():
    """CPU: the largest condition number any reference system of section 3 has (run when the seeds were chosen)"""
    worst = 0.0
    for n0, n1 in SIZES:
        for kind in KINDS:
            p, coords, values, centres, pc, lab, w, Fs = boundary_case(n0, n1, kind)
            for i in [q for q, n in enumerate((n0, n1)) if n > 0]:
                F0 = None if kind is None else block_f0(kind, coords[i], pc, lab, w, len(centres))
                ref = block_reference(p, coords, values, HAV, centres, pc, lab, w, i, WHOLE, Fs, F0)
                assert np.all(ref["status"] == OK), (n0, n1, kind, i, ref["status"])
                worst = max(worst, ref["cond"].max())
    for metric, md in ((HAV, 400.0), (EUC, 1.6)):
        for kind in KINDS:
            p, coords, values, centres, pc, lab, w, Fs = general_case(metric, kind)
            for i in (0, 1):
                F0 = None if kind is None else block_f0(kind, coords[i], pc, lab, w, len(centres))
                ref = block_reference(p, coords, values, metric, centres, pc, lab, w, i, md, Fs, F0)
                print(metric, kind, i, "k", ref["k"].min(), ref["k"].max(), "status", np.bincount(ref["status"] + 1), "cond", ref["cond"].max())
                worst = max(worst, ref["cond"].max())
    print("largest condition number", worst)
    return worst


# ---- 1. singleton identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "constant"])
@pytest.mark.parametrize("variant", ["plain", "cap", "noise"])
def test_singleton_blocks_are_the_point_call_bit_for_bit(native, kind, variant):
    """400 km over 700 + 650 sites: both size classes in one call (without a trend the point call's classes are the block call's
    under the default local_tile_min); the centres are the sites, so the point call searches the same neighbourhoods"""
    p, coords, values = big_data(HAV)
    pc = np.vstack([tlu.pred_sites(np.random.default_rng(17), HAV, 118), [[10.0, -170.0], [62.0, -95.0]]])   # two far away
    m = len(pc)
    h = tlu.handle(native, p, coords, values, HAV)
    if variant == "cap":
        h.set_local_neighbours(16, 12)
    if variant == "noise":
        rng = np.random.default_rng(43)
        for k in range(2):
            h.set_noise(k, 1e-2 * p.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, len(coords[k])), (1.5, 0.7)[k])
    F0 = None
    if kind is not None:
        set_trend(h, [tlu.design(kind, c, c) for c in coords])
        F0 = tlu.design(kind, coords[1], pc)
    pp, pe, pinfo = h.predict_local_universal(1, pc, F0, max_dist=400.0, cv=False, want_beta=True)
    bp, be, binfo = h.predict_local_blocks(1, pc, pc, np.arange(m), np.ones(m), f0=F0, max_dist=400.0, want_beta=True)
    h.close()
    assert pinfo["n_empty"] == 2 and np.isfinite(pp).sum() == m - 2
    if variant == "cap":
        assert pinfo["k_max"] <= 40
    else:
        assert pinfo["k_max"] > 64 and np.isfinite(pp).sum() > 0   # both classes
    np.testing.assert_array_equal(bp, pp)
    np.testing.assert_array_equal(be, pe)
    for key in ("n_empty", "n_not_pd", "n_rank_def", "k_max"):
        assert binfo[key] == pinfo[key], key
    if kind is not None:
        np.testing.assert_array_equal(binfo["beta"], pinfo["beta"])


@pytest.mark.parametrize("kind", [None, "constant"])
def test_singleton_blocks_on_the_tiled_path_alone(native, kind):
    """local_tile_min = 0: every neighbourhood, the smallest included, is a tiled system in both calls"""
    p, coords, values = big_data(HAV)
    pc = tlu.pred_sites(np.random.default_rng(19), HAV, 40)
    h = tlu.handle(native, p, coords, values, HAV)
    h.set_option("local_tile_min", 0)
    F0 = None
    if kind is not None:
        set_trend(h, [tlu.design(kind, c, c) for c in coords])
        F0 = tlu.design(kind, coords[0], pc)
    pp, pe, _ = h.predict_local_universal(0, pc, F0, max_dist=250.0)
    bp, be, _ = h.predict_local_blocks(0, pc, pc, np.arange(40), np.ones(40), f0=F0, max_dist=250.0)
    h.close()
    assert np.isfinite(pp).sum() > 30
    np.testing.assert_array_equal(bp, pp)
    np.testing.assert_array_equal(be, pe)


# ---- 2. whole-domain identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(40, 20), (70, 50)])   # k = 60: the LDS class; k = 120: the tiled class
@pytest.mark.parametrize("i", [0, 1])
def test_whole_domain_blocks_are_the_joint_block_predictor(native, n0, n1, i):
    p, coords, values = tlu.make_data(29, BIV, HAV, n0=n0, n1=n1)
    rng = np.random.default_rng(31)
    sizes = [1, 2, 5, 37]
    centres = tlu.pred_sites(rng, HAV, 4)
    pc, lab, w = make_blocks(rng, centres, sizes, HAV, spread=2.0)
    w[np.flatnonzero(lab == 3)[1]] *= -1.0            # one negative weight; no block's weights sum to 1
    assert np.all(np.abs(np.bincount(lab, weights=w) - 1.0) > 1e-3)
    h = tlu.handle(native, p, coords, values, HAV)
    bp, be, info = h.predict_local_blocks(i, centres, pc, lab, w, max_dist=WHOLE)
    tm = h.local_blocks_timings()
    assert info["k_max"] == n0 + n1 and info["n_empty"] == 0 and info["n_not_pd"] == 0
    assert (tm["tiled_ms"] > 0.0) == (n0 + n1 > 64)
    h.assemble_joint()
    assert h.factor() == 0
    jp, je, _ = h.predict_blocks(i, pc, lab, w, 4)
    h.close()
    print(f"N={n0 + n1} i={i}: max |dpred| {np.max(np.abs(bp - jp)):.2e} max |dvar| {np.max(np.abs(be ** 2 - je ** 2)):.2e}")
    np.testing.assert_allclose(bp, jp, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(be ** 2, je ** 2, rtol=RTOL, atol=ATOL)


# ---- 3. the dense float64 chain ----------------------------------------------------------------------------------------
SIZES = [(63, 0), (64, 0), (32, 32), (33, 32), (40, 26)]   # k = 63, 64, 64 | 65, 66: the first sizes beyond the LDS class
KINDS = [None, "constant", "linear"]


@pytest.mark.parametrize("tile_min", [None, 0])   # the default classes | everything tiled
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n0,n1", SIZES)
def test_chain_at_the_class_boundary(native, n0, n1, kind, tile_min):
    case = boundary_case(n0, n1, kind)
    for i in [q for q, n in enumerate((n0, n1)) if n > 0]:   # a process without neighbours cannot carry its own trend
        ref, tm = run_blocks(native, case, i, WHOLE, kind, tile_min=tile_min, label=f"{n0}+{n1} {kind} i={i} tile_min={tile_min}",
                             key=("boundary", n0, n1, kind, i))
        assert np.all(ref["k"] == n0 + n1) and np.all(ref["status"] == OK)
        assert (tm["tiled_ms"] > 0.0) == (tile_min == 0 or n0 + n1 > 64)


@pytest.mark.parametrize("tile_min", [None, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric,max_dist", [(HAV, 400.0), (EUC, 1.6)])
def test_chain_on_both_classes_and_metrics(native, metric, max_dist, kind, tile_min):
    case = general_case(metric, kind)
    for i in (0, 1):
        ref, _ = run_blocks(native, case, i, max_dist, kind, tile_min=tile_min, metric=metric,
                            label=f"metric {metric} {kind} i={i} tile_min={tile_min}", key=("general", metric, kind, i))
        assert ref["k"][ref["k"] > 0].min() <= 64 < ref["k"].max()


# ---- 4. degenerate blocks ----------------------------------------------------------------------------------------------
def degenerate_case():
    """process 0 lives in the west, process 1 in the east, with an overlap: a centre in the far east has no neighbour of
    process 0 (rule 3 under a trend), one off the map none at all (rule 1), one block gets a NaN regressor (rule 5), one holds
    the same member site twice and a third time with another weight (the nugget where h = 0)"""
    rng = np.random.default_rng(61)
    p = orc.Params.from_flat(BIV)
    coords = [np.column_stack([rng.uniform(28, 48, 260), rng.uniform(-120, -92, 260)]),
              np.column_stack([rng.uniform(28, 48, 240), rng.uniform(-100, -72, 240)])]
    S = orc.joint_cov(p, coords, HAV)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0]) + 0.3
    values = [z[:260], z[260:]]
    centres = np.array([[38.0, -96.0], [10.0, -170.0], [40.0, -75.0], [36.0, -110.0], [42.0, -97.0], [33.0, -95.0]])
    sizes = [5, 4, 6, 3, 7, 3]
    pc, lab, w = make_blocks(rng, centres, sizes, HAV)
    dup = np.flatnonzero(lab == 5)
    pc[dup[1]] = pc[dup[0]]      # the same site twice ...
    pc[dup[2]] = pc[dup[0]]      # ... and a third time, every copy with its own weight
    return p, coords, values, centres, pc, lab, w, [np.ones((len(c), 1)) for c in coords]


def degenerate_f0(case, i, trend):
    p, coords, values, centres, pc, lab, w, Fs = case
    F0 = block_f0("constant", coords[i], pc, lab, w, 6) if trend else None
    if trend:
        F0[4, 0] = np.nan
    return F0


def test_degenerate_blocks(native):
    case = degenerate_case()
    p, coords, values, centres, pc, lab, w, Fs = case
    for i, trend in ((0, True), (1, True), (0, False)):
        F0 = degenerate_f0(case, i, trend)
        h = tlu.handle(native, p, coords, values, HAV)
        set_trend(h, Fs if trend else None)
        pred, err, info = h.predict_local_blocks(i, centres, pc, lab, w, f0=F0, max_dist=300.0, want_beta=True)
        h.close()
        ref = block_reference(p, coords, values, HAV, centres, pc, lab, w, i, 300.0, Fs if trend else None, F0)
        compare(pred, err, info, ref, beta=info["beta"] if trend else None, label=f"degenerate i={i} trend={trend}")
        assert ref["status"][1] == EMPTY and info["n_empty"] == 1
        assert ref["status"][5] == OK   # the duplicated members
        if trend:
            assert ref["status"][4] == -1 and np.isnan(pred[4]) and np.all(np.isnan(info["beta"][4]))
            # the far east sees process 1 only, the far west process 0 only: the other process cannot carry its constant
            assert ref["status"][2 if i == 0 else 3] == RANK_DEF and info["n_rank_def"] == 1
            assert ref["status"][3 if i == 0 else 2] == OK and np.isnan(info["beta"][3 if i == 0 else 2]).sum() == 1   # a dropped column
            assert info["n_empty"] + info["n_not_pd"] + info["n_rank_def"] == int(np.isnan(pred).sum()) - 1   # block 4: no counter
        else:
            assert ref["status"][2] == OK and ref["status"][4] == OK


# ---- 5. determinism and order ------------------------------------------------------------------------------------------
def test_repeated_permuted_and_batched_calls_give_the_same_bits(native):
    case = general_case(HAV, "linear", seed=23, r=32)
    p, coords, values, centres, pc, lab, w, Fs = case
    F0 = block_f0("linear", coords[1], pc, lab, w, 32)

    def call(pc, lab, w, **opts):
        h = tlu.handle(native, p, coords, values, HAV, site_order=opts.pop("site_order", 1))
        for k, v in opts.items():
            h.set_option(k, v)
        set_trend(h, Fs)
        out = [h.predict_local_blocks(1, centres, pc, lab, w, f0=F0, max_dist=400.0, want_beta=True) for _ in range(2)]
        h.close()
        for a, b in zip(out[0][:2] + (out[0][2]["beta"],), out[1][:2] + (out[1][2]["beta"],)):
            np.testing.assert_array_equal(a, b)          # two calls on one handle
        return out[0]

    base = call(pc, lab, w)
    # both classes; block 20 has four neighbours, too few for the six columns (rule 4): a NaN block is part of the comparison
    assert base[2]["k_max"] > 64 and base[2]["n_rank_def"] == 1 and np.isfinite(base[0]).sum() == 31
    # the caller's member order changed ACROSS blocks, kept inside every block: sorting by block with a stable sort, and a
    # random interleaving that keeps every block's members in their order
    stable = np.argsort(lab, kind="stable")
    rng = np.random.default_rng(2)
    keys = np.empty(len(lab))
    for b in range(32):
        mem = np.flatnonzero(lab == b)
        keys[mem] = np.sort(rng.random(len(mem)))
    for order in (stable, np.argsort(keys, kind="stable")):
        for b in range(32):
            assert np.array_equal(order[lab[order] == b], np.flatnonzero(lab == b))
        other = call(pc[order], lab[order], w[order])
        for a, b in zip(base[:2] + (base[2]["beta"],), other[:2] + (other[2]["beta"],)):
            np.testing.assert_array_equal(a, b)
    small = call(pc, lab, w, local_slab_mb=3)             # several batches of tiled systems
    for a, b in zip(base[:2] + (base[2]["beta"],), small[:2] + (small[2]["beta"],)):
        np.testing.assert_array_equal(a, b)
    so = call(pc, lab, w, site_order=0)                   # the tolerance of tests/test_gpu_local.py for this change
    np.testing.assert_allclose(so[0], base[0], rtol=1e-9, atol=1e-11, equal_nan=True)
    np.testing.assert_allclose(so[1] ** 2, base[1] ** 2, rtol=1e-9, atol=1e-11, equal_nan=True)
    assert so[2]["k_max"] == base[2]["k_max"]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_with_the_offender_named(native):
    p, coords, values = small_data()
    h = tlu.handle(native, p, coords, values, HAV)
    centres = np.array([[35.0, -100.0], [40.0, -90.0], [45.0, -80.0]])
    pc = np.repeat(centres, 2, axis=0) + 0.1
    lab, w = np.repeat(np.arange(3), 2), np.full(6, 0.5)
    ok = h.predict_local_blocks(0, centres, pc, lab, w, max_dist=500.0)
    assert np.isfinite(ok[0]).all()

    def bad(match, centres=centres, pc=pc, lab=lab, w=w, f0=None):
        with pytest.raises(native.NativeError, match=match):
            h.predict_local_blocks(0, centres, pc, lab, w, f0=f0, max_dist=500.0)

    bad(r"label 3 of site 4", lab=np.array([0, 0, 1, 1, 3, 2]))
    bad(r"label -1 of site 0", lab=np.array([-1, 0, 1, 1, 2, 2]))
    bad(r"block 1 has no site", lab=np.array([0, 0, 0, 2, 2, 2]))
    bad(r"weight of site 2 is not finite \(nan\)", w=np.array([0.5, 0.5, np.nan, 0.5, 0.5, 0.5]))
    bad(r"weight of site 5 is not finite \(inf\)", w=np.array([0.5, 0.5, 0.5, 0.5, 0.5, np.inf]))
    c2 = centres.copy()
    c2[1, 1] = np.nan
    bad(r"coordinate 1 of centre 1 is not finite", centres=c2)
    p2 = pc.copy()
    p2[3, 0] = np.inf
    bad(r"coordinate 0 of site 3 is not finite", pc=p2)
    for k in range(2):
        h.set_trend(k, np.ones((len(coords[k]), 1)))
    bad(r"null block regressors f0 with a trend of p_i = 1")
    again = h.predict_local_blocks(0, centres, pc, lab, w, f0=np.full((3, 1), 1.0), max_dist=500.0)   # the handle still works
    assert np.isfinite(again[0]).all()
    h.close()


def test_a_partitioned_handle_is_refused(native):
    p, coords, values = small_data()
    h = tlu.handle(native, p, coords, values, HAV)
    h.set_partition(0, 2)
    with pytest.raises(native.NativeError, match=r"ck_predict_local_blocks is the single-process form.*world = 2"):
        h.predict_local_blocks(0, coords[0][:2], coords[0][:2], np.arange(2), np.ones(2), max_dist=500.0)
    h.close()


# ---- 7. the Python layer -----------------------------------------------------------------------------------------------
def predictor(native, **kw):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    p, coords, values = big_data(HAV)
    at = dict(scale_fact=1.7, spatial_mean=0.25, temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
              covariate_scales=[12.0, 6.0], spatial_model=_StubTrend([0.3, -0.2], 0.05))
    fs = [fields.Field(coords[k], values[k]) for k in range(2)]
    for f in fs:
        f.ds = _Attrs(at)
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    return point_prediction.Predictor(mod, fields.MultiField(fs), **kw), at


class _StubTrend:
    def __init__(self, coef, intercept):
        self.coef, self.intercept = np.asarray(coef, dtype=float), float(intercept)

    def predict(self, X):
        return np.asarray(X, dtype=float) @ self.coef + self.intercept


class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


def test_predictor_blocks_frame_centres_and_postprocess(native):
    from sif_xco2_cokriging_amd.joint_prediction import Predictor as Joint
    P, at = predictor(native, trend="constant", max_neighbours=(24, 24))
    rng = np.random.default_rng(9)
    pcn = np.column_stack([rng.uniform(30, 45, 300), rng.uniform(-115, -75, 300)])
    cell = [f"c{int(a) // 5:02d}_{int(-b) // 10:02d}" for a, b in pcn]     # 5 x 10 degree cells, string labels
    cell[7] = None                                                            # a site in no block
    wts = rng.uniform(0.3, 1.5, 300)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                        # nothing empty, nothing rank deficient
        raw = P.predict_blocks(1, pd.DataFrame(pcn, columns=["lat", "lon"]), cell, wts, max_dist=600.0, postprocess=False)
    labels = sorted({c for c in cell if c is not None})
    assert list(raw.index) == labels and raw.index.name == "block"
    assert list(raw.columns) == ["pred", "pred_err", "n_sites", "lat", "lon"]
    assert raw["n_sites"].sum() == 299 and np.isfinite(raw["pred"]).all()
    assert P.trend_coef.shape == (len(labels), 2) and P.info["n_capped"] > 0 and P.info["k_max"] >= 48
    # the library call underneath, with the default centres written out: the normalised mean of the members' unit vectors
    inside = np.array([c is not None for c in cell])
    codes = np.array([labels.index(c) for c in np.array(cell, dtype=object)[inside]])
    pc, w, r = pcn[inside], wts[inside], len(labels)
    la, lo = np.radians(pc[:, 0]), np.radians(pc[:, 1])
    u = np.column_stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    mu = np.column_stack([np.bincount(codes, weights=u[:, c], minlength=r) for c in range(3)])
    mu /= np.linalg.norm(mu, axis=1)[:, None]
    cc = np.column_stack([np.degrees(np.arcsin(mu[:, 2])), np.degrees(np.arctan2(mu[:, 1], mu[:, 0]))])
    np.testing.assert_allclose(P._block_centres(pc, codes, pd.Index(labels), None), cc, rtol=0, atol=1e-12)
    # explicit centres, as an array and as a mapping, give the same frame
    for centres in (cc, {lab: tuple(cc[k]) for k, lab in enumerate(labels)}):
        again = P.predict_blocks(1, pcn, cell, wts, max_dist=600.0, centres=centres, postprocess=False)
        np.testing.assert_allclose(again["pred"].values, raw["pred"].values, rtol=1e-9, atol=1e-11)
    with pytest.raises(ValueError, match="centres has shape"):
        P.predict_blocks(1, pcn, cell, wts, centres=cc[:-1])
    with pytest.raises(ValueError, match="no entry for block"):
        P.predict_blocks(1, pcn, cell, wts, centres={labels[0]: (40.0, -100.0)})
    # postprocess=True: _postprocess_blocks on the synthetic attributes, and that arithmetic written out
    df = P.predict_blocks(1, pcn, cell, wts, max_dist=600.0, postprocess=True)
    P.i = 1
    want = Joint._postprocess_blocks(P, pc, codes, w, r, raw["pred"].values.copy(), raw["pred_err"].values.copy(), None)
    np.testing.assert_array_equal(df["pred"].values, want[0])
    np.testing.assert_array_equal(df["pred_err"].values, want[1])
    assert np.max(np.abs(df["pred"].values - 1.7 * raw["pred"].values)) > 0.1   # the offsets were added
    np.testing.assert_allclose(df["pred_err"].values, 1.7 * raw["pred_err"].values, rtol=1e-15)
    P.close()


def test_default_centres_across_the_date_line_and_cancelling_members(native):
    P, _ = predictor(native)
    pc = np.array([[10.0, 179.0], [10.0, -179.0], [-20.0, 170.0], [-22.0, 172.0]])
    cc = P._block_centres(pc, np.array([0, 0, 1, 1]), pd.Index(["a", "b"]), None)
    assert abs(abs(cc[0, 1]) - 180.0) < 1e-9 and abs(cc[0, 0] - 10.0) < 0.01      # near +-180, not 0
    assert abs(cc[1, 1] - 171.0) < 0.01
    with pytest.raises(ValueError, match="'a'.*centres="):
        P._block_centres(np.array([[0.0, 0.0], [0.0, 180.0]]), np.array([0, 0]), pd.Index(["a"]), None)
    P.close()


def test_more_than_one_device_is_refused(native):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    p, coords, values = small_data()
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    mf = fields.MultiField([fields.Field(coords[k], values[k]) for k in range(2)])
    P = point_prediction.Predictor(mod, mf, devices=[0, 1])
    with pytest.raises(NotImplementedError, match=r"devices=\[0, 1\]"):
        P.predict_blocks(0, coords[0][:4], [0, 0, 1, 1])
    P.close()
