"""What tests/test_gpu_global_sites.py leans on, from the oracle alone (no GPU): the whole-globe inputs of tests/global_sites.py are
well conditioned under every parameter set, half of their pairs lie beyond the covariance tables' upper end, the two clusters
overflow the deferral worklist, the two spellings of one place are distinct sites for the oracle (d > 0) while a true duplicate
is at exactly 0, exact antipodes have a finite distance, and no prediction site has an empty neighbourhood."""
import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import global_sites as gs

HAV = 0
MAX_DISTS = (3000.0, 9000.0, 12000.0, 19500.0, 1e9)     # the reaches of the local predictor's GPU tests


@pytest.mark.parametrize("name", list(gs.GLOBE_PARAMS))
def test_sigma_is_finite_and_well_conditioned(name):
    S = orc.joint_cov(orc.Params.from_flat(gs.GLOBE_PARAMS[name]), gs.GLOBE["coords"], HAV)
    assert S.shape == (gs.N0 + gs.N1,) * 2 and np.all(np.isfinite(S))
    w = np.linalg.eigvalsh(S)
    print(f"{name}: cond {w[-1] / w[0]:.3g}, smallest eigenvalue {w[0]:.3g}")
    assert w[0] > 0 and w[-1] / w[0] < 1e4


def test_half_of_the_pairs_lie_beyond_the_table():
    allc = np.vstack(gs.GLOBE["coords"])
    D = orc.haversine_km(allc, allc)
    iu = np.triu_indices(len(allc), k=1)
    share = np.mean(D[iu] > gs.QUARTER_KM)
    q = gs.chord_q(allc, allc)
    print(f"share of pairs beyond {gs.QUARTER_KM:.1f} km: {share:.4f}; by chord q > 2: {np.mean(q[iu] > 2.0):.4f}")
    assert 0.4 < share < 0.6
    # the chord helper and the oracle's distance say the same thing away from the boundary: q = 4 sin^2(d / 2R)
    far = np.abs(D[iu] - gs.QUARTER_KM) > 1e-6
    assert np.array_equal((q[iu] > 2.0)[far], (D[iu] > gs.QUARTER_KM)[far])
    np.testing.assert_allclose(q, 4.0 * np.sin(D / (2.0 * orc.EARTH_RADIUS)) ** 2, rtol=0, atol=1e-14)


def test_clusters_overflow_the_worklist():
    a, b = gs.CLUSTERS["coords"]
    q = gs.chord_q(a, b)
    D = orc.haversine_km(a, b)
    print(f"A x B: {q.size} pairs, q in {q.min():.4f} .. {q.max():.4f}, d in {D.min():.0f} .. {D.max():.0f} km")
    assert q.min() > 2.0 * (1.0 + 1e-12)
    assert q.size > gs.WORKLIST_CAP
    assert D.min() > gs.QUARTER_KM
    # inside a cluster nothing is beyond the table
    assert gs.chord_q(a, a).max() < 2.0 and gs.chord_q(b, b).max() < 2.0
    (la, lb), (oa, ob) = gs.CLUSTERS["box_b"]
    assert b[:, 0].min() >= la and b[:, 0].max() <= lb and b[:, 1].min() >= oa and b[:, 1].max() <= ob


def test_two_spellings_of_one_place_are_distinct_sites_and_a_duplicate_is_not():
    def d(p, q):
        return float(orc.haversine_km([p], [q])[0, 0])
    c0, c1 = gs.GLOBE["coords"]
    pairs = {"poles": ((90.0, 0.0), (90.0, 120.0)), "antimeridian": ((10.0, 180.0), (10.0, -180.0)),
             "equator": ((0.0, 180.0), (0.0, -180.0)), "lon + 360": (tuple(c0[6]), tuple(c1[5]))}
    for what, (p, q) in pairs.items():
        print(f"{what}: {d(p, q):.3e} km")
        assert 0.0 < d(p, q) < 1e-9, what
    assert tuple(c0[2]) == (10.0, 180.0) and tuple(c0[3]) == (10.0, -180.0)       # both spellings inside process 0
    assert tuple(c1[0]) == (90.0, 120.0) and tuple(c0[0]) == (90.0, 0.0)
    assert c1[5][1] == c0[6][1] + 360.0 and c1[5][0] == c0[6][0]
    assert d(c0[2], c1[2]) == 0.0                                                    # (10, 180) of both processes
    assert np.array_equal(c1[50:50 + gs.N_CO], c0[100:100 + gs.N_CO])
    D01 = orc.haversine_km(c0, c1)
    assert np.count_nonzero(D01 == 0.0) == gs.N_CO + 2                               # the block, (10, 180) and (0, 0)


def test_antipodes_have_a_finite_distance_and_a_well_conditioned_sigma():
    rng = np.random.default_rng(3)
    lat, lon = np.degrees(np.arcsin(rng.uniform(-1, 1, 4000))), rng.uniform(-180, 180, 4000)
    anti = np.column_stack([-lat, np.where(lon > 0, lon - 180.0, lon + 180.0)])
    D = orc.haversine_km(np.column_stack([lat, lon]), anti).diagonal()
    assert np.all(np.isfinite(D)) and np.all(np.abs(D - np.pi * orc.EARTH_RADIUS) < 1e-3)
    ap = gs.antipodes()
    d = orc.haversine_km(ap["base"], ap["anti"]).diagonal()
    # asin at its branch point: one rounding of r below 1 is 2 R sqrt(2 * 1.1e-16) = 1.9e-4 km
    print(f"antipodes: pi R - d up to {np.max(np.pi * orc.EARTH_RADIUS - d):.3e} km")
    assert np.all(np.isfinite(d)) and np.all(np.abs(d - np.pi * orc.EARTH_RADIUS) < 1e-3)
    dc = orc.haversine_km(ap["base"], ap["copy"]).diagonal()
    print(f"lon -+ 360 copies: d in {dc.min():.3e} .. {dc.max():.3e} km, {np.count_nonzero(dc == 0)} at exactly 0")
    assert np.all(dc < 1e-9)
    p = orc.Params.from_flat(gs.GLOBE_PARAMS["long"])
    S = orc.joint_cov(p, ap["coords"], HAV)
    w = np.linalg.eigvalsh(S)
    print(f"antipodes: cond {w[-1] / w[0]:.3g}")
    assert np.all(np.isfinite(S)) and w[0] > 0 and w[-1] / w[0] < 1e4
    # an antipodal covariance is not small under this set: exp(-10) of the variance
    n = len(ap["base"])
    assert np.all(S[np.arange(n), n + np.arange(n)] > 1e-5)


@pytest.mark.parametrize("what", ["antipodes-long", "globe-short", "globe-A"])
def test_oracle_floor_under_a_one_ulp_nudge_justifies_the_entry_bound(what):
    """The GPU tests compare Sigma with orc.joint_cov entry by entry at gs.joint_cov_tolerance: rtol 5e-13 plus the move of the
    oracle's own entry under the haversine formula's rounding.  Nudging every coordinate by one ulp (as
    test_parity_in_units_of_the_oracles_own_perturbation_floor does) moves the ORACLE by more than rtol 5e-13 near the antipode
    -- 1.5e-7 relative at exact antipodes under len_scale 2000, 1e-11 under len_scale 100 -- and never by more than the bound."""
    data, name = what.split("-")
    coords = gs.antipodes()["coords"] if data == "antipodes" else gs.GLOBE["coords"]
    p = orc.Params.from_flat(gs.GLOBE_PARAMS[name])
    S = orc.joint_cov(p, coords, HAV)
    tol = gs.joint_cov_tolerance(p, coords, S)
    floor, n_beyond = 0.0, 0
    for toward in (np.inf, -np.inf):
        Sn = orc.joint_cov(p, [np.nextafter(c, toward) for c in coords], HAV)
        dS = np.abs(Sn - S)
        nz = S != 0
        floor = max(floor, float(np.max(dS[nz] / np.abs(S[nz]))))
        n_beyond = max(n_beyond, int(np.count_nonzero(dS > 5e-13 * np.abs(S))))
        assert np.all(dS <= tol), (what, float(np.max(dS / np.maximum(tol, 1e-300))))
    widened = np.count_nonzero(tol > 6e-13 * np.abs(S)) / S.size
    print(f"{what}: the oracle moves by up to {floor:.2e} relative under a 1-ulp nudge ({n_beyond} entries beyond rtol 5e-13); "
          f"share of entries whose bound exceeds rtol 6e-13: {widened:.4f}")
    # measured: antipodes-long 1.55e-07 (24 entries beyond rtol 5e-13), globe-short 2.60e-12 (430 entries), globe-A 2.96e-13 (none)
    if what != "globe-A":
        assert floor > 5e-13
    # the bound stays a bound: at most the move of the distance at the exact antipode (5.4e-4 km) times the covariance's
    # steepest logarithmic slope sqrt(2 nu) / len_scale (1.2 x: nu < 1/2 overshoots it slightly), and rtol 1e-12 for half the entries
    rel_tol = tol[S != 0] / np.abs(S[S != 0])
    slope = float(np.max(np.sqrt(2.0 * p.nu) / p.len_scale))
    print(f"{what}: bound / |entry|: median {np.median(rel_tol):.2e}, largest {rel_tol.max():.2e}")
    assert rel_tol.max() < 5e-13 + 1.2 * 5.4e-4 * slope and np.median(rel_tol) < 1e-12


@pytest.mark.parametrize("m", [70, 300])
def test_prediction_sites_hold_the_awkward_places_and_have_neighbours(m):
    pc = gs.globe_pred_sites(np.random.default_rng(m), m)
    c0, c1 = gs.GLOBE["coords"]
    assert pc.shape == (m, 2) and np.all(np.abs(pc[:, 0]) <= 90.0)
    assert np.any(pc[:, 0] == 90.0) and np.any(pc[:, 0] == -90.0)
    d_east = orc.haversine_km([pc[2]], [(pc[2][0], 180.0)])[0, 0]
    d_west = orc.haversine_km([pc[3]], [(pc[3][0], -180.0)])[0, 0]
    assert pc[2][1] > 0 > pc[3][1] and 0 < d_east < 1.0 and 0 < d_west < 1.0
    assert np.array_equal(pc[4], c0[gs.PRED_DATUM]) and pc[5][0] == pc[4][0] and abs(pc[5][1] - pc[4][1]) == 360.0
    assert orc.haversine_km([pc[4]], [c0[gs.PRED_DATUM]])[0, 0] == 0.0
    assert 0.0 < orc.haversine_km([pc[5]], [c0[gs.PRED_DATUM]])[0, 0] < 1e-9
    for i, c in enumerate((c0, c1)):
        near = np.count_nonzero(orc.haversine_km(pc, c) <= min(MAX_DISTS), axis=1)
        print(f"m = {m}: neighbours of process {i} within {min(MAX_DISTS):.0f} km: {near.min()} .. {near.max()}")
        assert near.min() >= 1


def test_local_oracle_has_no_nan_on_the_globe():
    """the case-count convention of tests/test_gpu_local.py: NaN only where the oracle has them -- here nowhere"""
    pc = gs.globe_pred_sites(np.random.default_rng(12), 12)
    p = orc.Params.from_flat(gs.GLOBE_PARAMS["A"])
    for md in MAX_DISTS:
        pred, err = orc.local_predict(p, gs.GLOBE["coords"], gs.GLOBE["values"], pc, 0, HAV, md)[:2]
        assert np.all(np.isfinite(pred)) and np.all(np.isfinite(err)), md


def test_variogram_oracle_reaches_beyond_half_the_circumference():
    c, v = gs.vario_sites(700, 5)
    half = np.pi * orc.EARTH_RADIUS
    total = {}
    for md in (3000.0, 12000.0, 20015.0, 1e9):
        cen, edg, mean, cnt = orc.variogram(c, v, c, v, True, HAV, md, 20)
        total[md] = int(cnt.sum())
        if md >= 20015.0:
            assert edg[-1] > half
    print("pairs per reach:", total)
    assert total[3000.0] < total[12000.0] < total[20015.0] <= total[1e9] == 700 * 699 // 2
