"""What tests/test_gpu_global_sites.py leans on, from the oracle alone (no GPU): the whole-globe inputs of tests/global_sites.py are
well conditioned under every parameter set, half of their pairs lie beyond the covariance tables' upper end, the two clusters
overflow the deferral worklist, the two spellings of one place are distinct sites for the oracle (d > 0) while a true duplicate
is at exactly 0, exact antipodes have a finite distance, and no prediction site has an empty neighbourhood.  For
tests/test_gpu_global_sites_newer.py: the blocks, simulation sites, folds and Vecchia fixtures on the globe reach what that file
claims -- pairs strictly outside the table among (member, neighbour) pairs, member pairs, candidates and set members, both size
classes, a fold across the antimeridian, d = 0 across the processes -- with every cut in a gap of the distances."""
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


# ---------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_global_sites_newer.py leans on: every pinned value is the REFERENCE's property, not the device's
# ---------------------------------------------------------------------------------------------------------------------
def newer():
    from tests import test_gpu_global_sites_newer as tn
    return tn


def outside_pairs(A, B):
    """number of pairs (a, b) strictly outside a haversine table [0, 2): beyond 10 007.5 km by more than rounding"""
    return int(np.count_nonzero(gs.strictly_outside(gs.chord_q(A, B), 0.0, 2.0)))


def test_around_is_a_great_circle_offset_that_keeps_the_longitude_as_it_comes():
    rng = np.random.default_rng(1)
    dist, bearing = rng.uniform(0.0, 19000.0, 200), rng.uniform(0.0, 2.0 * np.pi, 200)
    for centre in [(90.0, 37.0), (-90.0, 0.0), (20.0, 179.995), (-33.0, -179.995), (12.5, -460.0), (89.99, 10.0)]:
        x = gs.around(centre, dist, bearing)
        d = orc.haversine_km([centre], x)[0]
        assert np.max(np.abs(d - dist)) < 1e-8 * orc.EARTH_RADIUS, centre
        assert np.all(np.abs(x[:, 0]) <= 90.0) and np.all(np.abs(x[:, 1] - centre[1]) <= 180.0)
        if abs(centre[1]) > 170.0:
            assert np.any(np.abs(x[:, 1]) > 180.0)                   # not brought back into [-180, 180]
    # at a pole the centre's longitude says where bearing 0 points: due "north" of the south pole along its own meridian
    x = gs.around((-90.0, 25.0), [1000.0, 1000.0], [0.0, 0.5 * np.pi])
    np.testing.assert_allclose(x[:, 1], [25.0, 115.0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(gs.around((10.0, 20.0), 0.0, 1.0), [[10.0, 20.0]], rtol=0, atol=1e-12)


def test_globe_blocks_are_what_the_gpu_tests_say_they_are():
    tn = newer()
    centres, pc, lab, w = tn.block_case()
    assert np.array_equal(centres, gs.globe_pred_sites(np.random.default_rng(gs.BLOCK_SEED), 8))
    assert np.array_equal(np.bincount(lab), gs.BLOCK_SIZES) and len(lab) == sum(gs.BLOCK_SIZES)
    assert pc[:, 1].min() < -180.0 and pc[:, 1].max() > 180.0       # the device must be periodic in lon
    wsum = np.bincount(lab, weights=w)
    for b, (q, reach) in enumerate(zip(gs.BLOCK_SIZES, gs.BLOCK_REACH_KM)):
        x = pc[lab == b]
        d = orc.haversine_km(centres[b:b + 1], x)[0]
        assert d.max() <= reach + 1e-6 and (q < 17 or d.max() > 0.5 * reach), b
        if q > 1:
            assert orc.haversine_km(x, x)[np.triu_indices(q, k=1)].min() > 1e-6, b   # no nugget decision between members rests on rounding
        if b == gs.BLOCK_CANCELLING:
            assert abs(wsum[b]) < 1e-15 and np.any(w[lab == b] < 0)
        else:
            assert abs(wsum[b] - 1.0) < 1e-14 and np.all(w[lab == b] > 0)
    assert not np.array_equal(lab, np.sort(lab))                     # the members of the blocks are interleaved
    # sigma_BB over member pairs on opposite sides of the globe
    far_members = {b: outside_pairs(pc[lab == b], pc[lab == b]) // 2 for b in gs.BLOCK_HEMISPHERES}
    print(f"member pairs beyond {gs.QUARTER_KM:.1f} km in the hemisphere blocks: {far_members}")
    assert min(far_members.values()) > 100


@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_block_chain_on_the_globe(max_dist):
    """every block OK in block_reference, the size class, the conditioning, the variance, and the (member, neighbour) pairs beyond
    the table: at 3 000 km every one of them is a pair the centre itself does not have (its neighbours are within the table)"""
    tn = newer()
    centres, pc, lab, w = tn.block_case()
    n_far = 0
    for b in range(len(centres)):
        near = orc.haversine_km(centres[b:b + 1], gs.GLOBE["coords"][0])[0] <= max_dist
        n_far += outside_pairs(pc[lab == b], gs.GLOBE["coords"][0][near])
    print(f"blocks at {max_dist:g} km: (member, datum of process 0) pairs strictly beyond the table: {n_far}")
    assert n_far > (10000 if max_dist == 12000.0 else 100)
    p = orc.Params.from_flat(gs.GLOBE_PARAMS["long"])
    for i in (0, 1):
        for kind in (None, "constant"):
            for noise in (False, True):
                if noise and kind is not None:
                    continue
                ref = tn.block_chain(i, max_dist, kind, noise)
                print(f"blocks {max_dist:g} km i {i} {kind} noise {noise}: k {ref['k'].min()} .. {ref['k'].max()}, cond {ref['cond'].max():.2e}, "
                      f"var {ref['var'].min():.3e} .. {ref['var'].max():.3e}, sigma_BB of the contrast {ref['sbb'][gs.BLOCK_CANCELLING]:.3e}")
                assert np.all(ref["status"] == tn.OK)
                assert (ref["k"].max() <= 64) if max_dist == 3000.0 else (ref["k"].min() > 64)   # the LDS class | the tiled class
                assert ref["cond"].max() < 1e3 and ref["var"].min() >= 1e-3
                assert 0 < ref["sbb"][gs.BLOCK_CANCELLING] < 0.01 * (p.sigma[i] ** 2 + p.nugget[i])


@pytest.mark.parametrize("max_dist", gs.BLOCK_REACHES)
def test_a_wrong_entry_beyond_the_table_moves_the_block_chain_far_beyond_the_tolerance(monkeypatch, max_dist):
    """The teeth of the comparison, shown on the reference: every covariance beyond 10 007.5 km off by 1 % -- a wrong
    table-or-exact decision is off by the order of the entry itself -- moves pred of every block that has such a pair by more than
    a thousand tolerances (rtol 1e-8, atol 1e-10) and the variance of the hemisphere blocks by more than ten.  At 3 000 km the only
    such pairs are (member, neighbour) and (member, member) pairs of the hemisphere blocks; at 12 000 km Sigma_loc holds them too.
    Measured with 1e-4 instead of 1e-2: pred 76 and 303 tolerances (3 000 km), 56 .. 2 899 (12 000 km); variance 38 and 53, 0.3
    and 3.1 -- the variance of a compact block sees its far entries in second order only."""
    tn = newer()
    from tests import test_gpu_local_blocks as tlb
    centres, pc, lab, w = tn.block_case()
    ref = tn.block_chain(0, max_dist, None)
    cov, cross = orc.covariance, orc.cross_covariance

    def off(c, d):
        return c * np.where(np.asarray(d) > gs.QUARTER_KM, 1.0 + 1e-2, 1.0)
    monkeypatch.setattr(orc, "covariance", lambda p, i, d, use_nugget=True: off(cov(p, i, d, use_nugget=use_nugget), d))
    monkeypatch.setattr(orc, "cross_covariance", lambda p, i, j, d: off(cross(p, i, j, d), d))
    bad = tlb.block_reference(orc.Params.from_flat(gs.GLOBE_PARAMS["long"]), gs.GLOBE["coords"], gs.GLOBE["values"], HAV, centres, pc,
                              lab, w, 0, max_dist)
    tol_p, tol_v = 1e-8 * np.abs(ref["pred"]) + 1e-10, 1e-8 * np.abs(ref["var"]) + 1e-10
    moved_p, moved_v = np.abs(bad["pred"] - ref["pred"]) / tol_p, np.abs(bad["var"] - ref["var"]) / tol_v
    print(f"{max_dist:g} km: far entries off by 1e-2 move pred by {moved_p.round(1)} and the variance by {moved_v.round(1)} tolerances")
    for b in gs.BLOCK_HEMISPHERES:
        assert moved_p[b] > 1000.0 and moved_v[b] > 10.0, b
    if max_dist == 12000.0:                                           # here Sigma_loc itself holds far pairs: every block moves
        assert np.all(moved_p > 1000.0)


def test_lon_folds_put_a_fold_across_the_antimeridian():
    c0, c1 = gs.GLOBE["coords"]
    f0, f1 = gs.lon_folds(c0), gs.lon_folds(c1)
    assert np.bincount(f0).tolist() == [53, 50, 53, 68, 52, 54] and np.bincount(f1).tolist() == [51, 44, 51, 55, 38, 51]
    for c, f in ((c0, f0), (c1, f1)):
        lon = c[f == 0, 1]
        assert np.all((lon >= 150.0) | (lon < -150.0)) and np.any(lon > 150.0) and np.any(lon < -150.0)
    assert f0[2] == f0[3] == 0 and f1[2] == 0                        # (10, 180), (10, -180)
    assert f1[5] == f0[6] == 0                                        # (45, -179.999) and its lon + 360 copy
    assert np.array_equal(f1[50:50 + gs.N_CO], f0[100:100 + gs.N_CO])  # co-located data share their fold
    assert gs.lon_folds(np.array([[0.0, 149.999], [0.0, 150.0], [0.0, -150.0], [0.0, -150.001 - 360.0]])).tolist() == [5, 0, 1, 0]


@pytest.mark.parametrize("i", [0, 1])
def test_simulation_references_on_the_globe(i):
    tn = newer()
    full = gs.globe_pred_sites(np.random.default_rng(gs.SIM_SITE_SEED), gs.SIM_M)
    sites = gs.sim_sites(np.random.default_rng(gs.SIM_SITE_SEED), gs.SIM_M, i)
    gone = [r for r in range(gs.SIM_M) if not (sites == full[r]).all(axis=1).any()]
    assert gone == ([0, 1, 4, 5] if i == 0 else [0, 1])              # (90, 37) IS the datum (90, 0) / (90, 120)
    for row in (2, 3, 6):
        assert (sites == full[row]).all(axis=1).any()
    for which, (max_dist, caps) in enumerate(gs.SIM_CASES):
        pb, ref = tn.sim_case(i, which)
        allc = np.vstack([gs.GLOBE["coords"][0], gs.GLOBE["coords"][1], pb["sites"]])
        D = orc.haversine_km(pb["sites"], allc)
        n_far = int(np.count_nonzero(gs.strictly_outside(gs.chord_q(pb["sites"], allc), 0.0, 2.0) & (D <= max_dist)))
        print(f"{pb['label']}: gap {ref['gap']:.2e}, k_max {ref['k_max']}, levels {ref['n_levels']}, ns_max {ref['ns_max']}, var >= "
              f"{ref['var'].min():.3f}, candidates beyond the table {n_far}")
        assert ref["info"] == 0 and ref["gap"] > 1e-9 and ref["k_max"] <= 64 and ref["n_levels"] >= 4 and ref["n_empty"] == 0
        assert np.count_nonzero(ref["count"][:, 2] >= 3) >= 1 and ref["var"].min() > 0.05
        assert np.min(np.abs(D - max_dist)) > 1e-9 * max_dist        # no candidate within rounding of the reach
        if max_dist == 12000.0:
            assert n_far > 1000 and ref["n_capped"] == len(pb["sites"])
            cross = [np.ptp(np.mod(allc[mem, 1], 360.0)) < 60.0 and np.ptp(allc[mem, 1]) > 300.0 for mem in ref["members"]]
            assert any(cross)                                         # a set across the antimeridian
        # sites on data, the pole that is a datum: regular once every datum carries measurement error
        pbn, refn = tn.sim_case(i, which, on_data=True)
        assert len(pbn["sites"]) == gs.SIM_M and refn["info"] == 0 and refn["gap"] > 1e-9 and refn["k_max"] <= 64 and refn["n_empty"] == 0
        assert orc.haversine_km(pbn["sites"], gs.GLOBE["coords"][0]).min(axis=1)[[0, 1, 4, 5]].max() < 1e-6   # sites on data


@pytest.mark.parametrize("i", [0, 1])
def test_cross_validation_selections_on_the_globe(i):
    """numpy's selection of every case lies in gaps of the distances; the cases reach both size classes, k = 65, emptied
    neighbourhoods, and neighbourhoods with pairs beyond the table"""
    tn = newer()
    D = tn.cv_distances(i)
    assert np.count_nonzero(D[1 - i] == 0.0) == gs.N_CO + 2          # d = 0 across the processes
    for case in gs.CV_CASES:
        max_dist, caps, buf, labelled = case
        sel = tn.cv_selection(i, case)
        k = sel[0][0].sum(axis=1) + sel[1][0].sum(axis=1)
        gap = min(s[3].min() for s in sel)
        near_reach = min(np.min(np.abs(d - max_dist)) for d in D) / max_dist
        near_buffer = min((np.min(np.abs(D[q][D[q] > 0] - buf[q])) / buf[q] for q in range(2) if buf is not None and buf[q]), default=np.inf)
        print(f"cv {case} i {i}: k {k.min()} .. {k.max()}, {np.count_nonzero(k == 65)} at 65, {np.count_nonzero(k == 0)} emptied, smallest gap "
              f"{gap:.2e}, nearest to the reach {near_reach:.2e}, to the buffer {near_buffer:.2e}")
        assert gap > 1e-9 and near_reach > 1e-9 and near_buffer > 1e-9
        assert not any(sel[i][0][a, a] for a in range(len(k)))       # no datum predicts itself
        if max_dist == 3000.0:
            assert k.max() <= 64 and (np.count_nonzero(k == 0) > 0) == labelled   # the LDS class; a fold empties some neighbourhoods
        elif caps != (0, 0):
            assert np.all(k == 65)                                    # the first size beyond the LDS class
        else:
            assert k.min() > 200                                      # the tiled class at some hundreds
            n_far = 0
            for a in range(0, len(k), 10):
                x = np.vstack([gs.GLOBE["coords"][q][sel[q][0][a]] for q in range(2)])
                n_far += outside_pairs(x, x) // 2
            assert n_far > 10000
    fold = gs.lon_folds(gs.GLOBE["coords"][i])
    case = gs.CV_CASES[3]                                             # labels alone: a fold member sees nothing of its fold
    sel = tn.cv_selection(i, case)
    for q in range(2):
        fq = gs.lon_folds(gs.GLOBE["coords"][q])
        assert not np.any(sel[q][0] & (fold[:, None] == fq[None, :]))


def test_cross_validation_culling_sites():
    coords = gs.culling_sites()
    assert [len(c) for c in coords] == [3000, 2600]
    assert np.bincount(gs.lon_folds(coords[0]), minlength=6).min() > 0
    D = [orc.haversine_km(coords[0][:60], c) for c in coords]
    for md in gs.CV_CULL_REACHES + gs.CV_CULL_BUFFER:
        assert min(np.min(np.abs(d[d > 0] - md)) for d in D) > 1e-9 * md
    assert all(np.any(d[d > 0] <= gs.CV_CULL_BUFFER[q]) for q, d in enumerate(D))   # the buffer withholds something


def test_vecchia_fixtures_on_the_globe():
    """the sets are those of test_vecchia_on_the_globe; set members lie beyond the table; the information reference's floor
    (the procedure of tests/test_vecchia_info_host.py: test_reference_floor) leaves info_tol's default as the bound"""
    from tests import dense_chains as dc
    from tests import vecchia_info_ref as vir
    allc = np.vstack(gs.GLOBE["coords"])
    for label in ("globe16/long", "globe16noise/long"):
        f, sets = vir.fixture(label), vir.sets_of(label)
        assert np.array_equal(f["ranks"], np.random.default_rng(gs.VECCHIA_RANK_SEED).permutation(gs.N0 + gs.N1))
        assert (f["max_dist"], tuple(f["caps"])) == (gs.VECCHIA_REACH, gs.VECCHIA_CAPS) and f["params"] == gs.GLOBE_PARAMS["long"]
        assert sets["gap"].min() > 1e-9 and sets["info"] == 0 and sets["k_max"] == 32 and sets["n_capped"] > 500
        n_far = sum(outside_pairs(allc[np.r_[np.flatnonzero(sets["keep"][t]), t]], allc[np.r_[np.flatnonzero(sets["keep"][t]), t]]) // 2
                    for t in range(0, len(allc), 5))
        e = dc.class_errors(dc.normalised(vir.reference(label, scale=0.5), vir.reference(label)), 11)
        print(f"{label}: smallest gap {sets['gap'].min():.2e}, pairs beyond the table inside every fifth set {n_far}; floor of the "
              f"reference exact {e['exact']:.2e} length scale {e['len']:.2e} nu {e['nu']:.2e}")
        assert n_far > 1000
        assert label not in vir.INFO_LEN_FLOOR and vir.info_tol(label) == dict(exact=1e-9, len=1e-9, nu=1e-6)
        assert e["exact"] == 0.0 and 10.0 * e["len"] <= 1e-9 and e["nu"] < 1e-7


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
