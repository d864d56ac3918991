"""Whole-globe inputs for the haversine paths: sites uniform on the sphere with the places that are awkward there (poles,
the antimeridian written both ways, lon and lon + 360, exact antipodes), two clusters a third of the globe apart, and the
chord-space arithmetic of the covariance tables in numpy.  Plain numpy plus the oracle; tests/test_global_sites_host.py pins
what the GPU tests (tests/test_gpu_global_sites.py, tests/test_gpu_global_sites_newer.py) lean on.

Half of all pairs of GLOBE are more than a quarter of the way round (10 007.5 km, squared chord q = 2): beyond the upper end of
every haversine covariance table, where the table kernels hand the entry to the exact evaluator.  Every cross pair of CLUSTERS
is, and there are more of them than the deferral worklist holds (2 ** 22)."""
import numpy as np

from oracle import cokrige_oracle as orc

HAV, EUC = 0, 1
QUARTER_KM = 0.5 * np.pi * orc.EARTH_RADIUS          # 10 007.5 km: q = 2
WORKLIST_CAP = 1 << 22                               # csrc/ck_api.hip: build_tables

SET_A = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]   # synth.SET_A
GLOBE_PARAMS = {
    "A": SET_A,
    "long": [1.3, 0.6, 0.5, 1.5, 2.5, 2000.0, 2000.0, 2000.0, 0.05, 0.1, 0.35],    # exp(-10) at the antipodes: not small
    "closed": [1.0, 1.0, 1.5, 1.5, 1.5, 1500.0, 1200.0, 1000.0, 0.02, 0.02, -0.6],
    "short": [1.3, 0.6, 3.5, 3.5, 3.5, 100.0, 100.0, 100.0, 0.05, 0.1, 0.35],      # scaled lags up to 20 015 sqrt(7) / 100 = 530
}

# the first sites of each process.  Inside one process two spellings of one place are a pair at ~1e-12 km without a nugget
# between them: the smallest eigenvalue of Sigma is then the nugget, which every set of GLOBE_PARAMS has.
SPECIAL_0 = [(90.0, 0.0), (-90.0, 0.0), (10.0, 180.0), (10.0, -180.0), (0.0, 0.0), (0.0, 180.0), (45.0, -179.999)]
SPECIAL_1 = [(90.0, 120.0), (-90.0, -45.0), (10.0, 180.0), (0.0, -180.0), (0.0, 0.0), (45.0, -179.999 + 360.0)]
N0, N1, N_CO = 330, 290, 40


def sphere_sites(rng, n):
    """n sites [lat, lon] uniform on the sphere: z uniform, lon uniform"""
    return np.column_stack([np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)])


def _globe():
    rng = np.random.default_rng(20250)
    c0, c1 = sphere_sites(rng, N0), sphere_sites(rng, N1)
    c0[:len(SPECIAL_0)] = SPECIAL_0
    c1[:len(SPECIAL_1)] = SPECIAL_1
    c1[50:50 + N_CO] = c0[100:100 + N_CO]              # the co-located block: h == 0 across the processes
    sig = SET_A[:2]
    values = [sig[0] * rng.standard_normal(N0), sig[1] * rng.standard_normal(N1)]
    return dict(coords=[c0, c1], values=values, metric=HAV)


GLOBE = _globe()
PRED_DATUM = 200                                       # the datum of process 0 that globe_pred_sites repeats


def _clusters():
    rng = np.random.default_rng(20251)
    n = 2100
    a = np.column_stack([rng.uniform(25.0, 50.0, n), rng.uniform(-120.0, -70.0, n)])
    b = np.column_stack([rng.uniform(-40.0, -15.0, n), rng.uniform(115.0, 150.0, n)])
    values = [SET_A[0] * rng.standard_normal(n), SET_A[1] * rng.standard_normal(n)]
    return dict(coords=[a, b], values=values, metric=HAV, params=SET_A, box_b=((-40.0, -15.0), (115.0, 150.0)))


CLUSTERS = _clusters()


def globe_pred_sites(rng, m):
    """m prediction sites on the whole sphere.  The first seven are always: both poles, a site within 1 km of the antimeridian
    on either side, a datum of process 0 verbatim, the same datum with lon -+ 360, and a site near a pole."""
    assert m >= 7
    pc = sphere_sites(rng, m)
    d = GLOBE["coords"][0][PRED_DATUM]
    pc[0] = (90.0, 37.0)
    pc[1] = (-90.0, 0.0)
    pc[2] = (20.0, 179.995)                            # 0.005 degrees of longitude: at most 0.56 km
    pc[3] = (-33.0, -179.995)
    pc[4] = d
    pc[5] = (d[0], d[1] - 360.0 if d[1] > 0 else d[1] + 360.0)
    pc[6] = (89.99, 10.0)
    return pc


def around(centre, dist_km, bearing):
    """sites [lat, lon] at the great-circle distance dist_km from centre = [lat, lon] under the initial bearing (radians from
    north, clockwise), through the centre's own east / north frame, so that a pole is a centre like any other: its longitude
    says where bearing 0 points.  The longitude is the centre's plus the offset in (-180, 180], NOT brought back into
    [-180, 180]: the device has to be periodic in it."""
    lat, lon = np.radians(float(centre[0])), float(centre[1])
    dl, th = np.asarray(dist_km, dtype=np.float64) / orc.EARTH_RADIUS, np.asarray(bearing, dtype=np.float64)
    x = np.cos(dl) * np.cos(lat) - np.sin(dl) * np.cos(th) * np.sin(lat)         # in the frame turned by the centre's longitude
    y = np.sin(dl) * np.sin(th)
    z = np.cos(dl) * np.sin(lat) + np.sin(dl) * np.cos(th) * np.cos(lat)
    return np.column_stack([np.degrees(np.arctan2(z, np.hypot(x, y))), lon + np.degrees(np.arctan2(y, x))])


BLOCK_SIZES = (64, 300, 3, 17, 17, 1, 64, 33)
BLOCK_REACH_KM = (9000.0, 800.0, 800.0, 800.0, 800.0, 0.0, 800.0, 15000.0)
BLOCK_CANCELLING = 4                                   # its weights sum to zero
BLOCK_HEMISPHERES = (0, 7)                             # member pairs on opposite sides of the globe


def globe_blocks(rng):
    """(centres (8, 2), pc, lab, w): eight blocks centred on the first eight rows of globe_pred_sites -- both poles, either side
    of the antimeridian, a datum of process 0, its lon -+ 360 copy, the site near the pole, one free -- with BLOCK_SIZES members
    uniform in distance and bearing within BLOCK_REACH_KM of the centre (gs.around: longitudes unnormalised), the members of
    all blocks interleaved.  The weights are positive and sum to 1, except those of block 4, which have their mean taken off: a
    contrast, whose sigma_BB is small against the variance.  No two members of a block are closer than 1e-6 km, so the nugget
    rule h == 0 between members does not rest on the last bit of anybody's distance (block 5 is its centre alone)."""
    centres = globe_pred_sites(rng, 8)
    pc, lab, w = [], [], []
    for b, (q, reach) in enumerate(zip(BLOCK_SIZES, BLOCK_REACH_KM)):
        x = around(centres[b], reach * rng.random(q), rng.uniform(0.0, 2.0 * np.pi, q)) if reach > 0 else np.repeat(centres[b][None], q, 0)
        d = orc.haversine_km(x, x)
        assert q == 1 or d[np.triu_indices(q, k=1)].min() > 1e-6, b
        wb = rng.uniform(0.2, 2.0, q)
        wb = wb / wb.sum()
        if b == BLOCK_CANCELLING:
            wb = wb - wb.mean()
        pc.append(x)
        lab.append(np.full(q, b))
        w.append(wb)
    pc, lab, w = np.vstack(pc), np.concatenate(lab), np.concatenate(w)
    perm = rng.permutation(len(lab))
    return centres, pc[perm], lab[perm], w[perm]


def lon_folds(coords):
    """six folds by longitude, floor(((lon + 210) mod 360) / 60): fold 0 is [150, 180] and [-180, -150), across the antimeridian"""
    lon = np.asarray(coords, dtype=np.float64)[:, 1]
    return np.floor(np.mod(lon + 210.0, 360.0) / 60.0).astype(np.int32)


def sim_sites(rng, m, i):
    """globe_pred_sites(rng, m) without the rows within 1e-6 km of a datum of process i: a simulation site on a noise-free datum
    is singular by the rule of ck_simulate_local.  The sites either side of the antimeridian and (89.99, 10) stay."""
    pc = globe_pred_sites(rng, m)
    return pc[orc.haversine_km(pc, GLOBE["coords"][i]).min(axis=1) > 1e-6]


# ---- the cases of tests/test_gpu_global_sites_newer.py, pinned without a GPU in tests/test_global_sites_host.py ------------------
BLOCK_SEED = 300
BLOCK_REACHES = (3000.0, 12000.0)                      # every neighbourhood in the LDS class | in the tiled class
SIM_SITE_SEED, SIM_RANK_SEED, SIM_M = 101, 102, 64
SIM_CASES = ((12000.0, (12, 12)), (3000.0, (0, 0)))    # (max_dist, caps)
SIM_DATA_NOISE = 0.01                                  # on every datum, where sites sit on data
# (max_dist, caps, buffer per process or None, lon_folds labels or none): the first five are the fold cases, the last two the
# buffer-only calls that show what the buffer alone does to the special sites
CV_CASES = ((3000.0, (0, 0), (500.0, 500.0), True), (12000.0, (40, 25), (500.0, None), True), (12000.0, (40, 25), (0.0, 0.0), True),
            (3000.0, (0, 0), None, True), (12000.0, (0, 0), (500.0, 500.0), True),
            (3000.0, (0, 0), (0.0, 0.0), False), (3000.0, (0, 0), (500.0, 500.0), False))
CV_CULL_REACHES = (1500.0, 12000.0, 19500.0)
CV_CULL_BUFFER = (300.0, 300.0)
VECCHIA_RANK_SEED, VECCHIA_REACH, VECCHIA_CAPS = 3, 12000.0, (16, 16)


def culling_sites():
    """the 3 000 + 2 600 sites of test_radius_search_culling_on_the_globe: 12 + 11 chunks of 256"""
    rng = np.random.default_rng(4)
    coords = [sphere_sites(rng, 3000), sphere_sites(rng, 2600)]
    coords[0][:len(SPECIAL_0)] = SPECIAL_0
    coords[1][:len(SPECIAL_1)] = SPECIAL_1
    return coords


def vario_sites(n, seed):
    """n whole-sphere sites with values for the variogram tests: the poles and (0, +-180) included"""
    rng = np.random.default_rng(seed)
    c = sphere_sites(rng, n)
    c[:4] = [(90.0, 0.0), (-90.0, 0.0), (0.0, 180.0), (0.0, -180.0)]
    return c, rng.standard_normal(n)


def antipodes(n=32, seed=20252):
    """n sites, their exact antipodes (-lat, lon -+ 180) and their lon -+ 360 copies, as two processes: process 0 holds the
    sites and the antipodes, process 1 the copies and the sites once more verbatim.  All of lat, lon and their images are
    exactly representable (multiples of 1/8 degree), so that -lat and lon -+ 180 are the antipode's own coordinates."""
    rng = np.random.default_rng(seed)
    lat = rng.integers(-8 * 80, 8 * 80, n) / 8.0
    lon = rng.integers(-8 * 179, 8 * 179, n) / 8.0
    lat[0], lon[0] = 0.0, 0.0                          # (0, 0) / (0, 180)
    lat[1], lon[1] = 90.0, 0.0                         # the poles are each other's antipode
    base = np.column_stack([lat, lon])
    anti = np.column_stack([-lat, np.where(lon > 0, lon - 180.0, lon + 180.0)])
    copy = np.column_stack([lat, np.where(lon > 0, lon - 360.0, lon + 360.0)])
    return dict(base=base, anti=anti, copy=copy, coords=[np.vstack([base, anti]), np.vstack([copy, base])])


# ---- what the haversine formula itself can hold near the antipode --------------------------------------------------------
def haversine_rounding_km(D, ulps=8):
    """How far `ulps` ulp (2 ** -52 relative) of rounding error in r = sin^2(dlat / 2) + cos cos sin^2(dlon / 2) move the
    distance d = 2 R asin(sqrt(r)), for distances D in km.  r is built from four sin / cos values (up to 1 ulp each), their
    squares and products and one sum: up to about 8 half-ulps per implementation, 8 ulp between two of them.  The move is
    R * ulps * 2 ** -52 * tan(d / 2R) until asin's branch point takes over: 5e-4 km at the exact antipode (r = 1), where one
    rounding of r alone is 1.9e-4 km.  Evaluated through atan2, which has no branch point there."""
    a = np.asarray(D, dtype=np.float64) / (2.0 * orc.EARTH_RADIUS)
    e = ulps * 2.0 ** -52
    s, c = np.sin(a), np.cos(a)
    return 2.0 * orc.EARTH_RADIUS * (a - np.arctan2(s * np.sqrt(1.0 - e), np.sqrt(c * c + e * s * s)))


def joint_cov_tolerance(p, coords, S, rtol=5e-13, ulps=8):
    """Entry-wise bound for comparing a haversine Sigma with orc.joint_cov: the covariance tolerance of the neighbouring tests
    (test_cov_dense_blocks: rtol 5e-13) plus what the distance formula's own rounding moves the ORACLE's entry by,
    |C(d - dd) - C(d)| with dd = haversine_rounding_km(d).  The second term is below 1e-13 |C| for continental pairs under
    every parameter set; it reaches 3e-13 |C| a quarter of the way round at len_scale = 100, and 1.5e-7 |C| at the exact
    antipode at len_scale = 2000 -- tests/test_global_sites_host.py measures the oracle moving by that much under a 1-ulp nudge
    of its inputs."""
    allc = np.vstack(coords)
    n0 = len(coords[0])
    D = orc.haversine_km(allc, allc)
    d_lo = np.where(D > 0, np.maximum(D - haversine_rounding_km(D, ulps), np.nextafter(0.0, 1.0)), 0.0)
    sl = [slice(0, n0), slice(n0, None)]
    moved = np.empty_like(S)
    for i in range(2):
        for j in range(2):
            d = d_lo[sl[i], sl[j]]
            moved[sl[i], sl[j]] = orc.covariance(p, i, d) if i == j else orc.cross_covariance(p, i, j, d)
    return rtol * np.abs(S) + np.abs(moved - S)


# ---- chord space: the table kernels' own coordinate ---------------------------------------------------------------------------
def unit_vectors(coords, metric=HAV):
    """(n, 3): the unit vector of every [lat, lon] site (csrc/ck_cov.hip: prep_site); Euclidean: (x, y, 0)"""
    c = np.atleast_2d(np.asarray(coords, dtype=np.float64))
    if metric == EUC:
        return np.column_stack([c[:, 0], c[:, 1], np.zeros(len(c))])
    lat, lon = np.radians(c[:, 0]), np.radians(c[:, 1])
    return np.column_stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


def chord_q(A, B, metric=HAV):
    """(a, b): the squared chord q = |u_i - u_j|^2 of every pair"""
    d = unit_vectors(A, metric)[:, None, :] - unit_vectors(B, metric)[None, :, :]
    return np.einsum("ijk,ijk->ij", d, d)


def strictly_outside(q, q_lo, q_hi, margin=1e-12):
    """mask of the pairs outside the table [q_lo, q_hi) by more than a relative `margin`: rounding of q (the device's sin / cos
    differ from numpy's in the last bit) cannot move such a pair across an end"""
    return (q < q_lo * (1.0 - margin)) | (q > q_hi * (1.0 + margin))


def count_outside_sigma(coords, tables, metric=HAV):
    """pairs of the lower triangle of Sigma (diagonal included) strictly outside their block's table; tables[b] = the dict of
    Handle.table_info(b) for b = i + j"""
    n_out = 0
    for i in range(len(coords)):
        for j in range(i + 1):
            t = tables[i + j]
            out = strictly_outside(chord_q(coords[i], coords[j], metric), t["q_lo"], t["q_hi"])
            n_out += int(np.count_nonzero(np.tril(out) if i == j else out))
    return n_out


def count_outside_aux(coords, pcoords, i_pred, tables, metric=HAV):
    """pairs (prediction site, datum) strictly outside the table of their block"""
    return sum(int(np.count_nonzero(strictly_outside(chord_q(pcoords, coords[j], metric), tables[i_pred + j]["q_lo"],
                                                      tables[i_pred + j]["q_hi"]))) for j in range(len(coords)))
