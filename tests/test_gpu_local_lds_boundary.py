"""GPU tests of the local solver's shared device steps (csrc/ck_local.hip: lp_compact, lp_triangle, lp_cz_rows, lp_noise, lp_chol,
lp_dots) at the sizes around the LDS limit of 64 neighbours, where the kernels that compose them hand over to one another.

With max_dist beyond the domain and no cv every neighbourhood is the whole data set, so (n0, n1) chooses k = n0 + n1 exactly
(a process with n = 0 has three sites on the other side of the globe, beyond max_dist: data, but no neighbour):
  (1, 0), (0, 1), (1, 1)                         the Cholesky loop without trailing columns, a process without neighbours
  (63, 0), (32, 32), (64, 0)                     a full LDS system, one process or two
  (33, 32), (40, 26)                             the first sizes that leave it: through local_tile_min = 0 (tiled path) and 10**6
                                                 (the slab kernel; the universal form has none and stays tiled)
each with the noise off and on, for the simple and the universal predictor.  Seeded random sites (the generator of
tests/test_gpu_local_universal.py), so no system is singular.  References and tolerances are those files' own: the simple
predictor against oracle.cokrige_oracle.local_predict (with noise: the per-site chain of tests/test_gpu_noise_local.py on
Sigma + diag(s d)), the universal one against tests/test_gpu_local_universal.py's Reference (with noise: the same on its
diagonal blocks); rtol 1e-8, atol 1e-10 on pred and pred_err^2.

Cases other files pin already are left out here: the simple predictor without noise at (1, 1), (32, 32), (33, 32) with
local_tile_min = 0 (tests/test_gpu_local.py: test_local_system_sizes_around_the_padding_boundaries), the universal one with a
constant trend at (32, 32) and at (33, 32) on its default route, without noise (tests/test_gpu_local_universal.py:
test_padding_boundaries) and with it (tests/test_gpu_noise_local.py: test_padding_sizes, which also has the simple predictor
with noise at (32, 32)).

The Vecchia value and gradient on 65 data under full conditioning: the conditioning sets run through every size 0 .. 64 in one
call.  The gradient without noise against tests/vecchia_grad_ref.py at this size is tests/test_gpu_vecchia_grad.py:
test_full_conditioning_is_the_dense_gradient; here the value against tests/vecchia_ref.py, the gradient with noise, and the
fact the shared steps make structural: the gradient call's means and v . v are the value call's, bit for bit.  The C API
returns them from the gradient call as out3 only -- (l, sum log s_t^2, sum e_t^2 / s_t^2), summed by the same terms kernels from
the means and v . v the gradient kernel wrote -- so the three totals are what is compared with array_equal."""
import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import test_gpu_local_universal as tlu
from tests import test_gpu_noise_local as tnl
from tests import test_gpu_vecchia as tgv
from tests import test_gpu_vecchia_grad as tgg
from tests import vecchia_grad_ref as vgr

pytestmark = pytest.mark.gpu

HAV = 0
RTOL, ATOL = 1e-8, 1e-10
SCALE = (1.5, 0.7)
SIZES = [(1, 0), (0, 1), (1, 1), (63, 0), (32, 32), (64, 0), (33, 32), (40, 26)]
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def data():
    """70 + 40 seeded random sites, noise variances as tests/test_gpu_noise_local.py draws them, 7 prediction sites"""
    if "data" not in _cache:
        p, coords, values = tlu.make_data(41, tlu.BIV, HAV, n0=70, n1=40)
        rng = np.random.default_rng(43)
        d = [1e-2 * p.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, n) for k, n in enumerate((70, 40))]
        _cache["data"] = (p, coords, values, d, tlu.pred_sites(np.random.default_rng(5), HAV, 7))
    return _cache["data"]


def cases(pinned_elsewhere):
    out = []
    for n0, n1 in SIZES:
        routes = [None] if n0 + n1 <= 64 else [0, 10 ** 6]
        for tile_min in routes:
            for noise in (False, True):
                if (n0, n1, tile_min, noise) not in pinned_elsewhere:
                    out.append(pytest.param(n0, n1, tile_min, noise, id=f"{n0}+{n1}-tile{tile_min}-{'noise' if noise else 'plain'}"))
    return out


# tests/test_gpu_local.py: test_local_system_sizes_around_the_padding_boundaries; tests/test_gpu_noise_local.py: test_padding_sizes
SIMPLE_PINNED = [(1, 1, None, False), (32, 32, None, False), (33, 32, 0, False), (32, 32, None, True), (33, 32, 0, True)]
# tests/test_gpu_local_universal.py: test_padding_boundaries; tests/test_gpu_noise_local.py: test_padding_sizes (the universal
# form's default route beyond 64 is the one local_tile_min = 10**6 leaves it on)
UNIVERSAL_PINNED = [(32, 32, None, False), (32, 32, None, True), (33, 32, 10 ** 6, False), (33, 32, 10 ** 6, True)]


MAX_DIST = 8000.0   # km: beyond the prediction sites' reach over the data (< 5 500 km), short of FAR (> 12 000 km)
FAR = (np.array([[-40.0, 100.0], [-41.0, 101.0], [-42.0, 99.0]]), np.array([0.1, -0.2, 0.3]), np.array([0.01, 0.02, 0.0]))


def subset(n0, n1):
    p, coords, values, d, pc = data()
    take = lambda x, far: [x[k][:n] if n else far for k, n in enumerate((n0, n1))]   # noqa: E731
    return p, take(coords, FAR[0]), take(values, FAR[1]), take(d, FAR[2]), pc


def targets(n0, n1):
    """the processes the universal form can predict: those with neighbours (rule 3)"""
    return [i for i, n in enumerate((n0, n1)) if n > 0]


def handle(native, p, coords, values, d, noise, tile_min):
    h = tlu.handle(native, p, coords, values, HAV)
    if tile_min is not None:
        h.set_option("local_tile_min", tile_min)
    if noise:
        for k in range(2):
            h.set_noise(k, d[k], SCALE[k])
    return h


def close(pred, err, rp, rvar, label):
    print(f"{label}: max |d pred| {np.max(np.abs(pred - rp)):.2e} max |d var| {np.max(np.abs(err ** 2 - rvar)):.2e}")
    np.testing.assert_allclose(pred, rp, rtol=RTOL, atol=ATOL, err_msg=label)
    np.testing.assert_allclose(err ** 2, rvar, rtol=RTOL, atol=ATOL, err_msg=label)


@pytest.mark.parametrize("n0,n1,tile_min,noise", cases(SIMPLE_PINNED))
def test_simple_predictor(native, n0, n1, tile_min, noise):
    p, coords, values, d, pc = subset(n0, n1)
    h = handle(native, p, coords, values, d, noise, tile_min)
    for i in (0, 1):   # also the process that has no neighbour of its own: (0, 1) with i = 0
        pred, err, info = h.predict_local(i, pc, max_dist=MAX_DIST)
        assert info["k_max"] == n0 + n1 and info["n_not_pd"] == 0 and info["n_empty"] == 0, info
        if noise:
            Sn = orc.joint_cov(p, coords, HAV) + np.diag(np.concatenate([SCALE[0] * d[0], SCALE[1] * d[1]]))
            rp, rvar, kk, st = tnl.reference(p, coords, values, Sn, pc, i, HAV, MAX_DIST)
            assert np.all(st == 0) and np.all(kk == n0 + n1)
        else:
            rp, re = orc.local_predict(p, coords, values, pc, i, HAV, MAX_DIST)[:2]
            rvar = re ** 2
        close(pred, err, rp, np.maximum(rvar, 0.0), f"simple n0={n0} n1={n1} i={i} tile_min={tile_min} noise={noise}")
    h.close()


@pytest.mark.parametrize("n0,n1,tile_min,noise", cases(UNIVERSAL_PINNED))
def test_universal_predictor(native, n0, n1, tile_min, noise):
    """a constant per process; the column of a process without neighbours is dropped (rule 3 of include/cokrige.h)"""
    p, coords, values, d, pc = subset(n0, n1)
    h = handle(native, p, coords, values, d, noise, tile_min)
    Fs = [np.ones((len(c), 1)) for c in coords]
    for k in range(2):
        h.set_trend(k, Fs[k])
    ref = tlu.Reference(p, coords, values, HAV, Fs)
    if noise:
        for k in range(2):
            ref.Sigma[k, k] = ref.Sigma[k, k] + np.diag(SCALE[k] * d[k])
    for i in targets(n0, n1):
        F0 = np.ones((len(pc), 1))
        pred, err, info = h.predict_local_universal(i, pc, F0, max_dist=MAX_DIST, want_beta=True)
        want = ref(pc, i, MAX_DIST, F0)
        assert info["k_max"] == n0 + n1 and info["n_rank_def"] == 0 and np.all(want["status"] == tlu.OK), info
        agree = tlu.compare(pred, err, info, want, beta=info["beta"])
        assert agree.any()
    h.close()


@pytest.mark.parametrize("noise", [False, True])
def test_vecchia_value_and_gradient_through_every_set_size(native, noise):
    from sif_xco2_cokriging_amd import vecchia
    pb = tgg.small_problem("GEN")                                     # 33 + 32 data
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 1)
    d = None
    if noise:
        rng = np.random.default_rng(22)
        d = [rng.uniform(0.01, 0.05, 33), rng.uniform(0.01, 0.05, 32)]
    ref, want = tgg.reference(pb, 2.0, (0, 0), ranks=ranks, noise_d=d, scales=tgg.SCALES, key=("lds boundary", noise))
    assert np.array_equal(np.sort(ref["count"].sum(axis=1)), np.arange(65))   # every set size 0 .. 64, once
    h = tgg.make_handle(native, pb["params"], tgg.EUC, pb["coords"], pb["values"])
    if noise:
        for k in range(2):
            h.set_noise(k, d[k], tgg.SCALES[k])
    out3, info, st = h.loglik_vecchia(ranks, 2.0, terms=True)
    tgv.check_against(ref, out3, info, st, f"65 data, noise={noise}")
    g3, grad, ginfo, gst = h.loglik_vecchia_grad(ranks, 2.0, scores=True)
    h.close()
    assert ginfo == 0 and gst["k_max"] == 64 and gst["n_empty"] == 1
    assert np.array_equal(g3, out3), (g3, out3)                       # the same means and v . v, bit for bit
    if noise:                                                         # (without: test_full_conditioning_is_the_dense_gradient)
        tgg.check_scores(grad, gst["score"], want, np.arange(13), "65 data with noise")
        assert vgr.measure(grad, want["grad13"]).max() < tgg.TOL
