"""GPU tests of the Vecchia entry points -- ck_loglik_vecchia, _grad, _fisher, _trend, _trend_grad and ck_debug_vecchia_trend -- at
the sizes their kernels index by: the treatment tests/test_gpu_newer_entry_edge_sizes.py gives the dense entry points.  The
fixtures and references are in tests/vecchia_edge_ref.py; tests/test_vecchia_edge_host.py checks on the host that no comparison
here leaves a datum out (cap gaps above 1e-9) and that no bound is vacuous.

1. The ladder: prefixes of half_colocated_sites(600), SET_B_UNIT, caps (4, 4), max_dist 0.5, and one process alone.
     (1, 1) (2, 1) (7, 9) (8, 8) (9, 8) (8, 9)     processes below, on and one past k_vecchia_info's run of 8 (row0 = ceil(n0 / 8))
     (64, 64) (63, 65) (65, 63) (64, 1) (1, 64)    the boundary ga >= n0p on a 64-row strip with and without a gap, one-site processes
     (128, 129) (255, 1)                           N = 257 and N = 256: the 256-term trees with a tail of one and without a tail
     (256, 256) (257, 255) (300, 213)              N = 512 exactly (two ways), N = 513
     one process: N = 1, 8, 9, 256, 257
   Value, gradient and scores, information, trend (profile, REML and the per-datum solves) on every rung against the numpy loops
   of tests/vecchia_ref.py, vecchia_grad_ref.py, vecchia_info_ref.py, vecchia_trend_ref.py, through the checks and at the bounds
   of the four existing GPU modules (check_against, check_scores, check_matrix / check_shape, check_case).
2. The sums held to their own terms: a call's totals against math.fsum of that call's per-datum outputs within 64 u sum |x_t|
   (for the Gram matrix recovered through inv(Cov(beta)) plus 1e-12 |G_ab|) -- on every rung and on 3a.
3a. N = 35 000 + 35 001: 274 partial sums, the second trip of the loops of k_vecchia_sum, k_vecchia_grad_sum and
   k_vecchia_info_sum (the Gram matrix's tree); per datum against a reference on a sample of 256 data.
3b. N = 1 030 + 1 029: 258 rows of k_vecchia_info, the second workgroup of k_vecchia_info_part.
4. Trend width: p = 8 + 8 at k_max = 64 (the largest LDS request, 153 of the 156 triangle threads), a process without a trend,
   unequal blocks, p = 16 under full conditioning against dense GLS.
5. One handle across settings: caps, noise and trend widths set and cleared in turn, every output equal bit for bit to a fresh
   handle's.  (ck_set_data refuses a laid-out handle -- asserted -- so the data sizes change with the handle.)

Wall time on an MI355X.  3a: the six calls at N = 70 001 take 0.12 s together (the select pass 11 ms of each call's 18 - 30 ms);
each of its four tests 0.7 s or less, the sampled numpy reference included.  3b: the call 1.4 ms, the test 4.4 s (the numpy
reference at N = 2 059).  Every other test is below 0.5 s.

Largest deviations seen on an MI355X over all cases of this file (the tests print them per case):
  value, per datum            |dmean| 1.3e-13, relative dvar 6.6e-14 (bounds rtol 1e-8, atol 1e-10); the tall sample the same
  gradient                    the sum 2.2e-8, a datum's score 5.3e-8 in the project's gradient measure (bound 1e-6)
  information                 exact 1.3e-14, nu 5.9e-9, length scale 9.7e-9 -- 1.07 x the reference's own floor on every rung
                              (the bound is 10 floors: the device's analytic derivative shows the reference's error, not its own)
  trend, per datum            |dmu| 1.3e-13, relative ds2 4.1e-14, |dg| 1.2e-14
  sums against their terms    value 2.0, gradient 1.8, gradient of the profiled value 1.4, sum log s^2 of the trend call 1.8, all in
                              units of u sum |x_t| (bound 64); the recovered Gram matrix 0.05 of its bound
  one handle across settings  every output bit for bit a fresh handle's
No bound was fitted to these numbers: each was set before the first run."""
import time

import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import test_gpu_vecchia as tgv
from tests import test_gpu_vecchia_grad as tgg
from tests import test_gpu_vecchia_info as tgi
from tests import test_gpu_vecchia_trend as tgt
from tests import vecchia_edge_ref as ve
from tests import vecchia_grad_ref as vgr
from tests import vecchia_trend_ref as vtr
from tests.test_gpu_newer_entry_edge_sizes import bits
from tests.test_gpu_vecchia import native  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

EUC = ve.EUC
RTOL, ATOL = tgv.RTOL, tgv.ATOL
LOG2PI = float(np.log(2.0 * np.pi))


def open_handle(native, pb, F=None):
    h = tgt.make_handle(native, pb["params"], pb["metric"], pb["coords"], pb["values"], F)
    h.set_local_neighbours(*ve.handle_caps(pb))
    return h


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sums, held to their own terms
# ---------------------------------------------------------------------------------------------------------------------
def check_sums(got, sums, label, what):
    """got[i] against (exact, bound)[i]; prints the largest deviation in units of u sum |x_t| (the bound is SUM_FACTOR of them)"""
    worst = 0.0
    for i, (g, (exact, bound)) in enumerate(zip(got, sums)):
        dev = abs(g - exact)
        if bound > 0:
            worst = max(worst, ve.SUM_FACTOR * dev / bound)
        assert dev <= bound, (label, what, i, g, exact, dev, bound)
    print(f"{label}: {what} against fsum of its own terms, largest deviation {worst:.2f} u sum|x| (bound {ve.SUM_FACTOR:.0f})")


def check_value_sums(out3, z, st, label):
    check_sums(out3[1:], ve.value_sums(z, st["mean"], st["var"]), label, "sum log s^2, sum e^2 / s^2")
    total = -0.5 * (len(z) * LOG2PI + out3[1] + out3[2])
    assert abs(out3[0] - total) <= 8 * ve.U * (len(z) * LOG2PI + abs(out3[1]) + abs(out3[2])), (label, out3, total)


def check_gram(out5, beta, cov, z, X, prior_own, dbg, label):
    """G recovered from the call against the Gram matrix of the rows built from debug_vecchia_trend's (mu, vv, g)"""
    mu, vv, g = dbg
    Gr, B = ve.gram_of_rows(ve.trend_rows(z, X, prior_own, mu, vv, g))
    x = ve.gram_excess(ve.recovered_gram(out5, beta, cov), Gr, B)
    print(f"{label}: recovered G against its own rows, largest |dG| / (64 u sum|r r| + 1e-12 |G|) = {x:.3f}")
    assert x <= 1.0, (label, x)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the ladder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ve.LADDER)
def test_value_on_the_ladder(native, label):
    pb, ref = ve.rung(label), ve.value_reference(label)
    assert ref["gap"].min() > 1e-9 and ref["info"] == 0
    h = open_handle(native, pb)
    out3, info, st = h.loglik_vecchia(pb["ranks"], pb["max_dist"], terms=True)
    h.close()
    tgv.check_against(ref, out3, info, st, label)
    check_value_sums(out3, ref["z"], st, label)


@pytest.mark.parametrize("label", ve.LADDER)
def test_gradient_on_the_ladder(native, label):
    pb, ref, want = ve.rung(label), ve.value_reference(label), ve.grad_reference(label)
    npar = ve.npar_of(pb)
    h = open_handle(native, pb)
    value = h.loglik_vecchia(pb["ranks"], pb["max_dist"])
    out3, grad, info, st = h.loglik_vecchia_grad(pb["ranks"], pb["max_dist"], scores=True)
    h.close()
    assert info == 0 and np.array_equal(out3, value[0])
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"])
    tgg.check_scores(grad, st["score"], want, np.arange(npar), label)
    assert np.all(grad[npar:] == 0.0) and np.all(st["score"][:, npar:] == 0.0)
    check_sums(grad, ve.score_sums(st["score"]), label, "the gradient")


@pytest.mark.parametrize("label", ve.LADDER)
def test_information_on_the_ladder(native, label):
    pb, sets, ref = ve.rung(label), ve.value_reference(label), ve.info_reference(label)
    h = open_handle(native, pb)
    I, info, st = h.loglik_vecchia_fisher(pb["ranks"], pb["max_dist"])
    h.close()
    assert info == 0
    assert (st["n_empty"], st["k_max"], st["n_capped"]) == (sets["n_empty"], sets["k_max"], sets["n_capped"])
    tgi.check_matrix(I, ref, label, npar=ve.npar_of(pb), tol=ve.info_tol(label))
    tgi.check_shape(I, ve.info_live(ref))


@pytest.mark.parametrize("label", ve.LADDER)
def test_trend_on_the_ladder(native, label):
    pb, tr = ve.rung(label), ve.trend_reference(label)
    assert tr["gap"].min() > 1e-9 and np.linalg.cond(tr["A"]) < 1e3
    h = open_handle(native, pb, tr["F"])
    out5, beta, cov, st = tgt.check_case(h, pb, tr, pb["max_dist"], label)
    assert h.vecchia_trend_timings()["p"] == tr["p"]
    dbg = h.debug_vecchia_trend(pb["ranks"], pb["max_dist"])
    h.close()
    check_gram(out5, beta, cov, tr["z"], tr["X"], tr["prior"] + tr["own"], dbg, label)
    check_sums(out5[1:2], ve.value_sums(tr["z"], tr["mean"], st["var"])[:1], label, "sum log s^2 of the trend call")


def test_a_process_of_one_site_takes_no_linear_design(native):
    pb = ve.rung("1+1")
    with pytest.raises(ValueError, match="process 0 has 1 data sites for 3 regressors"):
        ve.trend_design(pb, ("linear", "constant"))
    h = open_handle(native, pb)
    with pytest.raises(native.NativeError, match="process 0 has 1 data sites for 3 regressors"):
        h.set_trend(0, np.ones((1, 3)))
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3a. the tall case: the second trip of every tree
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tall(native):
    """every call of the tall case on one handle, once"""
    pb = ve.tall_problem()
    ranks, md = pb["ranks"], pb["max_dist"]
    t0 = time.perf_counter()
    h = open_handle(native, pb)
    r = dict(pb=pb)
    r["value"] = h.loglik_vecchia(ranks, md, terms=True)
    r["value_timings"] = h.vecchia_timings()
    r["grad"] = h.loglik_vecchia_grad(ranks, md, scores=True)
    r["grad_timings"] = h.vecchia_grad_timings()
    r["X"], F = ve.constant_design(pb)
    for k in range(2):
        h.set_trend(k, F[k])
    r["debug"] = h.debug_vecchia_trend(ranks, md)
    r["trend"] = h.loglik_vecchia_trend(ranks, md, terms=True)
    r["trend_timings"] = h.vecchia_trend_timings()
    r["trend_grad"] = h.loglik_vecchia_trend_grad(ranks, md, scores=True)
    r["trend_grad_timings"] = h.vecchia_trend_timings()
    h.close()
    r["device_s"] = time.perf_counter() - t0
    print(f"tall case, N = {len(ranks)}: the six calls took {r['device_s']:.2f} s; vecchia_timings {r['value_timings']}; "
          f"gradient {r['grad_timings']}; trend {r['trend_timings']}; trend gradient {r['trend_grad_timings']}")
    p = orc.Params.from_flat(pb["params"])
    r["prior"] = np.concatenate([np.full(len(c), orc.covariance(p, k, np.zeros(1))[0]) for k, c in enumerate(pb["coords"])])
    r["z"] = np.concatenate(pb["values"])
    return r


def tall_kept(ref):
    """the sampled data whose sets numpy and the device must agree on"""
    ok = ref["gap"] >= 1e-9
    assert np.count_nonzero(~ok) <= 2
    return ok


def test_tall_value(tall):
    ref, N = ve.tall_reference(), len(tall["z"])
    ok, s = tall_kept(ref), ve.tall_reference()["index"]
    out3, info, st = tall["value"]
    assert info == 0 and np.all(np.isfinite(out3))
    assert -(-N // 256) > 256                                       # the sum kernels' threads 0 .. 17 take two partial sums
    assert np.array_equal(st["count"][s][ok], ref["count"][ok])
    print(f"tall value: max |dmean| {np.max(np.abs(st['mean'][s][ok] - ref['mean'][ok])):.2e}, max rel dvar "
          f"{np.max(np.abs(st['var'][s][ok] - ref['var'][ok]) / ref['var'][ok]):.2e} on {np.count_nonzero(ok)} sampled data")
    np.testing.assert_allclose(st["mean"][s][ok], ref["mean"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"][s][ok], ref["var"][ok], rtol=RTOL, atol=ATOL)
    check_value_sums(out3, tall["z"], st, "tall")
    ktot = st["count"].sum(axis=1)
    assert ktot.max() == st["k_max"] and np.count_nonzero(ktot == 0) == st["n_empty"]
    assert st["k_max"] >= ref["count"][ok].sum(axis=1).max() and st["k_max"] <= 6
    assert np.count_nonzero(ref["capped"][ok]) <= st["n_capped"] <= N
    assert np.all(st["count"][s][ok][ref["capped"][ok]].max(axis=1) == 3)   # a capped datum of the sample holds a full process
    tv = tall["value_timings"]
    assert tv["n_lds"] == N and tv["n_tiled"] == 0 and tv["select_ms"] > 0


def test_tall_gradient(tall):
    ref = ve.tall_reference()
    ok, s = tall_kept(ref), ref["index"]
    out3, grad, info, st = tall["grad"]
    assert info == 0 and np.array_equal(out3, tall["value"][0])
    es = vgr.measure(st["score"][s][ok][:, :11], ref["score"][ok][:, :11])
    print(f"tall gradient: score measure max {es.max():.2e} on {np.count_nonzero(ok)} sampled data")
    assert es.max() < tgg.TOL
    assert np.all(grad[11:] == 0.0) and np.all(st["score"][:, 11:] == 0.0)
    check_sums(grad, ve.score_sums(st["score"]), "tall", "the gradient")


def test_tall_trend(tall):
    ref = ve.tall_reference()
    ok, s = tall_kept(ref), ref["index"]
    mu, vv, g = tall["debug"]
    out5, beta, cov, info, st = tall["trend"]
    assert info == 0 and np.all(np.isfinite(out5))
    s2 = tall["prior"] - vv
    print(f"tall trend: max |dmu| {np.max(np.abs(mu[s][ok] - ref['mean'][ok])):.2e}, max |dg| {np.max(np.abs(g[s][ok] - ref['g'][ok])):.2e}")
    np.testing.assert_allclose(mu[s][ok], ref["mean"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(s2[s][ok], ref["var"][ok], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g[s][ok], ref["g"][ok], rtol=RTOL, atol=ATOL)
    plain = tall["value"]
    assert np.array_equal(st["var"], s2) and np.array_equal(st["var"], plain[2]["var"]) and np.array_equal(st["count"], plain[2]["count"])
    assert out5[1] == plain[0][1]                                   # the same tree over the same terms
    check_sums(out5[1:2], ve.value_sums(tall["z"], mu, st["var"])[:1], "tall", "sum log s^2 of the trend call")
    cond = np.linalg.cond(np.linalg.inv(cov))
    assert cond < 1e3, cond
    check_gram(out5, beta, cov, tall["z"], tall["X"], tall["prior"], tall["debug"], "tall")
    Q = out5[4] - (np.linalg.inv(cov) @ beta) @ beta
    assert abs(out5[3] - Q) <= 1e-12 * abs(out5[4])
    total = -0.5 * (len(mu) * LOG2PI + out5[1] + out5[3])
    assert abs(out5[0] - total) <= 8 * ve.U * (len(mu) * LOG2PI + abs(out5[1]) + abs(out5[3]))


def test_tall_trend_gradient(tall):
    pb = tall["pb"]
    out5, beta, cov, grad, info, st = tall["trend_grad"]
    value = tall["trend"]
    assert info == 0 and np.array_equal(out5, value[0]) and np.array_equal(beta, value[1]) and np.array_equal(cov, value[2])
    check_sums(grad, ve.score_sums(st["score"]), "tall", "the gradient of the profiled value")
    n0 = len(pb["coords"][0])
    r = tall["z"] - tall["X"] @ beta                                # the scores are those of the residual at beta-hat
    ref = ve.sampled_reference(pb, ve.tall_sample(), values=[r[:n0], r[n0:]])
    ok, s = tall_kept(ref), ref["index"]
    es = vgr.measure(st["score"][s][ok][:, :11], ref["score"][ok][:, :11])
    print(f"tall trend gradient: score measure max {es.max():.2e} on {np.count_nonzero(ok)} sampled data")
    assert es.max() < tgt.TOL_GRAD
    assert np.all(grad[11:] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 3b. the information beyond 256 rows
# ---------------------------------------------------------------------------------------------------------------------
def test_information_beyond_256_rows(native):
    pb, sets = ve.info_tall_problem(), ve.info_tall_sets()
    assert sets["gap"].min() > 1e-9 and sets["info"] == 0
    assert sum(-(-len(c) // 8) for c in pb["coords"]) == 258
    h = open_handle(native, pb)
    t0 = time.perf_counter()
    I, info, st = h.loglik_vecchia_fisher(pb["ranks"], pb["max_dist"])
    print(f"information at N = {len(pb['ranks'])}: {time.perf_counter() - t0:.2f} s, {h.vecchia_fisher_timings()}")
    h.close()
    assert info == 0 and (st["n_empty"], st["k_max"], st["n_capped"]) == (sets["n_empty"], sets["k_max"], sets["n_capped"])
    tgi.check_matrix(I, ve.info_tall_reference(), ve.INFO_TALL, tol=ve.info_tol(ve.INFO_TALL))
    tgi.check_shape(I, np.arange(11))


# ---------------------------------------------------------------------------------------------------------------------
# 4. trend width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,caps", ve.WIDE_CASES)
def test_wide_designs(native, ps, caps):
    pb, trend = tgt.problem(), ve.wide_trend(*ps)
    ref = tgt.reference(pb, trend, 0.5, caps)
    label = f"p = {ps} caps {caps}"
    assert ref["p"] == sum(ps) and ref["k_max"] == 2 * caps[0] and np.linalg.cond(ref["A"]) < 1e3
    h = tgt.make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], ref["F"])
    h.set_local_neighbours(*caps)
    out5, beta, cov, st = tgt.check_case(h, pb, ref, 0.5, label)
    assert h.vecchia_trend_timings()["p"] == sum(ps) and beta.shape == (sum(ps),)
    dbg = h.debug_vecchia_trend(pb["ranks"], 0.5)
    check_gram(out5, beta, cov, ref["z"], ref["X"], ref["prior"] + ref["own"], dbg, label)
    if ps == (8, 8):   # the method and the bound of tests/test_gpu_vecchia_trend.py: test_gradient_of_the_profiled_value
        want = tgt.grad_reference(pb, ref)
        out5g, betag, covg, grad, info, stg = h.loglik_vecchia_trend_grad(pb["ranks"], 0.5, scores=True)
        assert info == 0 and np.array_equal(out5g, out5) and np.array_equal(betag, beta) and np.array_equal(covg, cov)
        eg = vgr.measure(grad[:11], want["grad13"][:11])
        es = vgr.measure(stg["score"][:, :11], want["score"][:, :11])
        print(f"{label}: gradient measure max {eg.max():.2e}, score measure max {es.max():.2e}")
        assert eg.max() < tgt.TOL_GRAD and es.max() < tgt.TOL_GRAD, (grad, want["grad13"])
        assert np.all(grad[11:] == 0.0) and np.all(stg["score"][:, 11:] == 0.0)
        check_sums(grad, ve.score_sums(stg["score"]), label, "the gradient of the profiled value")
        x0 = np.array(pb["params"], dtype=float)
        for k in (0, 3, 6, 9, 10):
            e = 1e-5 * max(abs(x0[k]), 1.0)
            f = []
            for sgn in (1.0, -1.0):
                x = x0.copy()
                x[k] += sgn * e
                f.append(vtr.profile_value(x, pb["coords"], pb["values"], ref["X"], EUC, ref["keep"]))
            fd = (f[0] - f[1]) / (2 * e)
            assert vgr.measure(grad[k], fd) < tgt.TOL_GRAD, (k, grad[k], fd)
    h.close()


def test_sixteen_columns_under_full_conditioning_are_dense_gls(native):
    """40 + 25 data, p = 8 + 8: tests/test_gpu_vecchia_trend.py's comparison with numpy dense GLS, ck_loglik_reml and
    ck_predict_universal in both orderings, run on the wide design; then the Gram identity on the same references"""
    from sif_xco2_cokriging_amd import vecchia
    trend = ve.wide_trend(8, 8)
    tgt.test_full_conditioning_is_dense_gls(native, trend)
    pb = tgt.small_problem()
    F = vtr.design(trend, pb["coords"])[1]
    h = tgt.make_handle(native, pb["params"], EUC, pb["coords"], pb["values"], F)
    h.set_local_neighbours(0, 0)
    for ordering in ("random", "hilbert"):
        ranks = vecchia.ordering_ranks(pb["coords"], ordering, 1)
        ref = tgt.reference(pb, trend, 2.0, (0, 0), ranks=ranks, key=ordering)
        assert ref["p"] == 16 and ref["k_max"] == 64 and np.linalg.cond(ref["A"]) < 1e3
        out5, beta, cov, info, _ = h.loglik_vecchia_trend(ranks, 2.0)
        assert info == 0
        check_gram(out5, beta, cov, ref["z"], ref["X"], ref["prior"] + ref["own"], h.debug_vecchia_trend(ranks, 2.0),
                   f"p = 16 full conditioning {ordering}")
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. one handle across settings
# ---------------------------------------------------------------------------------------------------------------------
def all_calls(h, pb, F):
    """every Vecchia call under the handle's present caps and noise: the trend-free three, then the trend calls with F, then the
    trend cleared again (p_k = 0).  Floats as bit patterns."""
    ranks, md = pb["ranks"], pb["max_dist"]
    out = [h.loglik_vecchia(ranks, md, terms=True), h.loglik_vecchia_grad(ranks, md, scores=True), h.loglik_vecchia_fisher(ranks, md)]
    for k in range(len(F)):
        h.set_trend(k, F[k])
    out += [h.loglik_vecchia_trend(ranks, md, terms=True), h.loglik_vecchia_trend(ranks, md, reml=True),
            h.loglik_vecchia_trend_grad(ranks, md, scores=True), h.debug_vecchia_trend(ranks, md)]
    for k in range(len(F)):
        h.set_trend(k, np.zeros((len(pb["coords"][k]), 0)))
    out.append(h.loglik_vecchia_trend(ranks, md))                   # without a trend: the plain likelihood
    return flat(out)


def flat(x):
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (tuple, list)):
        return [flat(y) for y in x]
    return bits(x) if isinstance(x, np.ndarray) else x


def same_bits(a, b):
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, tuple):
        return a[0] == b[0] and same_bits(a[1], b[1])
    return np.array_equal(a, b)


def apply_settings(h, pb, caps, noise, scale):
    h.set_local_neighbours(*caps)
    h.set_noise(0, noise, scale)


@pytest.mark.parametrize("label", ["300+213", "8+9", "64+1", "257+255"])
def test_one_handle_across_settings(native, label):
    """caps (4, 4) -> (0, 0) where the sets stay within 64 -> (4, 4); noise on process 0 set at one stop and cleared at the next;
    the trend from 16 columns down to the rung's own and to unequal blocks, cleared after every stop.  Each stop's outputs equal a
    fresh handle's, which is given that stop's settings only."""
    pb = ve.rung(label)
    n = ve.sizes_of(label)
    d0 = 0.05 + 0.1 * np.random.default_rng(21).random(n[0])
    own = ve.trend_design(pb, ve.trend_kinds(n))[1]
    wide = [ve.wide_columns(c)[:, :min(8, max(1, len(c) // 2))] for c in pb["coords"]]   # p = 16 where the sites allow it
    uneven = [wide[0][:, :1], wide[1][:, :7]]
    stops = [(ve.CAPS, None, 1.0, wide), ((0, 0) if sum(n) <= 64 else (2, 3), d0, 2.0, own), (ve.CAPS, None, 1.0, uneven),
             (ve.CAPS, d0, 0.5, own), (ve.CAPS, None, 1.0, own)]
    h = open_handle(native, pb)
    gots = []
    for i, (caps, noise, scale, F) in enumerate(stops):
        apply_settings(h, pb, caps, noise, scale)
        gots.append(all_calls(h, pb, F))
        fresh = open_handle(native, pb)
        apply_settings(fresh, pb, caps, noise, scale)
        want = all_calls(fresh, pb, F)
        fresh.close()
        assert same_bits(gots[i], want), (label, i)
        with pytest.raises(native.NativeError, match="data already laid out on the device; create a new handle"):
            h.set_data(0, pb["coords"][0][:1], pb["values"][0][:1])
    h.close()
    assert same_bits(gots[0][:3], gots[4][:3])                      # back at the first settings: the first bits
    for i in (1, 3):
        assert not same_bits(gots[0][:3], gots[i][:3])              # and the stops in between did change the outputs
    # the first stop is the ladder's own case, held to the reference there: ("count", array) leads loglik_vecchia's stats
    assert gots[0][0][2][0][0] == "count" and np.array_equal(gots[0][0][2][0][1], ve.value_reference(label)["count"])
