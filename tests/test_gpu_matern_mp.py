"""The DEVICE build of the covariance evaluator (csrc/ck_math.h: ck_matern_rho_scaled, ck_matern_dlen_scaled, ck_matern_grad,
and the interpolation table built from them) against extended precision: tests/golden/matern_mp.npz, made by mpmath alone
(tests/golden/make_matern_mp.py).  The bounds are stated and derived in tests/matern_mp_ref.py; tests/test_matern_mp_host.py
shows on the CPU that the host build of the same header meets them.  Every test prints its measured maximum in units of its
bound."""
import numpy as np
import pytest

from tests import dense_chains as dc
from tests import matern_mp_ref as ref

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


@pytest.fixture(scope="module")
def g():
    return ref.load()


def _set(h, params):
    p = np.asarray(params, dtype=float)
    h.set_model(2, p[0:2], p[2:5], p[5:8], p[8:10], p[10])


@pytest.fixture(scope="module")
def lag_runs(native, g):
    """every (nu, ell) of the lag grid on ONE handle through repeated set_model -- with tables built before the first change of
    the model, so that every later one marks them stale: (Lags, cov_lags, model_variogram at the small lags, debug_matern_grad)"""
    h = native.Handle(0)
    h.set_metric(EUC)
    h.set_option("site_order", 0)
    sites = np.array([[0.0, 0.0], [0.3, 0.4], [1.0, 1.0]])
    h.set_model(1, [1.0], [1.3] * 3, [1.0] * 3, [0.0], 0.0)
    h.set_data(0, sites, np.zeros(3))
    h.assemble_joint()
    first = h.debug_get_lower(3)
    runs = []
    for k in range(len(g["nus"])):
        for e in range(len(g["ells"])):
            L = ref.Lags(g, k, e)
            h.set_model(1, [1.0], [L.nu] * 3, [L.ell] * 3, [0.0], 0.0)
            runs.append((L, h.cov_lags(0, 0, L.h_all, use_nugget=False), h.model_variogram(0, 0, L.h[:len(L.omM)]),
                         h.debug_matern_grad(0, L.h_all)))
    # the handle still assembles after 56 models, with the tables of the model it has now
    h.set_model(1, [1.0], [1.3] * 3, [1.0] * 3, [0.0], 0.0)
    h.assemble_joint()
    assert np.array_equal(h.debug_get_lower(3), first)
    h.close()
    return runs


def _report(name, worst, where):
    print(f"device, {name}: largest error {worst:.3g} of its bound at (nu, ell) = {where}")


def test_values_at_every_order(lag_runs):
    """cov_lags: |M_dev / M - 1| <= 8 u + 5e-15 where M > 1e-290, 1e-290 absolute below, exactly 1 at h = 0"""
    worst, where = 0.0, None
    for L, cov, _, _ in lag_runs:
        assert cov[-1] == 1.0, (L.nu, L.ell)
        e = L.value(cov[:-1])
        if e > worst:
            worst, where = e, (L.nu, L.ell)
    _report("value", worst, where)
    assert worst <= 1.0, (worst, where)


def test_semivariogram_at_small_lags(lag_runs):
    """model_variogram: |gamma_dev - sigma^2 (1 - M)| <= sigma^2 M (8 u + 5e-15): the value bound carried through the subtraction"""
    worst, where = 0.0, None
    for L, _, gam, _ in lag_runs:
        e = L.gamma(gam)
        if e > worst:
            worst, where = e, (L.nu, L.ell)
    _report("semivariogram", worst, where)
    assert worst <= 1.0, (worst, where)


def test_derivatives_per_entry(lag_runs):
    """ck_debug_matern_grad: M and dM/dlen to the value bound, dM/dnu to the rounding bound against the library's formula
    evaluated exactly and to 1e-7 against the true derivative; exact zeros where M is 0 and (1, 0, 0) at h = 0"""
    names = ("value", "dM/dlen", "dM/dnu rounding", "dM/dnu against the true derivative")
    worst, where = [0.0] * 4, [None] * 4
    for L, cov, _, out in lag_runs:
        assert np.array_equal(out[:, 0], cov), (L.nu, L.ell)      # the gradient's M is the evaluator's
        for q, e in enumerate(ref.check_grad_rows(L, out)):
            if e > worst[q]:
                worst[q], where[q] = e, (L.nu, L.ell)
    for q in range(3):
        _report(names[q], worst[q], where[q])
    print(f"device, {names[3]}: largest error {worst[3]:.3g} (bound 1e-7) at (nu, ell) = {where[3]}")
    assert max(worst[:3]) <= 1.0, (worst, where)
    assert worst[3] <= 1e-7, (worst[3], where[3])


# ---- Sigma and c0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("tag,metric", [("hav", HAV), ("euc", EUC)])
def test_sigma_against_mpmath(native, g, tag, metric, exact, site_order):
    """the assembly's per-entry and table paths in both site orders (ck_debug_get_lower), with the tolerances
    test_assemble_and_factor_vs_oracle holds against scipy; n0 = 70: process 1 starts at row 128, behind 58 padding rows"""
    c = [g[f"{tag}_c0"], g[f"{tag}_c1"]]
    S = ref.sym(g[f"{tag}_S"])
    h = native.Handle(0)
    _set(h, g[f"{tag}_params"])
    h.set_metric(metric)
    for k in (0, 1):
        h.set_data(k, c[k], np.zeros(len(c[k])))
    h.set_option("exact_cov", int(exact))
    h.set_option("site_order", site_order)
    h.assemble_joint()
    if not exact:
        info = [h.table_info(b) for b in range(3)]
        assert all(t["enabled"] for t in info), info
    idx = np.concatenate([h.debug_site_order(0, 70), 70 + h.debug_site_order(1, 58)])
    if site_order == 0:
        assert np.array_equal(idx, np.arange(128))
    Sp = np.tril(S[np.ix_(idx, idx)])
    low = h.debug_get_lower(128)
    h.close()
    with np.errstate(all="ignore"):
        rel = np.max(np.abs(low[Sp != 0] / Sp[Sp != 0] - 1.0))
    print(f"device Sigma, {tag}, {'exact' if exact else 'table'} path, site_order {site_order}: largest relative error {rel:.3g}")
    if exact:
        np.testing.assert_allclose(low, Sp, rtol=5e-13, atol=1e-30)
    else:
        np.testing.assert_allclose(low, Sp, rtol=5e-13, atol=5e-19 * np.max(np.diag(S)))


@pytest.mark.parametrize("tag,metric", [("hav", HAV), ("euc", EUC)])
def test_cov_dense_blocks_and_c0_against_mpmath(native, g, tag, metric):
    """ck_cov_dense (the per-entry evaluator on device distances): the three blocks of Sigma and c0 of both processes, with
    test_cov_dense_blocks' tolerance"""
    c0, c1, pc = g[f"{tag}_c0"], g[f"{tag}_c1"], g[f"{tag}_pc"]
    S = ref.sym(g[f"{tag}_S"])
    h = native.Handle(0)
    _set(h, g[f"{tag}_params"])
    h.set_metric(metric)
    pairs = [(h.cov_dense(0, 0, c0, c0), S[:70, :70]), (h.cov_dense(0, 1, c0, c1), S[:70, 70:]), (h.cov_dense(1, 1, c1, c1), S[70:, 70:])]
    for i in (0, 1):
        pairs.append((np.vstack([h.cov_dense(i, 0, c0, pc), h.cov_dense(i, 1, c1, pc)]), g[f"{tag}_pcov{i}"]))
    h.close()
    rel = max(float(np.max(np.abs(a / b - 1.0))) for a, b in pairs)
    print(f"device cov_dense, {tag}: largest relative error over Sigma's blocks and both c0 {rel:.3g}")
    for a, b in pairs:
        np.testing.assert_allclose(a, b, rtol=5e-13, atol=1e-300)


# ---- gradient and Fisher information ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,metric", [("ghav", HAV), ("geuc", EUC)])
def test_gradient_and_information_from_the_fixtures_matrices(native, g, tag, metric):
    """ck_loglik's gradient and ck_loglik_fisher against 1/2 z^T S^-1 D_k S^-1 z - 1/2 tr(S^-1 D_k) and 1/2 tr(S^-1 D_j S^-1 D_k)
    in numpy on the fixture's matrices: with the library's own nu stencil in D every slot is an exact expression (1e-9), with
    the true nu derivative the nu slots carry the stencil's truncation (1e-6)"""
    c = [g[f"{tag}_c0"], g[f"{tag}_c1"]]
    h = native.Handle(0)
    _set(h, g[f"{tag}_params"])
    h.set_metric(metric)
    z = g[f"{tag}_z"]
    h.set_data(0, c[0], z[:24])
    h.set_data(1, c[1], z[24:])
    h.assemble_joint()
    info, _, grad = h.loglik(want_grad=True)
    assert info == 0
    h.assemble_joint()
    info, I = h.fisher()
    assert info == 0
    h.close()
    nu_slots = dc.SLOTS[11]["nu"]
    for stencil in (True, False):
        S, zz, D = ref.grad_reference(g, tag, stencil)
        gref = ref.dense_gradient(S, zz, D)
        eg = np.abs(grad - gref) / np.maximum(np.abs(gref), 1.0)
        e = dc.normalised(I, dc.fisher_of(S, D))
        if stencil:
            print(f"device, {tag}, stencil D_nu: gradient {eg.max():.3g}, information {e.max():.3g} (bound 1e-9)")
            assert eg.max() <= dc.FISHER_TOL["exact"], eg
            assert e.max() <= dc.FISHER_TOL["exact"], e
        else:
            en = max(e[nu_slots, :].max(), e[:, nu_slots].max())
            print(f"device, {tag}, true D_nu: gradient nu slots {eg[nu_slots].max():.3g}, information nu pairs {en:.3g} (bound 1e-6)")
            assert eg[nu_slots].max() <= dc.FISHER_TOL["nu"], eg
            assert en <= dc.FISHER_TOL["nu"], e
