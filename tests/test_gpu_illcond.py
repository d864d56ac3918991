"""GPU tests of the Cholesky paths on ill-conditioned Sigma against extended precision ("Stability of the
inverse-based row solves"; data sets, references and the derivation of the bounds: tests/illcond_ref.py; the conditions that
make these inputs fair: tests/test_illcond_host.py).

Dense path (ck_factor, ck_loocv, ck_loglik, the step-wise form), option exact_cov = 1, site_order 0 and 1.  All truth is computed
from the DEVICE's own Sigma (ck_debug_get_lower after ck_assemble_joint), in np.longdouble, so the entry errors of the
covariance do not enter; the test first asserts that LAPACK factors that Sigma.  With u = 2^-53, gamma_n = n u / (1 - n u),
L the longdouble factor and kappa_blk = max_j cond_2(L_jj) over the 64-blocks as the device cuts them:
  a  factor() == 0
  b  |Sigma - L_gpu L_gpu^T| <= gamma_{N+1} (1 + kappa_blk) |L||L^T| componentwise                                   (asserted)
  c  the amplification be_gpu / be_LAPACK, componentwise and normwise, and whether Higham's gamma_{N+1} |L||L^T| holds  (printed)
  d  x = Sigma^-1 z recovered from ck_loocv as x_q = (z_q - pred_q) / err_q^2:
     |z - Sigma x| <= gamma_{3N+1} (1 + kappa_blk) |L||L^T||x| + 4 u (|Sigma||x| + |z|)                             (asserted)
  e  ck_loglik: |d log|Sigma|| <= sum(|Sigma^-1| o bound_b) + 4 N u and |d z^T Sigma^-1 z| <= |x|^T bound_b |x| + 4 N u z^T Sigma^-1 z
     (the first-order consequences of b; the last terms are the roundings of the N-term sums themselves; |Sigma^-1| in float64
     from the longdouble factor rounded), with the ratio to LAPACK's own error printed                               (asserted)
  f  on NEARDUP_PANELS ck_panel_factor / ck_panel_apply give the bits of ck_factor (no other test drives them by hand)
UNI65 runs a, b, d.  |x| in the bounds is the longdouble solution's, never the library's.

Local solvers on NEARDUP with max_dist beyond the domain (every neighbourhood is the whole subset), site_order = 0, exact_cov = 1,
Sigma_loc and c from the oracle, EPS_C = 5e-13 the project's entry tolerance:
  LDS class (lp_chol, k = 32 + 32, through ck_debug_simulate_local_weights): per site
     |c - Sigma_loc w| <= (gamma_{3k+1} |L||L^T| + EPS_C |Sigma_loc|) |w| + EPS_C |c|        -- lp_chol uses no inverse: no kappa
  tiled and slab classes (k = 130 + 126, local_tile_min = 0 and 10**6, seven sites through ck_predict_local):
     |d pred| <= |w|^T (gamma_{3 kq + 1} (1 + kappa_blk) |L||L^T| + EPS_C |Sigma|) |a| + EPS_C |c|^T |a|,  a = Sigma^-1 z,
     and with c in place of z for pred_err^2.  csrc/ck_local.hip / csrc/ck_la.hip: the tiled route factors its diagonal blocks
     with k_lt_potrf64 (potrf64_body: factor and explicit inverse) and solves every row below -- the c and z rows among them,
     they are two more rows of the padded matrix -- as a product with that inverse (k_lt_rows*): kappa_blk over the 64-blocks of
     the compacted neighbour list, kq = k + 2 rounded up to 64.  The slab kernel (k_local_solve_big) factors 32-column panels
     in LDS and solves the rows below by substitution, one thread per row: no inverse, kappa_blk = 0, kq = k + 2.

Seen on an MI355X (pytest -s prints every figure).  Every asserted bound held; factor() returned 0 everywhere.
  b / c, the factor: componentwise backward error / (N u) of GPU | LAPACK (amplification), normwise GPU (amplification),
  |R| / block bound, Higham's gamma_{N+1}:
    set, site_order    kappa_blk   GPU      LAPACK   (ampl.)    normwise GPU (ampl.)   / block bound   Higham's
    WELL            0   2.3e1      0.068    0.059    (1.2)      1.1e-16 (1.8)          2.9e-3          holds
    WELL            1   2.2e1      0.081    0.034    (2.4)      1.2e-16 (2.8)          3.4e-3          holds
    SMOOTH          0   2.6e4      0.84     0.064    (13)       9.2e-16 (19)           3.2e-5          holds
    SMOOTH          1   3.8e4      39       0.063    (6.2e2)    3.6e-14 (7.8e2)        1.0e-3          does not hold
    NEARDUP         0   1.1e5      4.4e3    0.065    (6.7e4)    1.6e-13 (2.7e3)        4.0e-2          does not hold
    NEARDUP         1   1.2e5      7.7e3    0.050    (1.5e5)    2.4e-12 (7.7e4)        6.6e-2          does not hold
    NEARDUP_PANELS  0   3.1e4      5.6      0.035    (1.6e2)    5.4e-15 (72)           1.8e-4          does not hold
    NEARDUP_PANELS  1   5.0e4      8.2e2    0.031    (2.6e4)    3.6e-12 (7.7e4)        1.7e-2          does not hold
    UNI65           0   1.7e3      0.30     0.077    (3.9)      1.1e-16 (2.4)          1.8e-4          holds
    UNI65           1   1.7e3      0.43     0.054    (7.9)      1.0e-16 (3.6)          2.5e-4          holds
  The float64 emulation with a one-level inverse (tests/illcond_ref.py: emulate_inverse_blocked) predicts 62 for NEARDUP in the
  caller's order, the device shows 4.4e3: potrf64_body builds the inverse on two levels (16 x 16 diagonal blocks inverted, the
  blocks below them as products with those inverses), and the emulation of exactly that (two_level = True) gives 2.8e3, 7.8e3,
  4.9 and 9.1e2 on the four NEARDUP rows -- the device does what its algorithm does.  The normwise error on NEARDUP, site_order 1,
  is 0.09 / cond_2(Sigma): an order of magnitude from where "not positive definite" becomes a legitimate answer.
  d, the solve: largest |z - Sigma x| / bound 3.8e-4 (NEARDUP, site_order 1); against gamma_{3N+1} |L||L^T||x|, Higham's bound for a
    substitution-based solve, the residual stands at 12 and 45 on NEARDUP (0 / 1), 1.5 on SMOOTH 0, 1.7 on NEARDUP_PANELS 1,
    below 0.3 elsewhere; LAPACK's at 2e-3 or below everywhere.
  e, ck_loglik: |d log|Sigma|| GPU | LAPACK, |d z^T Sigma^-1 z| GPU | LAPACK (the bounds are 1e9 .. 1e3 times larger):
    WELL 0 / 1            1.1e-13 | 0        3.4e-13 | 0           3.1e-13 | 2.8e-14   8.5e-14 | 5.7e-14
    SMOOTH 0 / 1          5.9e-9 | 4.9e-8    1.4e-7 | 2.3e-8       1.8e-7 | 2.4e-8     1.8e-6 | 2.1e-8
    NEARDUP 0 / 1         1.5e-4 | 2.9e-6    1.6e-7 | 5.1e-7       5.2e-3 | 3.0e-7     4.0e-6 | 3.3e-6
    NEARDUP_PANELS 0 / 1  1.1e-5 | 1.9e-6    4.8e-5 | 5.3e-7       7.6e-5 | 1.5e-6     2.2e-5 | 5.0e-7
    the worst ratio to LAPACK: 91 on the log-determinant (NEARDUP_PANELS 1), 1.7e4 on the quadratic form (NEARDUP 0: 5.2e-3 of
    220, a relative 2.4e-5 -- beyond the 1e-6 parity target).
  f: identical bits, both site orders.
  local solvers: LDS class |c - Sigma_loc w| / bound 1.8e-3 | 1.6e-3 (process 0 | 1), cond_2(Sigma_loc) = 8.9e9;
    tiled class (kappa_blk 1.05e5): |d pred| 3.4e-6 | 9.3e-6, 670 | 820 times LAPACK's; |d var| 1.1e-8 | 3.3e-8, 240 | 140 times;
      1e-6 of the bound (the first-order forward bound is far from sharp here: it exceeds |pred| itself);
    slab class: |d pred| 4.0e-8 | 2.4e-8, 7.8 | 2.1 times LAPACK's; |d var| 4.5e-10 | 7.6e-10, 9.7 | 3.2 times; 1e-4 .. 9e-4 of
      the bound.
"""
import numpy as np
import pytest
import scipy.linalg as sla

from tests import illcond_ref as ir

pytestmark = pytest.mark.gpu

DENSE = ["WELL", "SMOOTH", "NEARDUP", "NEARDUP_PANELS"]
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def handle(native, p, coords, values, site_order):
    h = native.Handle(0)
    h.set_option("exact_cov", 1)
    h.set_option("site_order", site_order)
    if p.n_procs == 2:
        h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                    p.nugget, p.rho)
    else:
        h.set_model(1, p.sigma, [p.nu[0, 0]] * 3, [p.len_scale[0, 0]] * 3, p.nugget, 0.0)
    h.set_metric(ir.EUC)
    for k in range(p.n_procs):
        h.set_data(k, coords[k], values[k])
    return h


def internal_index(h, ds):
    """stacked caller indices in the handle's internal order"""
    out, off = [], 0
    for k, c in enumerate(ds.coords):
        out.append(off + h.debug_site_order(k, len(c)))
        off += len(c)
    return np.concatenate(out)


def dense_run(native, name, site_order):
    """everything the device computes for one (data set, site order), once: Sigma, info, L, the loocv outputs, loglik"""
    key = (name, site_order)
    if key in _cache:
        return _cache[key]
    ds = ir.data_set(name)
    h = handle(native, ds.p, ds.coords, ds.values, site_order)
    h.assemble_joint()
    idx = internal_index(h, ds)
    if site_order == 0:
        assert np.array_equal(idx, np.arange(ds.N))
    else:
        assert np.array_equal(np.sort(idx), np.arange(ds.N)) and not np.array_equal(idx, np.arange(ds.N))
    S = ir.sym_from_lower(h.debug_get_lower(ds.N))
    So = ds.S[np.ix_(idx, idx)]
    entry = float(np.max(np.abs(S - So) / np.abs(So)))
    try:
        Llap = np.linalg.cholesky(S)
    except np.linalg.LinAlgError as e:   # the input, not the library, is at fault
        pytest.fail(f"{name} site_order {site_order}: LAPACK does not factor the device's own Sigma ({e}); largest relative "
                    f"entry difference to the oracle {entry:.2e} -- the INPUT is at fault, not the factorisation")
    ref = ir.Reference(S, ir.blocks(ds.n0, ds.n1))
    r = dict(ds=ds, idx=idx, S=S, ref=ref, Llap=Llap, entry=entry, z=ds.z[idx])
    r["info"] = h.factor()
    if r["info"] == 0:
        r["L"] = np.tril(h.debug_get_lower(ds.N))
        x = []
        for k, c in enumerate(ds.coords):
            pred, err = h.loocv(k, len(c))
            x.append((ds.values[k] - pred) / err ** 2)
        r["x"] = np.concatenate(x)[idx]
        if ds.p.n_procs == 2:
            r["loglik"] = h.loglik()
    h.close()
    print(f"{name} site_order {site_order}: N = {ds.N} cond_2 = {ref.cond2:.2e} kappa_blk = {ref.kappa_blk:.2e}; device Sigma "
          f"against the oracle's, largest relative entry difference {entry:.2e}; factor() = {r['info']}")
    _cache[key] = r
    return r


CASES = [(n, so) for n in DENSE + ["UNI65"] for so in (0, 1)]
BIV_CASES = [(n, so) for n in DENSE for so in (0, 1)]


@pytest.mark.parametrize("name,site_order", CASES)
def test_factor_block_bound(native, name, site_order):
    """a, b asserted; c printed"""
    r = dense_run(native, name, site_order)
    ref, N = r["ref"], r["ds"].N
    assert r["info"] == 0, f"factor() reports minor {r['info']} on a Sigma LAPACK and the float64 emulation factor"
    comp, norm, Ra = ir.factor_errors(ref, r["L"])
    comp_l, norm_l, _ = ir.factor_errors(ref, r["Llap"])
    worst = float(np.max(Ra / ref.bound_b()))
    higham = float(np.max(Ra / ref.bound_b(False)))
    print(f"{name} site_order {site_order}: comp. backward err / (N u): GPU {comp / (N * ir.U):.3g} LAPACK {comp_l / (N * ir.U):.3g} "
          f"(amplification {comp / comp_l:.3g}); normwise: GPU {norm:.2e} LAPACK {norm_l:.2e} (amplification {norm / norm_l:.3g}); "
          f"|R| / block bound = {worst:.2e}; |R| / Higham's gamma_(N+1) |L||L^T| = {higham:.3g} "
          f"({'holds' if higham <= 1 else 'does NOT hold'})")
    assert worst <= 1.0


@pytest.mark.parametrize("name,site_order", CASES)
def test_solve_through_loocv(native, name, site_order):
    """d"""
    r = dense_run(native, name, site_order)
    assert r["info"] == 0
    ref, N, z = r["ref"], r["ds"].N, r["z"]
    xr = np.abs(np.asarray(ref.solve(z), dtype=np.float64))
    bound = ir.gamma(3 * N + 1) * (1.0 + ref.kappa_blk) * (ref.absLLt @ xr) + 4 * ir.U * (np.abs(ref.S) @ xr + np.abs(z))
    res = ir.solve_residual(ref.S, r["x"], z)
    res_l = ir.solve_residual(ref.S, sla.cho_solve((r["Llap"], True), z), z)
    plain = ir.gamma(3 * N + 1) * (ref.absLLt @ xr)
    print(f"{name} site_order {site_order}: |z - Sigma x| / bound = {np.max(res / bound):.2e}; against Higham's 3-gamma bound of a "
          f"substitution: GPU {np.max(res / plain):.3g} LAPACK {np.max(res_l / plain):.3g}; largest residual GPU {res.max():.2e} "
          f"LAPACK {res_l.max():.2e}")
    assert np.all(np.isfinite(r["x"]))
    assert np.all(res <= bound)


@pytest.mark.parametrize("name,site_order", BIV_CASES)
def test_loglik(native, name, site_order):
    """e"""
    r = dense_run(native, name, site_order)
    assert r["info"] == 0
    ref, N, z = r["ref"], r["ds"].N, r["z"]
    info, (l, logdet, quad), _ = r["loglik"]
    assert info == 0
    bb = ref.bound_b()
    xr = np.abs(np.asarray(ref.solve(z), dtype=np.float64))
    ld_ref, q_ref = ref.logdet(), ref.quad(z)
    b_ld = float(np.sum(ref.inverse_abs() * bb)) + 4 * N * ir.U
    b_q = float(xr @ bb @ xr) + 4 * N * ir.U * q_ref
    ld_lap = 2.0 * np.sum(np.log(np.diag(r["Llap"])))
    y = sla.solve_triangular(r["Llap"], z, lower=True)
    e_ld, e_q = abs(logdet - ld_ref), abs(quad - q_ref)
    e_ld_l, e_q_l = abs(ld_lap - ld_ref), abs(float(y @ y) - q_ref)
    print(f"{name} site_order {site_order}: log|Sigma| = {ld_ref:.6f}: |d| GPU {e_ld:.2e} LAPACK {e_ld_l:.2e} bound {b_ld:.2e}; "
          f"z^T Sigma^-1 z = {q_ref:.6f}: |d| GPU {e_q:.2e} LAPACK {e_q_l:.2e} bound {b_q:.2e}; "
          f"ratios to LAPACK {e_ld / max(e_ld_l, 1e-300):.3g} / {e_q / max(e_q_l, 1e-300):.3g}")
    assert e_ld <= b_ld
    assert e_q <= b_q
    # l from its own two terms: three roundings on numbers of these sizes
    assert abs(l + 0.5 * (N * np.log(2 * np.pi) + logdet + quad)) <= 4 * ir.U * (N * np.log(2 * np.pi) + abs(logdet) + abs(quad))


@pytest.mark.parametrize("site_order", [0, 1])
def test_stepwise_form_gives_the_bits_of_factor(native, site_order):
    """f"""
    r = dense_run(native, "NEARDUP_PANELS", site_order)
    assert r["info"] == 0
    ds = r["ds"]
    h = handle(native, ds.p, ds.coords, ds.values, site_order)
    h.assemble_joint()
    nK = h.num_panels()[0]
    assert nK == 3   # 513 + 511 pads to 576 + 512: row solves across panel boundaries
    for K in range(nK):
        h.panel_factor(K)
        h.panel_apply(K, native.APPLY_SIGMA)
    assert h.factor_info() == 0
    L = np.tril(h.debug_get_lower(ds.N))
    h.close()
    assert np.array_equal(L, r["L"])


# ---- local solvers ------------------------------------------------------------------------------------------------------------------
def local_handle(native, ls, tile_min=None):
    h = handle(native, ir.data_set("NEARDUP").p, ls.coords, ls.values, 0)
    if tile_min is not None:
        h.set_option("local_tile_min", tile_min)
    return h


@pytest.mark.parametrize("i", [0, 1])
def test_lds_class_weights(native, i):
    """one site per call: a call's earlier sites would join the set of a later one and push it beyond the LDS limit"""
    pc = ir.pred_sites()
    ls = ir.LocalSystem(32, 32, i, pc, tiled=False)
    h = local_handle(native, ls)
    worst = 0.0
    for t in range(len(pc)):
        idx, w = h.simulate_local_weights(i, pc[t:t + 1], np.zeros(1, dtype=np.int64), ir.MAX_DIST)
        assert np.array_equal(idx[0], np.arange(64))
        res = ir.solve_residual(ls.ref.S, w[0], ls.c[:, t])
        bound = ls.weight_bound(t)
        worst = max(worst, float(np.max(res / bound)))
        assert np.all(res <= bound), (t, float(np.max(res / bound)))
    h.close()
    print(f"LDS class, process {i}: cond_2(Sigma_loc) = {ls.ref.cond2:.2e}; largest |c - Sigma_loc w| / bound over the sites {worst:.2e}")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("tile_min", [0, 10 ** 6])
def test_tiled_and_slab_classes(native, tile_min, i):
    pc = ir.pred_sites()
    tiled = tile_min == 0
    key = ("local", i, tiled)
    if key not in _cache:
        _cache[key] = ir.LocalSystem(130, 126, i, pc, tiled=tiled)
    ls = _cache[key]
    kq = 64 * ((ls.k + 2 + 63) // 64) if tiled else ls.k + 2
    h = local_handle(native, ls, tile_min)
    pred, err, info = h.predict_local(i, pc, max_dist=ir.MAX_DIST)
    h.close()
    assert info["k_max"] == 256 and info["n_not_pd"] == 0 and info["n_empty"] == 0, info
    bp, bv = ls.forward_bounds(kq)
    lp, lv = ls.lapack()
    dp, dv = np.abs(pred - ls.pred), np.abs(err ** 2 - np.maximum(ls.var, 0.0))
    dpl, dvl = np.abs(lp - ls.pred), np.abs(lv - ls.var)
    print(f"{'tiled' if tiled else 'slab'} class, process {i}: cond_2 = {ls.ref.cond2:.2e} kappa_blk = {ls.kappa:.2e}; "
          f"|d pred| / bound {np.max(dp / bp):.2e}, |d var| / bound {np.max(dv / bv):.2e}; largest |d pred| GPU {dp.max():.2e} "
          f"LAPACK {dpl.max():.2e} (ratio {dp.max() / dpl.max():.3g}); |d var| GPU {dv.max():.2e} LAPACK {dvl.max():.2e} "
          f"(ratio {dv.max() / dvl.max():.3g}); smallest variance {ls.var.min():.2e}")
    assert np.all(np.isfinite(pred)) and np.all(np.isfinite(err))
    assert np.all(dp <= bp)
    assert np.all(dv <= bv)
