"""GPU tests of per-observation measurement-error variances on the joint path: include/cokrige.h ck_set_noise with ck_predict,
ck_factor_predict, ck_predict_universal, ck_loocv, ck_cv_folds, ck_predict_blocks, ck_verify_model and ck_conditional_draws.

Truth is dense numpy in this file, from the oracle's pieces: Sigma_noise = orc.joint_cov(p, coords, metric) + diag(s d), then
cho_factor / cho_solve; c0, the prior variance and C_pp are the field's (no measurement error in them).

Data as tests/test_gpu_cv_folds.py: n0 = 300, n1 = 290 (N = 590 spans two 512-column panels), 150 co-located pairs, haversine and
Euclidean, nugget and zero-nugget parameters.  d: log-uniform over two decades around 1e-2 x the process variance, about 10 %
exact zeros; scales s = (1.5, 0.7).  Bounds: |d pred| < 1e-8 max(1, |pred|) and |d pred_err^2| < 1e-9 (tests/test_gpu_properties.py,
tests/test_gpu_cv_folds.py); draws to 1e-8 relative (tests/test_gpu_conditional.py).

Largest deviations seen on an MI355X over all cases of this file (|d pred| / max(1, |pred|), then |d pred_err^2|): predict,
factor_predict and predict_universal 1.4e-13 and 5.2e-15; LOOCV and folds 1.8e-13 and 7.4e-15; blocks 1.3e-13 and 1.6e-14, their
cov 1.8e-14; conditional draws 7.2e-14 relative; the co-located copies 1.3e-13 and 5.0e-15; through Predictor 6.4e-14 and 4.2e-15."""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
PARAMS = {
    ("nugget", HAV): [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19],
    ("nugget", EUC): [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.02, 0.025, -0.19],
    ("zero", HAV): [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.0, 0.0, -0.19],
    ("zero", EUC): [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.0, 0.0, -0.19],
}
N0, N1 = 300, 290
CASES = [("nugget", HAV), ("nugget", EUC), ("zero", HAV), ("zero", EUC)]
SCALE = (1.5, 0.7)
_cache = {}


def draw_noise(rng, p, ns):
    """d of each process: log-uniform over two decades around 1e-2 sigma_k^2, about 10 % exact zeros"""
    out = []
    for k, n in enumerate(ns):
        d = 1e-2 * p.sigma[k] ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, n)
        d[rng.random(n) < 0.1] = 0.0
        out.append(d)
    return out


def make_data(kind, metric):
    """sites as tests/test_gpu_cv_folds.py (process 1 datum a sits on process 0 datum 150 + a for a < 150); values drawn
    from the noisy model; the dense noisy Sigma and its factor, computed once per case"""
    key = (kind, metric)
    if key not in _cache:
        rng = np.random.default_rng(31 + 2 * metric + (kind == "zero"))
        p = orc.Params.from_flat(PARAMS[key])
        tot = N0 + N1
        if metric == HAV:
            pts = np.column_stack([rng.uniform(25, 50, tot), rng.uniform(-120, -70, tot)])
        else:
            pts = np.column_stack([rng.uniform(0, 10, tot), rng.uniform(0, 10, tot)])
        coords = [pts[:N0].copy(), pts[N0 // 2:N0 // 2 + N1].copy()]
        d = draw_noise(rng, p, (N0, N1))
        assert all((x == 0).any() and (x > 0).any() for x in d)
        S = orc.joint_cov(p, coords, metric) + np.diag(np.concatenate([SCALE[0] * d[0], SCALE[1] * d[1]]))
        z = np.linalg.cholesky(S) @ rng.standard_normal(tot)
        _cache[key] = (p, coords, [z[:N0].copy(), z[N0:].copy()], d, S, cho_factor(S, lower=True))
    return _cache[key]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def handle(native, p, coords, values, metric, noise=None, scale=SCALE, site_order=1, factor=True):
    h = native.Handle(0)
    if site_order != 1:
        h.set_option("site_order", site_order)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
    if noise is not None:
        for k in range(2):
            h.set_noise(k, noise[k], scale[k])
    h.assemble_joint()
    if factor:
        assert h.factor() == 0
    return h


def pred_sites(rng, coords, metric, i, m=40, n_on=12):
    """prediction sites partly on data sites of both processes"""
    if metric == HAV:
        pc = np.column_stack([rng.uniform(26, 49, m), rng.uniform(-118, -72, m)])
    else:
        pc = np.column_stack([rng.uniform(0.2, 9.8, m), rng.uniform(0.2, 9.8, m)])
    pc[:n_on] = coords[i][rng.permutation(len(coords[i]))[:n_on]]
    pc[n_on:n_on + 4] = coords[1 - i][-4:]   # sites of the other process only (not co-located)
    return pc[rng.permutation(m)]


def dense_predict(p, coords, values, pc, i, metric, cf):
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    w = cho_solve(cf, c0)
    pred = w.T @ np.concatenate(values)
    S = orc.pred_cov(p, pc, i, metric) - c0.T @ w
    return pred, S


def check(pred, err, rp, rvar, what):
    dp = np.max(np.abs(pred - rp) / np.maximum(1.0, np.abs(rp)))
    dv = np.max(np.abs(err ** 2 - np.maximum(rvar, 0.0)))
    print(f"{what}: max |d pred| / max(1, |pred|) = {dp:.3e}, max |d pred_err^2| = {dv:.3e}")
    assert dp < 1e-8, what
    assert dv < 1e-9, what


# ---- 1. the point predictors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site_order", [0, 1])
@pytest.mark.parametrize("kind,metric", CASES)
def test_predict_forms_match_the_dense_chain(native, kind, metric, site_order):
    p, coords, values, d, S, cf = make_data(kind, metric)
    for i in (0, 1):
        pc = pred_sites(np.random.default_rng(5 + i), coords, metric, i)
        rp, rS = dense_predict(p, coords, values, pc, i, metric, cf)
        h = handle(native, p, coords, values, metric, d, site_order=site_order, factor=False)
        info, pred, err = h.factor_predict(i, pc)
        assert info == 0
        check(pred, err, rp, np.diag(rS), f"factor_predict {kind} {metric} i={i} order={site_order}")
        p2, e2 = h.predict(i, pc)
        check(p2, e2, rp, np.diag(rS), f"predict {kind} {metric} i={i} order={site_order}")
        # universal, constant trend per process: the dense bordered chain with the noisy Sigma
        for k in range(2):
            h.set_trend(k, np.ones((len(coords[k]), 1)))
        pu, eu, beta, bcov = h.predict_universal(i, pc, np.ones((len(pc), 1)))
        X = np.zeros((N0 + N1, 2))
        X[:N0, 0], X[N0:, 1] = 1.0, 1.0
        z = np.concatenate(values)
        c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
        SiX, Siz, Sic = cho_solve(cf, X), cho_solve(cf, z), cho_solve(cf, c0)
        A = X.T @ SiX
        b = np.linalg.solve(A, X.T @ Siz)
        x0 = np.zeros((2, len(pc)))
        x0[i] = 1.0
        r = x0 - X.T @ Sic
        up = c0.T @ Siz + r.T @ b
        uv = np.diag(rS) + np.einsum("js,js->s", r, np.linalg.solve(A, r))
        check(pu, eu, up, uv, f"predict_universal {kind} {metric} i={i} order={site_order}")
        assert np.max(np.abs(beta - b)) < 1e-8
        h.close()


# ---- 2. cross-validation predicts the withheld observation ------------------------------------------------------------------
def dense_folds(p, coords, values, d, metric, i, fi, fo, S):
    """remove the fold, predict the withheld OBSERVATIONS of process i with the dense noisy Sigma: the variance has s d_q"""
    n_i = len(coords[i])
    off = [0, N0]
    z = np.concatenate(values)
    pred, var = np.full(n_i, np.nan), np.full(n_i, np.nan)
    lab = np.full(N0 + N1, -1)
    lab[off[i]:off[i] + n_i] = fi
    if fo is not None:
        lab[off[1 - i]:off[1 - i] + len(fo)] = fo
    for f in range(int(fi.max()) + 1):
        out = np.flatnonzero(lab == f)
        mine = out[(out >= off[i]) & (out < off[i] + n_i)]
        keep = np.flatnonzero(lab != f)
        cf = cho_factor(S[np.ix_(keep, keep)], lower=True)
        C = S[np.ix_(keep, mine)]
        W = cho_solve(cf, C)
        pred[mine - off[i]] = W.T @ z[keep]
        var[mine - off[i]] = np.diag(S[np.ix_(mine, mine)] - C.T @ W)
    return pred, var


@pytest.mark.parametrize("kind,metric", CASES)
def test_loocv_and_folds(native, kind, metric):
    p, coords, values, d, S, cf = make_data(kind, metric)
    h = handle(native, p, coords, values, metric, d)
    rng = np.random.default_rng(3)
    for i in (0, 1):
        n_i, n_o = len(coords[i]), len(coords[1 - i])
        pred, err = h.loocv(i, n_i)
        rp, rv = dense_folds(p, coords, values, d, metric, i, np.arange(n_i), None, S)
        check(pred, err, rp, rv, f"loocv {kind} {metric} i={i}")
        sd = SCALE[i] * d[i]
        assert np.all(err ** 2 >= sd - 1e-9)   # the withheld observation's own noise is in its variance
        # random tenths over both processes
        fi, fo = rng.integers(0, 10, n_i).astype(np.int32), rng.integers(0, 10, n_o).astype(np.int32)
        info, pred, err = h.cv_folds(i, fi, fo)
        assert info == 0
        rp, rv = dense_folds(p, coords, values, d, metric, i, fi, fo, S)
        check(pred, err, rp, rv, f"tenths {kind} {metric} i={i}")
    # a datum with its co-located partner: process 0 datum 150 + a and process 1 datum a, a < 150
    fi = np.full(N0, -1, dtype=np.int32)
    fo = np.full(N1, -1, dtype=np.int32)
    fi[150:300], fo[:150] = np.arange(150), np.arange(150)
    info, pred, err = h.cv_folds(0, fi, fo)
    assert info == 0
    rp, rv = dense_folds(p, coords, values, d, metric, 0, fi, fo, S)
    sel = fi >= 0
    assert np.array_equal(np.isnan(pred), ~sel)
    check(pred[sel], err[sel], rp[sel], rv[sel], f"partners {kind} {metric}")
    h.close()


# ---- 3. blocks and the verdict ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", CASES)
def test_blocks_and_verify(native, kind, metric):
    p, coords, values, d, S, cf = make_data(kind, metric)
    h = handle(native, p, coords, values, metric, d)
    rng = np.random.default_rng(8)
    for i in (0, 1):
        pc = pred_sites(rng, coords, metric, i, m=60, n_on=10)
        lab = rng.permutation(np.arange(60) % 7).astype(np.int32)
        w = rng.uniform(0.2, 1.0, 60)
        A = np.zeros((7, 60))
        A[lab, np.arange(60)] = w
        rp, rS = dense_predict(p, coords, values, pc, i, metric, cf)
        pred, err, cov = h.predict_blocks(i, pc, lab, w, 7, want_cov=True)
        want = A @ rS @ A.T
        check(pred, err, A @ rp, np.diag(want), f"blocks {kind} {metric} i={i}")
        dc = np.max(np.abs(cov - want))
        print(f"blocks cov {kind} {metric} i={i}: max |d cov| = {dc:.3e}")
        assert dc < 1e-9
        # verify_model against the dense Schur complement: sites on data with s d > 0 do not make it singular
        on = np.array([(coords[i] == c).all(axis=1).any() for c in pc])
        sd = np.array([SCALE[i] * d[i][np.flatnonzero((coords[i] == c).all(axis=1))[0]] if o else np.nan for c, o in zip(pc, on)])
        good = ~on | (sd > 0)
        h.predict(i, pc[good])
        Sg = rS[np.ix_(good, good)]
        ok = np.linalg.eigvalsh(Sg).min() > 1e-10
        assert ok
        assert h.verify_model() == 0
        # (a site on a datum with d = 0 is exactly singular, as without noise: its Schur pivot is pure rounding, and the
        # predictors decide that case on the coordinates -- nothing to assert on the device's verdict)
    h.close()


# ---- 4. conditional simulation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", CASES)
def test_conditional_draws(native, kind, metric):
    p, coords, values, d, S, cf = make_data(kind, metric)
    h = handle(native, p, coords, values, metric, d)
    rng = np.random.default_rng(12)
    for i in (0, 1):
        pos, zero = np.flatnonzero(d[i] > 0)[:8], np.flatnonzero(d[i] == 0)[:5]
        if metric == HAV:
            free = np.column_stack([rng.uniform(26, 49, 20), rng.uniform(-118, -72, 20)])
        else:
            free = np.column_stack([rng.uniform(0.2, 9.8, 20), rng.uniform(0.2, 9.8, 20)])
        pc = np.vstack([coords[i][pos], coords[i][zero], free])
        m = len(pc)
        eps = rng.standard_normal((6, m))
        jit = 1e-10
        draws, pred, err, defl, info = h.conditional_draws(i, pc, 6, noise=eps, jitter=jit)
        assert info == 0
        assert not defl[:8].any(), "sites on data with s d > 0 are not deflated"
        assert defl[8:13].all(), "sites on data with d = 0 are"
        assert not defl[13:].any()
        rp, rS = dense_predict(p, coords, values, pc, i, metric, cf)
        kept = np.flatnonzero(~defl)
        c00 = p.sigma[i] ** 2 + p.nugget[i]
        L = np.linalg.cholesky(rS[np.ix_(kept, kept)] + jit * c00 * np.eye(len(kept)))
        want = np.broadcast_to(rp, (6, m)).copy()
        want[:, kept] += eps[:, kept] @ L.T
        dd = np.max(np.abs(draws - want)) / np.max(np.abs(want))
        print(f"draws {kind} {metric} i={i}: rel = {dd:.3e}")
        assert dd < 1e-8
    h.close()


# ---- 5. nothing set: the same bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("nugget", HAV), ("zero", EUC)])
def test_zero_cleared_and_scale_zero_are_bitwise_off(native, kind, metric):
    p, coords, values, d, S, cf = make_data(kind, metric)
    pc = pred_sites(np.random.default_rng(2), coords, metric, 0)

    def run(setup):
        h = handle(native, p, coords, values, metric, factor=False)
        setup(h)
        h.assemble_joint()
        info, out3, g = h.loglik(True)
        assert info == 0
        pr = h.predict(0, pc)
        h.close()
        return pr[0], pr[1], np.array(out3), g

    base = run(lambda h: None)
    variants = {
        "zeros": lambda h: [h.set_noise(k, np.zeros(len(coords[k]))) for k in range(2)],
        "cleared": lambda h: [(h.set_noise(k, d[k], 2.0), h.set_noise(k, None)) for k in range(2)],
        "scale 0": lambda h: [h.set_noise(k, d[k], 0.0) for k in range(2)],
    }
    for name, setup in variants.items():
        got = run(setup)
        for a, b in zip(base, got):
            assert np.array_equal(a, b), name


# ---- 6. co-located copies ---------------------------------------------------------------------------------------------------
def test_colocated_copies_need_noise(native):
    """two data of one process at identical coordinates with nugget 0: Sigma has two identical rows; measurement error on one
    of them (the true diagonal, by datum index) makes it positive definite.  Six such pairs: the pivot of an exact copy is
    pure rounding, of either sign, and one pair alone would fail to factor only every other time"""
    p, coords, values, d, S, cf = make_data("zero", HAV)
    src = np.array([7, 50, 99, 140, 201, 260])
    c0 = np.vstack([coords[0], coords[0][src]])
    v0 = np.append(values[0], values[0][src] + 0.05)
    cc, vv = [c0, coords[1]], [v0, values[1]]
    h = handle(native, p, cc, vv, HAV, factor=False)
    assert h.factor() != 0
    h.close()
    dn = [np.zeros(N0 + 6), np.zeros(N1)]
    dn[0][N0:] = 0.02
    h = handle(native, p, cc, vv, HAV, dn, scale=(1.0, 1.0), factor=False)
    assert h.factor() == 0
    Sn = orc.joint_cov(p, cc, HAV)
    assert Sn[7, N0] == Sn[7, 7]   # the copies' off-diagonal entry carries no measurement error
    Sn[np.arange(N0, N0 + 6), np.arange(N0, N0 + 6)] += 0.02
    pc = pred_sites(np.random.default_rng(4), coords, HAV, 0)
    rp, rS = dense_predict(p, cc, vv, pc, 0, HAV, cho_factor(Sn, lower=True))
    pred, err = h.predict(0, pc)
    dp = np.max(np.abs(pred - rp) / np.maximum(1.0, np.abs(rp)))
    dv = np.max(np.abs(err ** 2 - np.maximum(np.diag(rS), 0.0)))
    print(f"co-located copies: max |d pred| = {dp:.3e}, max |d pred_err^2| = {dv:.3e}")
    assert dp < 1e-8 and dv < 1e-9
    h.close()


# ---- 7. state rules ---------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(native):
    p, coords, values, d, S, cf = make_data("nugget", HAV)
    pc = pred_sites(np.random.default_rng(2), coords, HAV, 0)
    h = handle(native, p, coords, values, HAV, d)
    a = h.predict(0, pc)
    h.set_noise(0, d[0], 2.0)
    # as after ck_set_model: the factor and the assembled Sigma are gone, so the predictors ask for ck_factor and ck_factor
    # asks for ck_assemble_joint
    with pytest.raises(native.NativeError, match="ck_factor has not been called"):
        h.predict(0, pc)
    with pytest.raises(native.NativeError):
        h.verify_model()
    with pytest.raises(native.NativeError, match="ck_assemble_joint has not been called"):
        h.factor()
    h.set_noise(0, d[0], SCALE[0])
    h.assemble_joint()
    assert h.factor() == 0
    b = h.predict(0, pc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])   # repeated calls give equal bits
    with pytest.raises(native.NativeError, match=r"299 variances for process 0, which has 300"):
        h.set_noise(0, d[0][:-1])
    bad = d[1].copy()
    bad[17] = -1e-3
    with pytest.raises(native.NativeError, match=r"datum 17 of process 1"):
        h.set_noise(1, bad)
    bad[17] = np.nan
    with pytest.raises(native.NativeError, match=r"datum 17 of process 1"):
        h.set_noise(1, bad)
    for s in (-1.0, np.inf, np.nan):
        with pytest.raises(native.NativeError, match=r"scale of process 1"):
            h.set_noise(1, d[1], s)
    with pytest.raises(native.NativeError, match="ck_loglik_noise_grad"):
        h.loglik_noise_grad()
    h.close()
    hp = native.Handle(devices=[0, 0], rank=0)
    hp.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                 p.nugget, p.rho)
    hp.set_data(0, coords[0], values[0])
    with pytest.raises(native.NativeError, match=r"partitioned.*process 0"):
        hp.set_noise(0, d[0])
    hp.close()
    # ck_set_data clears the noise of its process
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(HAV)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
        h.set_noise(k, d[k])
        h.set_data(k, coords[k], values[k])
    h.assemble_joint()
    assert h.factor() == 0
    h0 = handle(native, p, coords, values, HAV)
    x, y = h.predict(0, pc), h0.predict(0, pc)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    h.close()
    h0.close()


def test_predictor_end_to_end(native):
    """Predictor(measurement_error=...): every handle it creates carries the noise, the per-fold ones of refactor_each too"""
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    p, coords, values, d, S, cf = make_data("nugget", HAV)
    mf = fields.MultiField([fields.Field(coords[k], values[k], variance_estimate=d[k]) for k in range(2)])
    mod = model.MultivariateMatern(2)
    mod.params.set_values(PARAMS["nugget", HAV])
    P = joint_prediction.Predictor(mod, mf, measurement_error=True, noise_scale=SCALE)
    pc = pred_sites(np.random.default_rng(2), coords, HAV, 0)
    pred, err = P.predict_arrays(0, pc)
    rp, rS = dense_predict(p, coords, values, pc, 0, HAV, cf)
    check(pred, err, rp, np.diag(rS), "Predictor")
    P0 = joint_prediction.Predictor(mod, mf)
    assert P._state_key() != P0._state_key()
    fi = (np.arange(N0) % 3).astype(np.int32)
    fast = P.cross_validation(0, postprocess=False, folds=fi)
    slow = P.cross_validation(0, postprocess=False, folds=fi, refactor_each=True)
    assert np.max(np.abs(fast["pred"].values - slow["pred"].values)) < 1e-8
    # refactor_each predicts the field at the withheld site, the one-factorisation form the withheld observation
    sd = pd_sorted_noise(fast, coords[0], SCALE[0] * d[0])
    assert np.max(np.abs(fast["pred_err"].values ** 2 - (slow["pred_err"].values ** 2 + sd))) < 1e-9
    P.close()
    P0.close()


def pd_sorted_noise(frame, coords, sd):
    """s d of the frame's rows (the frame is sorted by the coordinates)"""
    look = {tuple(c): v for c, v in zip(coords, sd)}
    return np.array([look[(a, b)] for a, b in zip(frame["d1"].values, frame["d2"].values)])
