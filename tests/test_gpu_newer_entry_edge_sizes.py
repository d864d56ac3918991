"""GPU tests of ck_loglik_fisher, ck_cv_folds and ck_set_noise at the sizes their kernels index by -- the treatment
tests/test_gpu_entry_edge_sizes.py gives the older entry points: data sets below a tile, on and around the 64-row strips
(n0p = roundup(n0, 64)), with the process boundary on a 128-column tile edge, inside a tile, on a 512-wide panel edge and in
the middle panel of three, a process of one site, one process down to N = 1.  The references are the dense float64 chains
of tests/dense_chains.py (dense_fisher, dense_folds and the likelihood chains with Sigma + diag(s d)); their own floors,
identities and sensitivity to boundary errors are checked on the host in tests/test_dense_chains.py.

Geometry of the Fisher units (ck_api.hip, "geometry of the units") on the rungs:
  n0p = 64    (1, 1) (5, 3) (63, 65) (64, 64) (64, 1) (1, 600)   boundary mid-tile, one panel (process 0 one column wide at n0 = 1)
  n0p = 448   (448, 64)                                          wpad[0] = 512 rounds up into process 1's columns
  n0p = 512   (449, 63) (511, 1) (512, 512)                      pK0[1] = 1, npan[0] = 1: process 1 starts a panel
  n0p = 576   (513, 511) (576, 100)                              boundary mid-tile in the second panel; (513, 511): Npad = 1536
Kernels and the tests that launch them at n0p in {64, 448, 512, 576}, n1 = 1 and Npad = 1536:
  k_fisher_expand, k_fisher_assemble, k_fisher_prod, k_fisher_contract     test_fisher_on_the_ladder (every rung)
  k_fisher_dh, k_fisher_ytv                                                test_fisher_reml_on_the_ladder, test_fisher_with_noise
  k_fisher_dh_diag                                                         test_fisher_with_noise (REML), test_fisher_grouped_products_...
  grouped contraction with diagonal operands                               test_fisher_grouped_products_with_everything_on
  k_fold_gram, k_fold_small, k_fold_big_fill, k_fold_big_reduce, the batched factorisation
                                                                           test_folds_on_the_ladder, test_big_fold_sizes
(n1 = 1: the rungs (64, 1) and (511, 1); Npad = 1536: (513, 511) and REFIT (700, 650)).

Bounds.  Fisher, in normalised()'s measure, per class of pairs: exact slots 1e-9 and nu slots 1e-6 (tests/test_gpu_fisher.py);
a length-scale slot with an exact or length-scale slot max(1e-9, 10 x the reference's floor) = 1e-9 on every rung (the floors
are in tests/test_dense_chains.py: at most 3.2e-11).  Folds: 1e-8 max(1, |pred|), 1e-9 on pred_err^2
(tests/test_gpu_cv_folds.py: check), the statistics 1e-8 max(1, |.|).  Noise: the bounds of test_loglik_and_gradient, 1e-9 for
the noise-scale gradient and the predictor.

REML on a rung with a process of one site: ck_set_trend refuses more columns than a process has data ("has 1 data sites
for 3 regressors" -- asserted), so that process gets the constant design.  Its unit vector then lies in the span of X, P
annihilates every derivative supported on that site (dense_chains.annihilated_slots), and those slots are held to 0 in the
scale of the ML information (1e-9, the exact class) on both sides.  The same holds for process 1 of (5, 3) under the linear
design: three sites, three columns.

Largest deviations seen on an MI355X over all cases of this file (the tests print them per case):
  Fisher, ML and with noise   exact 8.8e-14, length scale 3.3e-11 (the reference's floor there is 3.2e-11), nu 4.3e-10
  Fisher, REML                exact 4.5e-14, length scale 1.0e-11, nu 1.8e-10; annihilated slots 1.3e-14 of the ML scale
  the two site orders         6.4e-14; grouped (9 groups) against ungrouped: the same bits; masked against full: 0
  folds on the ladder         pred 5.3e-13, pred_err^2 2.0e-13, log|Q_SS| and the quadratic form 2.7e-13
  big folds (65 .. 1025)      pred 3.9e-13, pred_err^2 4.0e-14, statistics 2.2e-13
  noise at ragged sizes       l, log|Sigma|, quadratic form 1.9e-14; gradient 1.3e-10; noise-scale gradient 3.6e-14;
                              predictor 4.7e-14 / 6.8e-15; folds 1.3e-13 / 1.3e-13 / 1.6e-13
No bound was fitted to these numbers: each was set before the first run.
"""
import functools

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc
from tests import dense_chains as dc
from tests.test_gpu_entry_edge_sizes import GRAD_TOL, case_id, err, handle, native, same  # noqa: F401 (native: the fixture)

pytestmark = pytest.mark.gpu


def sizes(ds):
    return [len(c) for c in ds.coords]


def bits(x):
    """floats as their bit patterns (NaN compares equal to itself), through tuples"""
    if isinstance(x, (tuple, list)):
        return tuple(bits(y) for y in x)
    if x is None:
        return None
    a = np.ascontiguousarray(np.asarray(x))
    return a.astype(np.float64).view(np.uint64) if a.dtype.kind == "f" else a


def noisy_sigma(ds, d, scales=dc.NOISE_SCALES):
    dv = np.concatenate([scales[k] * d[k] if d[k] is not None else np.zeros(len(ds.coords[k])) for k in range(ds.p.n_procs)])
    return ds.S + np.diag(dv)


def set_noise(h, d, scales=dc.NOISE_SCALES):
    for k, x in enumerate(d):
        if x is not None:
            h.set_noise(k, x, scales[k])
    h.assemble_joint()


def designs(ds, kinds):
    return [dc.design(k, c, c) for k, c in zip(kinds, ds.coords)]


@functools.lru_cache(maxsize=None)
def derivatives(case):
    """D_k of a data set over all 13 slots (the noise variances of every process), once: the Bessel evaluations"""
    ds = dc.data_set(case)
    return dc.derivative_matrices(ds.params, ds.coords, ds.metric, noise=dc.noise_of(ds))


@functools.lru_cache(maxsize=None)
def fisher_ref(case, which=None, kinds=None):
    """dense_fisher of a data set (noise on the processes `which`, REML with the designs `kinds`) on the kept D_k"""
    ds = dc.data_set(case)
    X = dc.block_X(designs(ds, kinds)) if kinds else None
    D = {k: Dk for k, Dk in derivatives(case).items() if k < 11 or (which is not None and k - 11 in which)}
    S = dc.dense_sigma(ds.params, ds.coords, ds.metric, dc.noise_of(ds, which) if which else None, dc.NOISE_SCALES)
    return dc.fisher_of(S, D, X)


def check_fisher(I, ref, case, what, gone=()):
    """the class bounds of dense_chains.fisher_tol in normalised()'s measure; dead slots exactly 0; `gone`: see the header"""
    ds = dc.data_set(case)
    gone = list(gone)
    if gone:
        ml = fisher_ref(case)
        zi, zr = dc.ml_scaled(I, ml, gone), dc.ml_scaled(ref, ml, gone)
        print(f"{what}: annihilated slots {gone} in the ML scale: library {zi:.2e}, reference {zr:.2e}")
        assert zi <= 1e-9 and zr <= 1e-9
        I, ref = dc.drop_slots(I, gone), dc.drop_slots(ref, gone)
    dead = [k for k in range(13) if ref[k, k] == 0.0 and k not in gone]
    assert np.all(I[dead] == 0.0) and np.all(I[:, dead] == 0.0), (what, dead, I[dead])
    e = dc.class_errors(dc.normalised(I, ref), len(ds.params))
    tol = dc.fisher_tol(case)
    print(f"{what}: fisher exact {e['exact']:.2e} length scale {e['len']:.2e} nu {e['nu']:.2e} (dead slots {dead})")
    for c in ("exact", "len", "nu"):
        assert e[c] <= tol[c], (what, c, e[c], tol[c])
    return dead


def structure(h, **kw):
    """two calls: info 0, symmetric to the bit, the same bits"""
    info, I = h.fisher(**kw)
    info2, I2 = h.fisher(**kw)
    assert info == 0 and info2 == 0
    assert np.array_equal(I, I.T)
    assert np.array_equal(I, I2)
    return I


def orders_agree(Is, ref, what, skip=()):
    live = np.array([k for k in np.flatnonzero(np.diag(ref) > 0) if k not in skip], dtype=int)
    d = np.sqrt(np.outer(np.diag(Is[0])[live], np.diag(Is[0])[live]))
    e = (np.abs(Is[0] - Is[1])[np.ix_(live, live)] / d).max() if len(live) else 0.0
    print(f"{what}: site orders differ by {e:.2e}")
    assert e <= 1e-10


# ---- 1. Fisher information on the ladder --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.FISHER_CASES, ids=case_id)
def test_fisher_on_the_ladder(native, case):
    ds = dc.data_set(case)
    ref = fisher_ref(case)
    Is = []
    for so in (1, 0):
        h = handle(native, ds, so, factor=False)
        Is.append(structure(h))
        h.close()
        dead = check_fisher(Is[-1], ref, case, f"{case} site_order {so}")
    n = sizes(ds)
    want = [11, 12] + (list(range(4, 11)) if len(n) == 1 else [])   # no noise; one process: four parameters
    if len(n) == 1:
        want += [1, 2] if n[0] == 1 else []
    else:   # nu and len of a one-site process, nu_12 and len_12 at rho = 0: identically 0
        want += ([2, 5] if n[0] == 1 else []) + ([4, 7] if n[1] == 1 else []) + ([3, 6] if ds.p.rho == 0.0 else [])
    assert sorted(dead) == sorted(want)
    orders_agree(Is, ref, str(case))


# ---- 2. REML ---------------------------------------------------------------------------------------------------------------------
FISHER_REML = ([(c, kind) for c in dc.FIVE_RUNGS for kind in ("constant", "linear")] + [(c, "wide") for c in dc.FISHER_WIDE])


@pytest.mark.parametrize("case,kind", FISHER_REML, ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_fisher_reml_on_the_ladder(native, case, kind):
    ds = dc.data_set(case)
    kinds = tuple(dc.trend_kinds(ds, kind))
    assert kinds == (kind,) * ds.p.n_procs   # every process of these rungs has the data for the design
    Fs = designs(ds, kinds)
    assert kind != "wide" or sum(F.shape[1] for F in Fs) == 16
    ref = fisher_ref(case, None, kinds)
    gone = dc.annihilated_slots(sizes(ds), kinds)   # (5, 3) "linear": process 1 has three sites for three columns
    assert bool(gone) == (case[:2] == (5, 3) and kind == "linear")
    Is = []
    for so in (1, 0):
        h = handle(native, ds, so, factor=False)
        for k, F in enumerate(Fs):
            h.set_trend(k, F)
        Is.append(structure(h, reml=True))
        h.close()
        check_fisher(Is[-1], ref, case, f"{case} REML {kind} site_order {so}", gone)
    orders_agree(Is, ref, f"{case} REML {kind}", gone)


# ---- 3. noise scales ---------------------------------------------------------------------------------------------------------------
FISHER_NOISE = [(c, which, reml) for c in dc.FISHER_NOISE_CASES for which in ((0,), (0, 1)) for reml in (False, True)
                if c[1] > 0 or which == (0,)]


def set_linear_trend(native, h, ds):
    """"linear" where the process has the data for it; where it has not the library refuses it and "constant" is used"""
    kinds = tuple(dc.trend_kinds(ds, "linear"))
    for k, kind in enumerate(kinds):
        if kind != "linear":
            n_k = len(ds.coords[k])
            with pytest.raises(native.NativeError, match=f"process {k} has {n_k} data sites for 3 regressors"):
                h.set_trend(k, np.ones((n_k, 3)))
        h.set_trend(k, dc.design(kind, ds.coords[k], ds.coords[k]))
    return kinds


@pytest.mark.parametrize("case,which,reml", FISHER_NOISE,
                         ids=lambda v: case_id(v) if isinstance(v, tuple) and len(v) == 5 else str(v))
def test_fisher_with_noise(native, case, which, reml):
    ds = dc.data_set(case)
    d = dc.noise_of(ds, which)
    Is = []
    for so in (1, 0):
        h = handle(native, ds, so, factor=False)
        kinds = set_linear_trend(native, h, ds) if reml else None
        set_noise(h, d)
        Is.append(structure(h, reml=reml))
        h.close()
        ref = fisher_ref(case, which, kinds)
        gone = dc.annihilated_slots(sizes(ds), kinds)
        check_fisher(Is[-1], ref, case, f"{case} noise on {which} {'REML' if reml else 'ML'} site_order {so}", gone)
        for k in range(2):
            if 11 + k not in gone:
                assert (Is[-1][11 + k, 11 + k] > 0) == (k in which and k < ds.p.n_procs)
    orders_agree(Is, ref, f"{case} noise {which} reml={reml}", gone)


# ---- 4. grouped products with diagonal operands and REML ---------------------------------------------------------------------------
def test_fisher_grouped_products_with_everything_on(native):
    ds = dc.data_set(dc.LARGE)
    d = dc.noise_of(ds)
    h = handle(native, ds, factor=False)
    kinds = set_linear_trend(native, h, ds)
    set_noise(h, d)
    info, I = h.fisher(reml=True)
    assert info == 0 and h.fisher_timings()["groups"] == 1
    check_fisher(I, fisher_ref(dc.LARGE, (0, 1), kinds), dc.LARGE, "everything on, one group")
    h.set_option("fisher_product_mb", 40)   # Npad = 1536: a cross product is 18 MiB, those of process 0 / 1 7.5 / 12 MiB
    info, Ig = h.fisher(reml=True)
    t = h.fisher_timings()
    print("groups", t["groups"])
    assert info == 0 and t["groups"] >= 3
    assert np.array_equal(I, Ig)
    sub = [0, 5, 10, 11, 12]
    free = np.zeros(13, dtype=bool)
    free[sub] = True
    off = [k for k in range(13) if k not in sub]
    for mb in (40, 0):   # the mask on the grouped and on the ungrouped schedule
        h.set_option("fisher_product_mb", mb)
        info, Im = h.fisher(reml=True, free=free)
        assert info == 0
        assert np.all(Im[off] == 0.0) and np.all(Im[:, off] == 0.0)
        e = (np.abs(I - Im)[np.ix_(sub, sub)] / np.sqrt(np.outer(np.diag(I), np.diag(I)))[np.ix_(sub, sub)]).max()
        print(f"fisher_product_mb {mb}: masked against full {e:.2e}, groups {h.fisher_timings()['groups']}")
        assert e <= 1e-12
    h.close()


# ---- 5. leave-group-out folds on the ladder ------------------------------------------------------------------------------------------
def check_folds(out, ref, what):
    info, pred, e, stats = out
    rp, rv, rs = ref
    assert info == 0, what
    sel = ~np.isnan(rp)
    assert np.array_equal(np.isnan(pred), ~sel) and np.array_equal(np.isnan(e), ~sel), what
    dp = np.max(np.abs(pred[sel] - rp[sel]) / np.maximum(1.0, np.abs(rp[sel])))
    dv = np.max(np.abs(e[sel] ** 2 - rv[sel]))
    assert np.array_equal(stats[:, 0], rs[:, 0]), (what, stats[:, 0], rs[:, 0])
    dst = np.max(np.abs(stats[:, 1:] - rs[:, 1:]) / np.maximum(1.0, np.abs(rs[:, 1:])))
    print(f"{what}: folds {[int(s) for s in rs[:, 0]]}: pred {dp:.2e} pred_err^2 {dv:.2e} log|Q_SS|, quadratic form {dst:.2e}")
    assert dp < 1e-8, what
    assert dv < 1e-9, what
    assert dst < 1e-8, what


def run_folds(h, S, ds, calls, what):
    """every call (i, fi, fo) twice -- the same bits -- against dense_folds on S"""
    refs = dc.folds_references(S, ds.z, sizes(ds), calls)
    for (i, fi, fo), ref in zip(calls, refs):
        out = h.cv_folds(i, fi, fo, want_stats=True)
        check_folds(out, ref, f"{what} i={i}")
        assert same(bits(h.cv_folds(i, fi, fo, want_stats=True)), bits(out)), what
        assert same(bits(h.cv_folds(i, fi, fo)), bits(out[:3])), what


def ladder_calls(case, i):
    n_procs = 2 if case[1] > 0 else 1
    return [(i,) + dc.fold_labels(case, i, other, minus)[:2] for other, minus in dc.FOLD_VARIANTS if n_procs == 2 or not other] \
        + ([(i,) + dc.fold_labels(case, i, False, True)[:2]] if n_procs == 1 else [])


@pytest.mark.parametrize("case,i", dc.FOLD_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else f"i{v}")
def test_folds_on_the_ladder(native, case, i):
    ds = dc.data_set(case)
    pc = dc.pred_sites(np.random.default_rng(3), ds.metric, 40)
    f = handle(native, ds)
    want = f.predict(i, pc)
    f.close()
    h = handle(native, ds)
    run_folds(h, ds.S, ds, ladder_calls(case, i), str(case))
    assert same(h.predict(i, pc), want)   # afterwards: the bits of a handle that never saw the call
    h.close()


# ---- 6. big-fold sizes -------------------------------------------------------------------------------------------------------------
BIG_FOLDS = {dc.REFIT: [[65, 127, 128, 129], [191, 192, 193, 255], [256, 257, 321], [1024], [1025], [1, 63, 64, 65, 320]],
             # the univariate half has 700 data: the lists that fit, the longest cut into two calls
             dc.REFIT_UNI: [[65, 127, 128, 129], [191, 192, 193], [255, 256], [257, 321], [1, 63, 64, 65, 320]]}


@pytest.mark.parametrize("case,i", [(dc.REFIT, 0), (dc.REFIT, 1), (dc.REFIT_UNI, 0)], ids=lambda v: case_id(v) if isinstance(v, tuple) else f"i{v}")
def test_big_fold_sizes(native, case, i):
    """several folds per call, so the batch holds systems of unequal kq; the members scattered by a permutation over both
    processes, so every big fold spans all three panels"""
    ds = dc.data_set(case)
    n = sizes(ds)
    rng = np.random.default_rng(60 + i)
    calls = [(i,) + dc.labels_from_sizes(rng, n, i, sz)[:2] for sz in BIG_FOLDS[case]]
    if len(n) == 2:
        for (_, fi, fo), sz in zip(calls, BIG_FOLDS[case]):
            assert max(sz) < 65 or ((fi == int(np.argmax(sz))).any() and (fo == int(np.argmax(sz))).any())
    h = handle(native, ds)
    run_folds(h, ds.S, ds, calls, f"{case} big folds")
    h.close()


# ---- 7. the row window of the unit right-hand sides ---------------------------------------------------------------------------------
@pytest.mark.parametrize("site_order", [0, 1])
def test_fold_row_window(native, site_order):
    ds = dc.data_set(dc.LARGE)
    n = sizes(ds)
    h = handle(native, ds, site_order)
    calls = []
    for i in (0, 1):
        perm = h.debug_site_order(i, n[i])
        assert sorted(perm) == list(range(n[i])) and (site_order == 1 or list(perm) == list(range(n[i])))
        for a in (perm[-1], perm[0]):   # only the last internal position of process i withheld; only the first
            fi = np.full(n[i], -1, dtype=np.int32)
            fi[a] = 0
            calls += [(i, fi, None), (i, fi, np.full(n[1 - i], -1, dtype=np.int32))]
        # the first and the last datum of the stacked order in one fold: labels on both processes
        fi, fo = np.full(n[i], -1, dtype=np.int32), np.full(n[1 - i], -1, dtype=np.int32)
        (fi if i == 0 else fo)[0] = 0
        (fo if i == 0 else fi)[-1] = 0
        calls.append((i, fi, fo))
    run_folds(h, ds.S, ds, calls, f"row window site_order {site_order}")
    for a, b in ((0, 1), (2, 3), (5, 6), (7, 8)):   # no labels on the other process and labels of -1 throughout: the same bits
        x, y = (h.cv_folds(*calls[k], want_stats=True) for k in (a, b))
        assert same(bits(x), bits(y))
    h.close()


# ---- 8. noise at ragged sizes on the older entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.NOISE_CASES, ids=case_id)
def test_noise_at_ragged_sizes(native, case):
    ds = dc.data_set(case)
    n = sizes(ds)
    d = dc.noise_of(ds)
    Sn = noisy_sigma(ds, d)
    ref = dc.dense_ll(ds.params, ds.coords, ds.values, ds.metric, S=Sn)
    gref = dc.dense_ll_grad(ds.params, ds.coords, ds.values, ds.metric, S=Sn)
    Si = np.linalg.inv(Sn)
    Si = 0.5 * (Si + Si.T)
    a = Si @ ds.z
    w = 0.5 * (a * a - np.diag(Si)) * np.concatenate(d)
    rs = np.array([w[:n[0]].sum(), w[n[0]:].sum()])
    cf = cho_factor(Sn, lower=True)
    for so in (1, 0):
        h = handle(native, ds, so, factor=False)
        set_noise(h, d)
        info, v, g = h.loglik(True)
        assert info == 0
        gs = h.loglik_noise_grad()
        print(f"{case} site_order {so}: l, log|Sigma|, quad rel {[abs(x - y) / abs(y) for x, y in zip(v, ref)]}, gradient "
              f"{err(g, gref):.2e}, noise-scale gradient {err(gs, rs):.2e}")
        for x, y in zip(v, ref):
            assert abs(x - y) <= 1e-8 * abs(y), (so, v, ref)
        assert err(g, gref) < GRAD_TOL, (so, g, gref)
        assert err(gs, rs) < 1e-9, (so, gs, rs)
        for i in (0, 1):
            pc = dc.pred_sites(np.random.default_rng(129 + i), ds.metric, 129)
            pred, e = h.predict(i, pc)
            c0 = orc.pred_cross_cov(ds.p, ds.coords, pc, i, ds.metric)   # the field's: no measurement error in c0 or c00
            rp = c0.T @ cho_solve(cf, ds.z)
            rv = np.diag(orc.pred_cov(ds.p, pc[:1], i, ds.metric))[0] - np.sum(c0 * cho_solve(cf, c0), axis=0)
            print(f"    predict i={i}: pred {dc.rel(pred, rp):.2e} pred_err^2 {np.max(np.abs(e ** 2 - rv)):.2e}")
            assert dc.rel(pred, rp) < 1e-9 and np.max(np.abs(e ** 2 - rv)) < 1e-9
        run_folds(h, Sn, ds, [c for i in (0, 1) for c in ladder_calls(case, i)], f"{case} noisy folds site_order {so}")
        h.close()


@pytest.mark.parametrize("case", dc.NOISE_CASES, ids=case_id)
def test_noise_that_is_not_there_changes_no_bit(native, case):
    """a vector of zeros, a scale of 0 and a cleared vector: the bits of a handle that never saw ck_set_noise"""
    ds = dc.data_set(case)
    d = dc.noise_of(ds)
    pc = dc.pred_sites(np.random.default_rng(8), ds.metric, 129)

    def results(h):
        # the factor of the first call stays resident.  Of the information the 11 model parameters: a noise-scale slot
        # is live whenever its process has a vector (include/cokrige.h), zeros and a scale of 0 included
        out = [h.loglik(True), h.fisher()[1][:11, :11]]
        return out + [h.predict(i, pc) for i in (0, 1)] + [h.cv_folds(*c, want_stats=True) for c in ladder_calls(case, 1)]

    h = handle(native, ds, factor=False)
    want = bits(results(h))
    h.close()
    for what in ("zeros", "scale 0", "cleared"):
        h = handle(native, ds, factor=False)
        for k in range(2):
            if what == "zeros":
                h.set_noise(k, np.zeros(len(d[k])), dc.NOISE_SCALES[k])
            else:
                h.set_noise(k, d[k], 0.0 if what == "scale 0" else dc.NOISE_SCALES[k])
        if what == "cleared":
            h.assemble_joint()
            assert h.loglik(False)[0] == 0   # the noise was in Sigma once
            for k in range(2):
                h.set_noise(k, None)
        h.assemble_joint()
        assert same(bits(results(h)), want), what
        h.close()


# ---- 9. a sequence on one handle --------------------------------------------------------------------------------------------------------
def test_sequence_of_the_newer_entry_points(native):
    """every call of the sequence gives the bits of the same call on a fresh handle in that state: plain (assembled and
    factored), noisy (noise set, assembled) or noisy and factored"""
    ds = dc.data_set(dc.LARGE)
    d = dc.noise_of(ds)
    F = designs(ds, ("linear", "linear"))
    _, fi, fo = ladder_calls(dc.LARGE, 0)[2]
    rng = np.random.default_rng(9)
    pc = dc.pred_sites(rng, ds.metric, 300)
    lab, w = dc.block_labels(rng, 7, 300), rng.uniform(0.2, 2.0, 300)

    def noise_on(h):
        set_noise(h, d)

    def noise_off(h):
        for k in range(2):
            h.set_noise(k, None)
        h.assemble_joint()
        return h.factor()

    def fisher_reml(h):
        for k in range(2):
            h.set_trend(k, F[k])
        return h.fisher(reml=True)

    def fresh(state):
        f = handle(native, ds, factor=state == "plain")
        if state != "plain":
            noise_on(f)
            if state == "noisy, factored":
                assert f.factor() == 0
        return f

    steps = [("fisher ML", "plain", lambda h: h.fisher()),
             ("cv_folds", "plain", lambda h: h.cv_folds(0, fi, fo, want_stats=True)),
             ("set_noise, assemble", None, noise_on),
             ("fisher REML", "noisy", fisher_reml),
             ("loglik", "noisy", lambda h: h.loglik(True)),
             ("cv_folds with noise", "noisy, factored", lambda h: h.cv_folds(0, fi, fo, want_stats=True)),
             ("noise cleared, assemble, factor", None, noise_off),
             ("predict_blocks", "plain", lambda h: h.predict_blocks(1, pc, lab, w, 7, want_cov=True)),
             ("fisher ML again", "plain", lambda h: h.fisher())]
    h = handle(native, ds)
    got = {}
    for name, state, step in steps:
        got[name] = step(h)
        if state is None:
            continue
        f = fresh(state)
        want = step(f)
        f.close()
        assert same(bits(got[name]), bits(want)), name
    assert got["noise cleared, assemble, factor"] == 0
    assert same(bits(got["fisher ML again"]), bits(got["fisher ML"]))
    assert not same(bits(got["cv_folds with noise"]), bits(got["cv_folds"]))   # the noise reached the folds
    h.close()
