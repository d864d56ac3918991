"""GPU tests of leave-group-out cross-validation from one factorisation: include/cokrige.h ck_cv_folds,
native.Handle.cv_folds and Predictor.cross_validation(folds=..., also_withhold=...).

Truth: for every fold the fold's data are removed on the host and the CPU oracle's joint_predict runs at the withheld sites of
the predicted process -- one dense solve per fold.  Bounds: those test_gpu_properties.py holds ck_loocv to against the oracle,
|d pred| < 1e-8 max(1, |pred|) and |d pred_err^2| < 1e-9.

n0 = 300, n1 = 290: N = 590 spans two 512-column panels, fold members straddle the panel edge and, with random labels,
interleave in the internal (Hilbert) site order.

Largest deviations seen on an MI355X over all cases of this file: |d pred| / max(1, |pred|) = 1.4e-12 and |d pred_err^2| = 4.8e-14
(both with zero nugget, Euclidean); singleton folds against ck_loocv 3.0e-15 / 1.2e-15; fold statistics equal to 12 digits.

Not tested: a fold whose Q_SS cannot factor (info = 1 + fold).  Q_SS is a principal block of Sigma^-1 and so positive
definite whenever Sigma factors; the input proposed for it -- two data of one process at identical coordinates with nugget 0 --
makes Sigma itself exactly singular (two identical rows; the model has one nugget per process, none per copy), and the CPU
oracle's factorisation of that Sigma fails or passes by rounding alone.  No input was found that factors Sigma and not Q_SS."""
import warnings

import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests.dense_chains import oracle_folds   # the slow truth: one refit per fold through the oracle's joint_predict

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
_cache = {}


def make_data(kind, metric):
    """sites of two processes, 150 of process 1 co-located with process 0 (process 1 datum a sits on process 0 datum 150 + a
    for a < 150), values drawn from the model; computed once per case"""
    key = (kind, metric)
    if key not in _cache:
        rng = np.random.default_rng(17 + 2 * metric + (kind == "zero"))
        p = orc.Params.from_flat(PARAMS[key])
        tot = N0 + N1
        if metric == HAV:
            pts = np.column_stack([rng.uniform(25, 50, tot), rng.uniform(-120, -70, tot)])
        else:
            pts = np.column_stack([rng.uniform(0, 10, tot), rng.uniform(0, 10, tot)])
        coords = [pts[:N0].copy(), pts[N0 // 2:N0 // 2 + N1].copy()]
        S = orc.joint_cov(p, coords, metric)
        z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
        _cache[key] = (p, coords, [z[:N0].copy(), z[N0:].copy()], S)
    return _cache[key]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def handle(native, p, coords, values, metric):
    h = native.Handle(0)
    h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                p.nugget, p.rho)
    h.set_metric(metric)
    for k in range(2):
        h.set_data(k, coords[k], values[k])
    h.assemble_joint()
    assert h.factor() == 0
    return h


def check(pred, err, rp, re, what):
    sel = ~np.isnan(rp)
    assert np.array_equal(np.isnan(pred), ~sel), what
    dp = np.max(np.abs(pred[sel] - rp[sel]) / np.maximum(1.0, np.abs(rp[sel])))
    dv = np.max(np.abs(err[sel] ** 2 - re[sel] ** 2))
    print(f"{what}: max |d pred| / max(1, |pred|) = {dp:.3e}, max |d pred_err^2| = {dv:.3e}")
    assert dp < 1e-8, what
    assert dv < 1e-9, what


def labels_of_sizes(rng, n, sizes):
    """random labels: fold f gets sizes[f] data, the last fold the rest"""
    lab = np.repeat(np.arange(len(sizes) + 1), list(sizes) + [n - sum(sizes)]).astype(np.int32)
    return lab[rng.permutation(n)]


@pytest.mark.parametrize("kind,metric", CASES)
def test_truth_random_fold_sizes(native, kind, metric):
    """1. fold sizes 1, 2, 63, 64, 65, 130 and the rest (265) over the 590 data of both processes, assigned at random: the
    members interleave in the internal order and straddle the panel edge"""
    p, coords, values, _ = make_data(kind, metric)
    rng = np.random.default_rng(1)
    lab = np.full(N0 + N1, 6, dtype=np.int32)
    first = rng.permutation(N0)[:2]                      # folds 0 and 1 need a datum of the predicted process
    rest = np.setdiff1d(rng.permutation(N0 + N1), first, assume_unique=True)
    lab[first[0]], lab[first[1]], lab[rest[0]] = 0, 1, 1
    at = 1
    for f, sz in ((2, 63), (3, 64), (4, 65), (5, 130)):
        lab[rest[at:at + sz]] = f
        at += sz
    fi, fo = lab[:N0].copy(), lab[N0:].copy()
    assert all((fi == f).any() for f in range(7))
    h = handle(native, p, coords, values, metric)
    try:
        info, pred, err, stats = h.cv_folds(0, fi, fo, want_stats=True)
        assert info == 0
        assert np.array_equal(stats[:, 0], [1, 2, 63, 64, 65, 130, 265])
        rp, re = oracle_folds(p, coords, values, metric, 0, fi, fo)
        check(pred, err, rp, re, f"truth {kind} metric {metric}")
        # the other process, with some data never withheld
        f1 = labels_of_sizes(rng, N1, [3, 70, 100]).astype(np.int32)
        f1[f1 == 3] = -1
        info, pred, err = h.cv_folds(1, f1, None)
        assert info == 0
        rp, re = oracle_folds(p, coords, values, metric, 1, f1, None)
        check(pred, err, rp, re, f"truth process 1 {kind} metric {metric}")
    finally:
        h.close()


@pytest.mark.parametrize("kind,metric", CASES)
def test_both_processes_withheld(native, kind, metric):
    """2. also_withhold removes the co-located partner"""
    p, coords, values, _ = make_data(kind, metric)
    rng = np.random.default_rng(2)
    fi = labels_of_sizes(rng, N0, [5, 40, 64, 90])
    fo = np.full(N1, -1, dtype=np.int32)
    fo[:150] = fi[150:300]            # process 1 datum a sits on process 0 datum 150 + a
    h = handle(native, p, coords, values, metric)
    try:
        info, pred, err, stats = h.cv_folds(0, fi, fo, want_stats=True)
        assert info == 0
        sizes = np.bincount(fi, minlength=5) + np.bincount(fo[fo >= 0], minlength=5)
        assert np.array_equal(stats[:, 0], sizes)
        rp, re = oracle_folds(p, coords, values, metric, 0, fi, fo)
        check(pred, err, rp, re, f"both {kind} metric {metric}")
        _, pred1, _ = h.cv_folds(0, fi, None)
        if kind == "zero":   # the partner's value at the same place carries most of the information: the labels reach the device
            assert np.max(np.abs(pred1[150:] - pred[150:])) > 1e-3
    finally:
        h.close()


@pytest.mark.parametrize("kind,metric", [("nugget", EUC), ("zero", HAV)])
def test_process_one_with_partners_of_process_zero(native, kind, metric):
    """2, the other way round: process 1 is predicted (its labels are the C call's fold1) and the co-located data of process 0
    leave with its folds (fold0); folds of 3, 64, 65 and 158 data of process 1, some of process 0 never withheld"""
    p, coords, values, _ = make_data(kind, metric)
    rng = np.random.default_rng(9)
    f1 = labels_of_sizes(rng, N1, [3, 64, 65])
    f0 = np.full(N0, -1, dtype=np.int32)
    f0[150:300] = f1[:150]            # process 0 datum 150 + a sits on process 1 datum a
    h = handle(native, p, coords, values, metric)
    try:
        info, pred, err, stats = h.cv_folds(1, f1, f0, want_stats=True)
        assert info == 0
        assert np.array_equal(stats[:, 0], np.bincount(f1, minlength=4) + np.bincount(f0[f0 >= 0], minlength=4))
        rp, re = oracle_folds(p, coords, values, metric, 1, f1, f0)
        check(pred, err, rp, re, f"process 1 with partners {kind} metric {metric}")
        _, pred1, _ = h.cv_folds(1, f1, None)
        if kind == "zero":
            assert np.max(np.abs(pred1[:150] - pred[:150])) > 1e-3
    finally:
        h.close()


@pytest.mark.parametrize("kind,metric", [("nugget", HAV), ("zero", EUC)])
def test_singletons_are_loocv(native, kind, metric):
    """3. every datum its own fold"""
    p, coords, values, _ = make_data(kind, metric)
    h = handle(native, p, coords, values, metric)
    try:
        for i, n in ((0, N0), (1, N1)):
            info, pred, err, stats = h.cv_folds(i, np.random.default_rng(3).permutation(n).astype(np.int32), None, want_stats=True)
            assert info == 0 and np.array_equal(stats[:, 0], np.ones(n))
            lp, le = h.loocv(i, n)
            check(pred, err, lp, le, f"singletons process {i} {kind}")
    finally:
        h.close()


@pytest.mark.parametrize("kind,metric", [("nugget", EUC), ("zero", HAV)])
def test_large_folds_and_refactor_each(native, kind, metric):
    """4. folds of 129 and 100 + 71 (both processes) members: the batched path; against the oracle and refactor_each=True"""
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    p, coords, values, _ = make_data(kind, metric)
    rng = np.random.default_rng(4)
    fi = labels_of_sizes(rng, N0, [129, 100])
    fi[fi == 2] = -1
    fo = np.full(N1, -1, dtype=np.int32)
    fo[rng.permutation(N1)[:71]] = 1
    h = handle(native, p, coords, values, metric)
    try:
        info, pred, err, stats = h.cv_folds(0, fi, fo, want_stats=True)
        assert info == 0 and np.array_equal(stats[:, 0], [129, 171])
        rp, re = oracle_folds(p, coords, values, metric, 0, fi, fo)
        check(pred, err, rp, re, f"large {kind} metric {metric}")
    finally:
        h.close()
    mod = model.MultivariateMatern(2)
    mod.params.set_values(np.asarray(PARAMS[(kind, metric)]))
    mf = fields.MultiField([fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])])
    P = joint_prediction.Predictor(mod, mf, fast_dist=metric == HAV, dist_units="km" if metric == HAV else None)
    try:
        lab = [None if f < 0 else ("a", "b")[f] for f in fi]
        lab_o = [None if f < 0 else "b" for f in fo]
        fast = P.cross_validation(0, postprocess=False, folds=lab, also_withhold=lab_o)
        assert list(P.cv_folds_["label"]) == ["a", "b"] or list(P.cv_folds_["label"]) == ["b", "a"]
        assert sorted(P.cv_folds_["n_withheld"]) == [129, 171] and not P.cv_folds_["failed"].any()
        slow = P.cross_validation(0, postprocess=False, folds=lab, also_withhold=lab_o, refactor_each=True)
        assert len(fast) == 229 and list(fast["fold"]) == list(slow["fold"])
        check(fast["pred"].values, fast["pred_err"].values, slow["pred"].values, slow["pred_err"].values, f"refactor_each {kind}")
    finally:
        P.close()


@pytest.mark.parametrize("kind,metric", [("nugget", HAV), ("zero", EUC)])
def test_fold_stats_against_dense_sigma(native, kind, metric):
    """5. log|Q_SS| and alpha_S^T Q_SS^-1 alpha_S of three folds (LDS path, batched path, both processes) from the dense Sigma"""
    p, coords, values, S = make_data(kind, metric)
    rng = np.random.default_rng(5)
    fi = labels_of_sizes(rng, N0, [7, 150])
    fi[fi == 2] = -1
    fo = np.full(N1, -1, dtype=np.int32)
    fo[rng.permutation(N1)[:20]] = 2
    fi[np.flatnonzero(fi < 0)[:9]] = 2
    h = handle(native, p, coords, values, metric)
    try:
        info, _, _, stats = h.cv_folds(0, fi, fo, want_stats=True)
        assert info == 0
    finally:
        h.close()
    Q = np.linalg.inv(S)
    alpha = Q @ np.concatenate(values)
    for f in range(3):
        ix = np.concatenate([np.flatnonzero(fi == f), N0 + np.flatnonzero(fo == f)])
        assert stats[f, 0] == len(ix)
        ld = np.linalg.slogdet(Q[np.ix_(ix, ix)])[1]
        qf = alpha[ix] @ np.linalg.solve(Q[np.ix_(ix, ix)], alpha[ix])
        print(f"fold {f} ({len(ix)}): logdet {stats[f, 1]:.12e} vs {ld:.12e}, quad {stats[f, 2]:.12e} vs {qf:.12e}")
        assert abs(stats[f, 1] - ld) <= 1e-8 * abs(ld)
        assert abs(stats[f, 2] - qf) <= 1e-8 * abs(qf)


def test_state(native):
    """6. the handle around the call"""
    p, coords, values, _ = make_data("nugget", HAV)
    rng = np.random.default_rng(6)
    pc = np.column_stack([rng.uniform(26, 49, 100), rng.uniform(-118, -72, 100)])
    fi = labels_of_sizes(rng, N0, [1, 30, 64, 100])
    fo = labels_of_sizes(rng, N1, [0, 10, 0, 40]).astype(np.int32)
    fo[fo == 4] = -1
    h = handle(native, p, coords, values, HAV)
    try:
        a = h.predict(0, pc)
        r1 = h.cv_folds(0, fi, fo, want_stats=True)
        with pytest.raises(native.NativeError, match="ck_cv_folds"):
            h.verify_model()
        b = h.predict(0, pc)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert h.verify_model() == 0
        r2 = h.cv_folds(0, fi, fo, want_stats=True)
        for x, y in zip(r1[1:], r2[1:]):
            assert np.array_equal(x, y, equal_nan=True)
        h.loglik(False)
        r3 = h.cv_folds(0, fi, fo, want_stats=True)
        h.predict_blocks(0, pc, np.arange(100, dtype=np.int32) // 10, np.ones(100), 10)
        r4 = h.cv_folds(0, fi, fo, want_stats=True)
        for r in (r3, r4):
            assert r[0] == 0
            for x, y in zip(r1[1:], r[1:]):
                assert np.array_equal(x, y, equal_nan=True)
        t = h.cv_folds_timings()
        assert t["total_ms"] > 0 and t["sweep_ms"] > 0 and t["gram_ms"] > 0 and t["solve_ms"] > 0
        for bad, msg in ((np.full(N0, 7, dtype=np.int32), "outside"), (np.where(fi == 2, 0, fi).astype(np.int32), "fold 2 is empty")):
            with pytest.raises(native.NativeError, match=msg):
                h.cv_folds(0, bad, None, n_folds=5)
    finally:
        h.close()


def test_frame(native):
    """8. the frames of Predictor.cross_validation with and without folds"""
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    p, coords, values, _ = make_data("nugget", EUC)
    mod = model.MultivariateMatern(2)
    mod.params.set_values(np.asarray(PARAMS[("nugget", EUC)]))
    mf = fields.MultiField([fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])])
    P = joint_prediction.Predictor(mod, mf, fast_dist=False, dist_units=None)
    try:
        rng = np.random.default_rng(8)
        labels = np.array(["t%d" % k for k in rng.integers(0, 6, N0)], dtype=object)
        labels[:10] = None
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            df = P.cross_validation(0, postprocess=False, folds=labels)
        assert list(df.columns) == ["d1", "d2", "data", "pred", "residual", "pred_err", "fold"]
        assert len(df) == N0 - 10 and df["pred"].notna().all()
        key = df[["d1", "d2"]].values
        assert np.array_equal(np.lexsort((key[:, 1], key[:, 0])), np.arange(len(df)))
        assert np.allclose(df["residual"], df["data"] - df["pred"], rtol=0, atol=0)
        lut = {tuple(c): l for c, l in zip(coords[0], labels)}
        assert all(lut[(a, b)] == f for a, b, f in zip(df["d1"], df["d2"], df["fold"]))
        cf = P.cv_folds_
        assert list(cf.columns) == ["label", "n_withheld", "nlpd", "failed"] and len(cf) == 6
        assert cf["n_withheld"].sum() == N0 - 10 and np.isfinite(cf["nlpd"]).all() and not cf["failed"].any()
        fi = np.array([-1 if l is None else list(cf["label"]).index(l) for l in labels], dtype=np.int32)
        rp, re = oracle_folds(p, coords, values, EUC, 0, fi, None)
        order = np.lexsort((coords[0][:, 1], coords[0][:, 0]))
        order = order[fi[order] >= 0]
        check(df["pred"].values, df["pred_err"].values, rp[order], re[order], "frame")
        k5 = P.cross_validation(0, postprocess=False, folds=5, seed=3)
        assert len(k5) == N0 and sorted(P.cv_folds_["n_withheld"]) == [60] * 5
        plain = P.cross_validation(0, postprocess=False)
        assert list(plain.columns) == ["d1", "d2", "data", "pred", "residual", "pred_err"] and len(plain) == N0
        lp, le = P._factored_handle().loocv(0, N0)
        order = np.lexsort((coords[0][:, 1], coords[0][:, 0]))
        assert np.array_equal(plain["pred"].values, lp[order]) and np.array_equal(plain["pred_err"].values, le[order])
    finally:
        P.close()
