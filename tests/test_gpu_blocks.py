"""GPU tests of block (areal) cokriging: include/cokrige.h ck_predict_blocks, native.Handle.predict_blocks and
joint_prediction.Predictor.predict_blocks against a dense numpy chain (oracle covariances + scipy cho_solve), and the
state the call leaves on the handle."""
import numpy as np
import pandas as pd
import pytest
from scipy.linalg import cho_factor, cho_solve

from oracle import cokrige_oracle as orc

pytestmark = pytest.mark.gpu

HAV, EUC = 0, 1
BIV = [0.99, 0.81, 0.39, 0.695, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]
BIV_EUC = [0.99, 0.81, 0.39, 0.695, 1.0, 2.5, 2.5, 2.5, 0.02, 0.025, -0.19]
UNI = [1.1, 0.6, 380.0, 0.03]
UNI_EUC = [1.1, 0.6, 2.0, 0.03]


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def make_data(rng, params, metric, n_per=700):
    """sites of one or two processes (the second half co-located with the first), values drawn from the model"""
    p = orc.Params.from_flat(params)
    if metric == HAV:
        pts = np.column_stack([rng.uniform(25, 50, 2 * n_per), rng.uniform(-120, -70, 2 * n_per)])
    else:
        pts = np.column_stack([rng.uniform(0, 10, 2 * n_per), rng.uniform(0, 10, 2 * n_per)])
    coords = [pts[:n_per], pts[n_per // 2:n_per // 2 + n_per]] if p.n_procs == 2 else [pts[:n_per]]
    S = orc.joint_cov(p, coords, metric)
    z = np.linalg.cholesky(S) @ rng.standard_normal(S.shape[0])
    values = np.split(z, np.cumsum([len(c) for c in coords])[:-1])
    return p, coords, values


def pred_sites(rng, metric, m):
    if metric == HAV:
        return np.column_stack([rng.uniform(26, 49, m), rng.uniform(-118, -72, m)])
    return np.column_stack([rng.uniform(0.5, 9.5, m), rng.uniform(0.5, 9.5, m)])


def random_blocks(rng, r, max_size, singletons=5):
    """labels of r blocks of 1 .. max_size sites (the first `singletons` of one site, one of max_size), shuffled"""
    sizes = rng.integers(1, max_size + 1, r)
    sizes[:singletons] = 1
    sizes[singletons] = max_size
    lab = np.repeat(np.arange(r), sizes)
    return lab[rng.permutation(len(lab))]


def handle(native, p, coords, values, metric):
    h = native.Handle(0)
    if p.n_procs == 2:
        h.set_model(2, p.sigma, [p.nu[0, 0], p.nu[0, 1], p.nu[1, 1]], [p.len_scale[0, 0], p.len_scale[0, 1], p.len_scale[1, 1]],
                    p.nugget, p.rho)
    else:
        h.set_model(1, p.sigma, [p.nu[0, 0]] * 3, [p.len_scale[0, 0]] * 3, p.nugget, 0.0)
    h.set_metric(metric)
    for k in range(p.n_procs):
        h.set_data(k, coords[k], values[k])
    h.assemble_joint()
    assert h.factor() == 0
    return h


def dense_chain(p, coords, values, pc, i, metric, A):
    """A pred, A S A^T with S = C_pp - c0^T Sigma^-1 c0 (src/joint_prediction.py:60-78 with the full m x m matrix)"""
    cf = cho_factor(orc.joint_cov(p, coords, metric), lower=True)
    c0 = orc.pred_cross_cov(p, coords, pc, i, metric)
    pred = c0.T @ cho_solve(cf, np.concatenate(values))
    S = orc.pred_cov(p, pc, i, metric) - c0.T @ cho_solve(cf, c0)
    return A @ pred, A @ S @ A.T


def amat(lab, w, r):
    A = np.zeros((r, len(lab)))
    A[lab, np.arange(len(lab))] = w
    return A


CASES = [  # (params, metric, i, r): blocks of 1 .. 40 sites, m = sum of the sizes -- about 540 (r = 30: Hilbert-sorted rows)
    # or below 256 (r = 10)
    (BIV, HAV, 0, 30), (BIV, HAV, 1, 30), (BIV_EUC, EUC, 0, 30), (BIV_EUC, EUC, 1, 10),
    (UNI, HAV, 0, 30), (UNI_EUC, EUC, 0, 10), (BIV, HAV, 1, 10),
]


@pytest.mark.parametrize("params,metric,i,r", CASES)
def test_blocks_match_the_dense_chain(native, params, metric, i, r):
    rng = np.random.default_rng(7 + 31 * i + 3 * r + metric)
    p, coords, values = make_data(rng, params, metric)
    lab = random_blocks(rng, r, 40)
    m = len(lab)
    assert (m >= 256) == (r == 30)
    pc = pred_sites(rng, metric, m)
    w = rng.uniform(0.2, 2.0, m)
    h = handle(native, p, coords, values, metric)
    pred, err, cov = h.predict_blocks(i, pc, lab, w, r, want_cov=True)
    rp, rc = dense_chain(p, coords, values, pc, i, metric, amat(lab, w, r))
    assert rel(pred, rp) < 1e-9
    assert np.max(np.abs(err ** 2 - np.maximum(np.diag(rc), 0.0))) < 1e-10
    assert np.max(np.abs(cov - rc)) < 1e-10
    assert np.array_equal(cov, cov.T)
    # without the covariance: the same pred / err bits
    p2, e2, c2 = h.predict_blocks(i, pc, lab, w, r)
    assert c2 is None and np.array_equal(p2, pred) and np.array_equal(e2, err)
    h.close()


def test_many_blocks_and_one_block_match_the_dense_chain(native):
    """r = 900 blocks: the covariance spans two Schur panels (rows and columns beyond 512) -- every entry against the
    dense chain; then ONE block of all sites (a whole-domain mean: its 1.1 M pairs are spread over many pieces)"""
    rng = np.random.default_rng(21)
    p, coords, values = make_data(rng, BIV, HAV, n_per=300)
    lab = np.concatenate([np.arange(900), rng.integers(0, 900, 150)])
    lab = lab[rng.permutation(len(lab))]
    m = len(lab)
    pc = pred_sites(rng, HAV, m)
    w = rng.uniform(0.2, 2.0, m)
    h = handle(native, p, coords, values, HAV)
    for i in (0, 1):
        pred, err, cov = h.predict_blocks(i, pc, lab, w, 900, want_cov=True)
        rp, rc = dense_chain(p, coords, values, pc, i, HAV, amat(lab, w, 900))
        assert rel(pred, rp) < 1e-9
        assert np.max(np.abs(err ** 2 - np.maximum(np.diag(rc), 0.0))) < 1e-10
        assert np.max(np.abs(cov - rc)) < 1e-10
        assert np.max(np.abs(cov[512:, :512] - rc[512:, :512])) < 1e-10 and np.max(np.abs(cov[512:, 512:] - rc[512:, 512:])) < 1e-10
        one = np.zeros(m, dtype=np.int64)
        pred1, err1, cov1 = h.predict_blocks(i, pc, one, w, 1, want_cov=True)
        rp1, rc1 = dense_chain(p, coords, values, pc, i, HAV, amat(one, w, 1))
        assert rel(pred1, rp1) < 1e-9
        assert abs(err1[0] ** 2 - rc1[0, 0]) < 1e-10 * max(1.0, abs(rc1[0, 0]))
        assert abs(cov1[0, 0] - rc1[0, 0]) < 1e-10 * max(1.0, abs(rc1[0, 0]))
        again = h.predict_blocks(i, pc, one, w, 1, want_cov=True)
        assert np.array_equal(again[0], pred1) and np.array_equal(again[1], err1) and np.array_equal(again[2], cov1)
    h.close()


@pytest.mark.parametrize("nugget", [True, False])
def test_nugget_cases(native, nugget):
    """a site on a datum of process i (c0 carries the nugget there), and one site twice in a block (C_pp's nugget on
    both of its pairs); nugget 0: the singleton on the datum has zero variance and must come back as exactly 0 or a
    rounding residue, like the point path's nan_to_num"""
    rng = np.random.default_rng(11)
    params = list(BIV)
    if not nugget:
        params[8] = params[9] = 0.0
    p, coords, values = make_data(rng, params, HAV, n_per=300)
    for i in (0, 1):
        pc = pred_sites(rng, HAV, 40)
        pc[0] = coords[i][5]                 # block 0: the datum alone
        pc[1] = coords[i][17]                # block 1: a datum among other sites
        pc[2] = pc[3]                        # block 2: the same site twice
        lab = np.array([0, 1, 2, 2] + [1] * 6 + list(3 + np.arange(30) % 6))
        w = rng.uniform(0.5, 1.5, len(lab))
        h = handle(native, p, coords, values, HAV)
        pred, err, cov = h.predict_blocks(i, pc, lab, w, 9, want_cov=True)
        rp, rc = dense_chain(p, coords, values, pc, i, HAV, amat(lab, w, 9))
        assert rel(pred, rp) < 1e-9
        assert np.max(np.abs(err ** 2 - np.maximum(np.diag(rc), 0.0))) < 1e-10
        assert np.max(np.abs(cov - rc)) < 1e-10
        if not nugget:
            assert err[0] ** 2 < 1e-10 and abs(pred[0] - w[0] * values[i][5]) < 1e-7   # exact interpolation
        h.close()


@pytest.mark.parametrize("m", [600, 150])
def test_singleton_blocks_are_the_point_prediction(native, m):
    """blocks = arange(m) with weight 1: every block is one site, and the block path's arithmetic is the point path's
    (fma(1, row, 0) = row, the same sweep and reduction per row, C(0) + nugget = the point path's prior variance).
    Measured on the MI355X: bitwise equal for both pred and pred_err (the assertion allows 1e-12)."""
    rng = np.random.default_rng(5)
    p, coords, values = make_data(rng, BIV, HAV)
    pc = pred_sites(rng, HAV, m)
    h = handle(native, p, coords, values, HAV)
    for i in (0, 1):
        pp, pe = h.predict(i, pc)
        bp, be, _ = h.predict_blocks(i, pc, np.arange(m), np.ones(m), m)
        print(f"m={m} i={i}: pred bitwise {np.array_equal(bp, pp)}, pred_err bitwise {np.array_equal(be, pe)}")
        assert rel(bp, pp) <= 1e-12 and rel(be, pe) <= 1e-12
    h.close()


def test_reproducible_and_chunked(native):
    rng = np.random.default_rng(9)
    p, coords, values = make_data(rng, BIV, HAV)
    lab = random_blocks(rng, 50, 24)
    m = len(lab)
    pc = pred_sites(rng, HAV, m)
    w = rng.uniform(0.2, 2.0, m)
    h = handle(native, p, coords, values, HAV)
    a = h.predict_blocks(1, pc, lab, w, 50, want_cov=True)
    b = h.predict_blocks(1, pc, lab, w, 50, want_cov=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert h.timings()["blocks_chunks"] == 1
    h.set_option("block_chunk", 100)         # 100, 100, ... sites per K2 assembly (below 256: the caller's row order)
    c = h.predict_blocks(1, pc, lab, w, 50, want_cov=True)
    t = h.timings()
    assert t["blocks_chunks"] == (m + 99) // 100
    assert t["blocks_fold_ms"] > 0 and t["blocks_solve_ms"] > 0 and t["blocks_prior_ms"] > 0
    for x, y in zip(a, c):
        assert rel(y, x) < 1e-12
    h.set_option("block_chunk", 0)
    d = h.predict_blocks(1, pc, lab, w, 50, want_cov=True)
    for x, y in zip(a, d):
        assert np.array_equal(x, y)
    h.close()


def test_bad_input_is_refused_by_the_library(native):
    rng = np.random.default_rng(2)
    p, coords, values = make_data(rng, BIV, HAV, n_per=200)
    h = handle(native, p, coords, values, HAV)
    pc = pred_sites(rng, HAV, 6)
    for lab, w, r in [([0, 1, 2, 3, 0, 1], np.ones(6), 3),      # label out of range
                      ([0, 1, -1, 0, 1, 0], np.ones(6), 2),     # negative label
                      ([0, 0, 0, 2, 2, 2], np.ones(6), 3),      # block 1 empty
                      ([0, 0, 0, 1, 1, 1], [1, 1, np.nan, 1, 1, 1], 2),
                      ([0, 0, 0, 1, 1, 1], np.ones(6), 0)]:
        with pytest.raises(native.NativeError):
            h.predict_blocks(0, pc, lab, w, r)
    h.close()


def test_state_after_a_block_call(native):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    rng = np.random.default_rng(4)
    p, coords, values = make_data(rng, BIV, HAV, n_per=500)
    pc = pred_sites(rng, HAV, 300)
    lab = np.arange(300) % 17
    # the C ABI: ck_verify_model fails cleanly, ck_predict and ck_verify_model work again afterwards
    h = handle(native, p, coords, values, HAV)
    p0, e0 = h.predict(0, pc)
    assert h.verify_model() == 0
    h.predict_blocks(0, pc, lab, np.ones(300), 17)
    with pytest.raises(native.NativeError, match="ck_predict_blocks"):
        h.verify_model()
    p1, e1 = h.predict(0, pc)
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1)
    assert h.verify_model() == 0
    h.close()
    # the Predictor: __call__ gives the same bits before and after, on the same resident factor
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    mf = fields.MultiField([fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])])
    P = joint_prediction.Predictor(mod, mf)
    def call(P):
        out = P(1, pc, postprocess=False)
        out = out.to_dataframe() if hasattr(out, "to_dataframe") else out
        return out["pred"].values, out["pred_err"].values

    before = call(P)
    h0 = P._h
    factor_ms = h0.timings()["factor_ms"]
    df = P.predict_blocks(1, pc, lab, postprocess=False)
    assert P._h is h0 and h0.timings()["factor_ms"] == factor_ms
    after = call(P)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert list(df.index) == list(range(17)) and np.array_equal(df["n_sites"].values, np.bincount(lab))
    A = amat(lab, 1.0 / np.bincount(lab)[lab], 17)
    assert rel(df["pred"].values, A @ P.predict_arrays(1, pc)[0]) < 1e-9
    P.close()


class _StubTrend:
    def __init__(self, coef, intercept):
        self.coef, self.intercept = np.asarray(coef, dtype=float), float(intercept)

    def predict(self, X):
        return np.asarray(X, dtype=float) @ self.coef + self.intercept


class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


def test_postprocess_is_the_weighted_sum_of_the_point_postprocess(native):
    from sif_xco2_cokriging_amd import fields, joint_prediction, model
    rng = np.random.default_rng(8)
    p, coords, values = make_data(rng, BIV, HAV, n_per=500)
    at = dict(scale_fact=1.7, spatial_mean=0.25, temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
              covariate_scales=[12.0, 6.0], spatial_model=_StubTrend([0.3, -0.2], 0.05))
    f0, f1 = fields.Field(coords[0], values[0]), fields.Field(coords[1], values[1])
    for f in (f0, f1):
        f.ds = _Attrs(at)
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(BIV))
    P = joint_prediction.Predictor(mod, fields.MultiField([f0, f1]))
    pcn = pred_sites(rng, HAV, 400)
    pc = pd.DataFrame(pcn, columns=["lat", "lon"])
    lab = rng.integers(0, 40, 400)
    r = 40
    w = rng.uniform(0.3, 1.5, 400)
    out = P(1, pc, postprocess=True)
    out = out.to_dataframe().reset_index() if hasattr(out, "to_dataframe") else out.reset_index()
    out = pc.merge(out, on=["lat", "lon"], how="left")
    raw, cov_raw = P.predict_blocks(1, pc, lab, w, postprocess=False, return_cov=True)
    df, cov = P.predict_blocks(1, pc, lab, w, postprocess=True, return_cov=True)
    A = amat(lab, w, r)[np.unique(lab)]
    assert rel(df["pred"].values, A @ out["pred"].values) < 1e-12
    assert rel(df["pred_err"].values, 1.7 * raw["pred_err"].values) < 1e-12
    assert rel(cov, 1.7 ** 2 * cov_raw) < 1e-12
    P.close()


def test_full_size_one_degree_cells(native):
    """N = 40 000, the 8 833-point 0.5-degree grid folded into 1-degree cells"""
    from sif_xco2_cokriging_amd import synth
    pb = synth.conus_problem(20000)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.assemble_joint()
    pc = pb["pcoords"]
    m = len(pc)
    info, pred, err = h.factor_predict(0, pc)
    assert info == 0
    cells = np.floor(pc[:, 0]).astype(np.int64) * 1000 + np.floor(pc[:, 1]).astype(np.int64)
    uniq, lab = np.unique(cells, return_inverse=True)
    r = len(uniq)
    w = 1.0 / np.bincount(lab)[lab]
    bp, be, _ = h.predict_blocks(0, pc, lab, w, r)
    A = amat(lab, w, r)
    assert rel(bp, A @ pred) < 1e-9
    worst = np.zeros(r)
    np.maximum.at(worst, lab, err)
    assert np.all(be > 0) and np.all(be <= worst * (1 + 1e-12))   # sd of a mean <= the largest sd of its members
    # ~200 sites as blocks of their own: their point pred_err comes back
    rng = np.random.default_rng(1)
    alone = rng.choice(m, 200, replace=False)
    lab2 = lab.copy()
    lab2[alone] = r + np.arange(200)
    uniq2, lab2 = np.unique(lab2, return_inverse=True)
    w2 = 1.0 / np.bincount(lab2)[lab2]
    bp2, be2, cov2 = h.predict_blocks(0, pc, lab2, w2, len(uniq2), want_cov=True)
    assert rel(be2[lab2[alone]], err[alone]) < 1e-9
    assert rel(bp2[lab2[alone]], pred[alone]) < 1e-9
    assert np.array_equal(cov2, cov2.T)
    assert np.max(np.abs(np.diag(cov2) - be2 ** 2)) < 1e-10
    t = h.timings()
    print({k: round(v, 3) for k, v in t.items() if k.startswith("blocks_")})
    h.close()
