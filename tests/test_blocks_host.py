"""Host side of block cokriging (Predictor.predict_blocks), without a GPU: label compaction, site exclusion, default
weights, the validation that precedes any device work, and the postprocess arithmetic of a weighted sum.  The device
half (include/cokrige.h: ck_predict_blocks) is tests/test_gpu_blocks.py."""
import numpy as np
import pandas as pd
import pytest

from sif_xco2_cokriging_amd import joint_prediction


class _NoDevice(joint_prediction.Predictor):
    """predict_blocks must raise its ValueErrors before it asks for the resident factor"""

    def _factored_handle(self):
        raise AssertionError("device touched before the input was validated")


class _Field:
    def __init__(self, n, attrs=None):
        self.coords_main = np.zeros((n, 2))
        self.values_main = np.zeros(n)
        self.timestamp = "2020-07-01"
        if attrs is not None:
            self.ds = type("DS", (), {"attrs": attrs})()


class _MF:
    def __init__(self, fields):
        self.fields = fields
        self.n_procs = len(fields)


class _Mod:
    n_procs = 2


class _StubTrend:
    def __init__(self, coef, intercept):
        self.coef, self.intercept = np.asarray(coef, dtype=float), float(intercept)

    def predict(self, X):
        return np.asarray(X, dtype=float) @ self.coef + self.intercept


class _FakeHandle:
    """stands in for native.Handle: a 'point predictor' pred_a = f(site), covariance S = diag(e^2) + 0.1 e e^T, and the
    block results as the exact linear functionals A pred, A S A^T"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def point(pc):
        pred = np.sin(pc[:, 0]) + 0.1 * pc[:, 1]
        e = 0.2 + 0.01 * np.abs(pc[:, 0])
        return pred, np.diag(e ** 2) + 0.1 * np.outer(e, e)

    def predict_blocks(self, i, pc, codes, w, r, want_cov=False):
        self.calls.append((i, pc.copy(), codes.copy(), w.copy(), r, want_cov))
        A = np.zeros((r, len(pc)))
        A[codes, np.arange(len(pc))] = w
        pred, S = self.point(pc)
        cov = A @ S @ A.T
        return A @ pred, np.sqrt(np.diag(cov)), (cov if want_cov else None)


def _predictor(attrs=None, cls=joint_prediction.Predictor):
    return cls(_Mod(), _MF([_Field(3, attrs), _Field(3, attrs)]))


def test_label_compaction_exclusion_and_default_weights():
    pc = np.arange(16.0).reshape(8, 2)
    blocks = ["b", "a", None, "b", float("nan"), "c", "a", "b"]
    sites, codes, w, labels, inside = joint_prediction.Predictor._block_layout(pc, blocks)
    assert list(labels) == ["a", "b", "c"]                       # sorted labels -> codes 0 .. r - 1
    assert np.array_equal(inside, [True, True, False, True, False, True, True, True])
    assert np.array_equal(codes, [1, 0, 1, 2, 0, 1])
    assert codes.dtype == np.int32
    assert np.array_equal(sites, pc[inside])
    np.testing.assert_allclose(w, [1 / 3, 1 / 2, 1 / 3, 1.0, 1 / 2, 1 / 3], rtol=0, atol=0)
    # numeric labels with NaN, given weights kept for the sites inside a block
    b = np.array([5.0, np.nan, 2.0, 5.0])
    sites, codes, w, labels, inside = joint_prediction.Predictor._block_layout(pc[:4], b, weights=[1.0, np.nan, 2.0, 3.0])
    assert list(labels) == [2.0, 5.0] and np.array_equal(codes, [1, 0, 1]) and np.array_equal(w, [1.0, 2.0, 3.0])
    # tuples name cells (lat, lon); a DataFrame's first two columns are the coordinates
    df = pd.DataFrame({"lat": [30.2, 30.7, 31.1], "lon": [-100.4, -99.9, -99.6], "other": [0, 0, 0]})
    cells = list(zip(np.floor(df.lat).astype(int), np.floor(df.lon).astype(int)))
    sites, codes, w, labels, _ = joint_prediction.Predictor._block_layout(df, cells)
    assert sites.shape == (3, 2) and np.array_equal(sites, df[["lat", "lon"]].values)
    assert list(labels) == [(30, -101), (30, -100), (31, -100)] and np.array_equal(codes, [0, 1, 2])


@pytest.mark.parametrize("case", ["blocks_length", "weights_length", "weights_nan", "weights_inf", "no_block", "bad_coords"])
def test_validation_before_any_device_work(case):
    P = _predictor(cls=_NoDevice)
    pc = np.column_stack([np.linspace(30, 40, 5), np.linspace(-100, -90, 5)])
    blocks, weights = [0, 0, 1, 1, 2], None
    if case == "blocks_length":
        blocks = [0, 0, 1, 1]
    elif case == "weights_length":
        weights = np.ones(4)
    elif case == "weights_nan":
        weights = [1.0, np.nan, 1.0, 1.0, 1.0]
    elif case == "weights_inf":
        weights = [1.0, 1.0, np.inf, 1.0, 1.0]
    elif case == "no_block":
        blocks = [None, np.nan, None, None, None]
    elif case == "bad_coords":
        pc = np.arange(5.0)[:, None]
    with pytest.raises(ValueError):
        P.predict_blocks(0, pc, blocks, weights)


def test_results_frame_and_postprocess_arithmetic():
    at = dict(scale_fact=1.7, spatial_mean=0.25, temporal_trend=-0.4, covariate_means=[-95.0, 37.0],
              covariate_scales=[12.0, 6.0], spatial_model=_StubTrend([0.3, -0.2], 0.05))
    P = _predictor(at)
    fake = _FakeHandle()
    P._factored_handle = lambda: fake
    rng = np.random.default_rng(3)
    m = 40
    pc = np.column_stack([rng.uniform(30, 40, m), rng.uniform(-100, -90, m)])
    labels = rng.choice(np.array(["x", "y", "z", "w"], dtype=object), m)
    labels[[3, 7]] = None
    w = rng.uniform(0.5, 2.0, m)
    raw, cov_raw = P.predict_blocks(1, pc, labels, w, postprocess=False, return_cov=True)
    df, cov = P.predict_blocks(1, pc, labels, w, postprocess=True, return_cov=True)
    i, sites, codes, ww, r, want = fake.calls[-1]
    assert i == 1 and r == 4 and want and len(sites) == m - 2
    assert list(df.index) == ["w", "x", "y", "z"] and df.index.name == "block"
    keep = np.array([x is not None for x in labels])
    for b, lab in enumerate(df.index):
        sel = keep & (labels == lab)
        assert df["n_sites"].iloc[b] == sel.sum()
        np.testing.assert_allclose(df["lat"].iloc[b], np.sum(w[sel] * pc[sel, 0]) / np.sum(w[sel]), rtol=1e-14)
        np.testing.assert_allclose(df["lon"].iloc[b], np.sum(w[sel] * pc[sel, 1]) / np.sum(w[sel]), rtol=1e-14)
    # postprocess of the weighted sum == the weighted sum of the postprocessed point predictions
    # (pred_pp_a = scale_fact pred_a + spatial_mean + trend_a + temporal_trend, src/joint_prediction.py:155-205)
    pred_pt, _ = fake.point(pc[keep])
    trend = at["spatial_model"].predict(np.column_stack([(pc[keep, 1] + 95.0) / 12.0, (pc[keep, 0] - 37.0) / 6.0]))
    pp = pred_pt * 1.7 + 0.25 + trend - 0.4
    A = np.zeros((4, keep.sum()))
    A[codes, np.arange(keep.sum())] = w[keep]
    np.testing.assert_allclose(df["pred"].values, A @ pp, rtol=1e-13)
    np.testing.assert_allclose(df["pred_err"].values, raw["pred_err"].values * 1.7, rtol=1e-15)
    np.testing.assert_allclose(cov, cov_raw * 1.7 ** 2, rtol=1e-15)
    np.testing.assert_allclose(raw["pred"].values, A @ pred_pt, rtol=1e-14)
    # default weights: the plain block means
    df_mean = P.predict_blocks(1, pc, labels, postprocess=False)
    A1 = (A > 0) / (A > 0).sum(axis=1, keepdims=True)
    np.testing.assert_allclose(df_mean["pred"].values, A1 @ pred_pt, rtol=1e-14)


def test_postprocess_missing_trend_makes_the_block_nan():
    at = dict(scale_fact=2.0, spatial_mean=0.0, temporal_trend=0.0, covariate_means=[0.0, 0.0], covariate_scales=[1.0, 1.0],
              spatial_model=_StubTrend([0.0, 0.0], 0.0))
    P = _predictor(at)
    P.i = 0
    real = P._spatial_trend
    P._spatial_trend = lambda df: np.where(np.arange(len(df)) == 2, np.nan, real(df))   # site 2: covariate missing
    pc = np.column_stack([np.linspace(30, 31, 5), np.linspace(-100, -99, 5)])
    codes = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    w = np.ones(5)
    pred, err, cov = P._postprocess_blocks(pc, codes, w, 3, np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3]), None)
    assert np.isnan(pred[1]) and np.array_equal(pred[[0, 2]], [2.0, 6.0])
    assert np.array_equal(err, [0.2, 0.4, 0.6]) and cov is None
