"""Host side of conditional simulation (Predictor.conditional_simulation / conditional_draws_arrays), without a GPU: the
validation that precedes any device work, duplicate sites, and the postprocess of the draws.  The device half
(include/cokrige.h: ck_conditional_draws) is tests/test_gpu_conditional.py."""
import numpy as np
import pandas as pd
import pytest

from sif_xco2_cokriging_amd import joint_prediction


class _NoDevice(joint_prediction.Predictor):
    """the checks must raise before the resident factor is asked for"""

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


def _pc(m, seed=0):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(25, 50, m), rng.uniform(-120, -70, m)])


@pytest.fixture
def pred():
    return _NoDevice(_Mod(), _MF([_Field(5), _Field(5)]))


@pytest.mark.parametrize("n_draws", [0, -3, 2.5, True])
def test_bad_n_draws(pred, n_draws):
    with pytest.raises(ValueError, match="n_draws"):
        pred.conditional_draws_arrays(0, _pc(10), n_draws)
    with pytest.raises(ValueError, match="n_draws"):
        pred.conditional_simulation(0, _pc(10), n_draws=n_draws)


@pytest.mark.parametrize("shape", [(4, 10), (5, 9), (50,), (5, 10, 1)])
def test_bad_noise_shape(pred, shape):
    with pytest.raises(ValueError, match="noise"):
        pred.conditional_draws_arrays(0, _pc(10), 5, noise=np.zeros(shape))


def test_too_many_sites(pred):
    lat, lon = np.meshgrid(np.arange(257) * 0.01, np.arange(256) * 0.01, indexing="ij")
    pc = np.column_stack([lat.ravel(), lon.ravel()])
    assert len(pc) == 65792
    with pytest.raises(ValueError, match="65536"):
        pred.conditional_draws_arrays(0, pc, 1)


@pytest.mark.parametrize("i", [-1, 2, 7, 0.0])
def test_process_index_out_of_range(pred, i):
    with pytest.raises(ValueError, match="process index"):
        pred.conditional_draws_arrays(i, _pc(10), 3)


@pytest.mark.parametrize("kw", [{"tol": -1e-12}, {"jitter": -1e-9}, {"tol": np.nan}, {"jitter": np.inf}])
def test_negative_tol_or_jitter(pred, kw):
    with pytest.raises(ValueError, match="tol and jitter"):
        pred.conditional_draws_arrays(0, _pc(10), 3, **kw)
    with pytest.raises(ValueError, match="tol and jitter"):
        pred.conditional_simulation(1, _pc(10), 3, **kw)


def test_bad_seed(pred):
    with pytest.raises(ValueError, match="seed"):
        pred.conditional_draws_arrays(0, _pc(10), 3, seed=-1)
    with pytest.raises(ValueError, match="seed"):
        pred.conditional_draws_arrays(0, _pc(10), 3, seed=2 ** 64)


class _FakeHandle:
    """stands in for native.Handle: draws = pred + noise (identity L_S), the device's noise a function of the index"""

    def __init__(self):
        self.calls = []

    def conditional_draws(self, i, pc, n_draws, seed=0, noise=None, tol=1e-10, jitter=0.0):
        self.calls.append((i, pc.copy(), n_draws, seed, None if noise is None else noise.copy()))
        m = len(pc)
        pred = np.sin(pc[:, 0]) + 0.1 * pc[:, 1]
        err = 0.2 + 0.01 * np.abs(pc[:, 0])
        eps = noise if noise is not None else np.add.outer(np.arange(n_draws) * 1000.0, np.arange(m))
        defl = np.zeros(m, dtype=bool)
        defl[0] = True
        eps = np.where(defl, 0.0, eps)
        return pred + eps, pred, err, defl, 0

    def draws_timings(self):
        return {}


class _Fake(joint_prediction.Predictor):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.fake = _FakeHandle()

    def _factored_handle(self):
        return self.fake


def test_duplicates_are_one_variable():
    p = _Fake(_Mod(), _MF([_Field(5), _Field(5)]))
    pc = _pc(6)
    pcd = np.vstack([pc, pc[[4, 1, 4]]])           # sites 6, 7, 8 repeat 4, 1, 4
    noise = np.arange(7 * 9, dtype=float).reshape(7, 9)
    draws, pr, err, defl, seed = p.conditional_draws_arrays(1, pcd, 7, seed=5, noise=noise)
    (i, sent, n, s, e), = p.fake.calls
    assert i == 1 and n == 7 and s == 5 and np.array_equal(sent, pc)
    assert np.array_equal(e, noise[:, :6])         # the columns of the first occurrences
    for a, b in [(6, 4), (7, 1), (8, 4)]:
        assert np.array_equal(draws[:, a], draws[:, b]) and pr[a] == pr[b] and err[a] == err[b]
    assert defl[0] and not defl[1:].any()
    # the device stream is keyed on the de-duplicated index: no duplicates -> the caller's index
    d2, p2, *_ = p.conditional_draws_arrays(0, pcd, 3, seed=1)
    assert np.allclose(d2[:, 1:6] - p2[1:6], np.add.outer(np.arange(3) * 1000.0, np.arange(1, 6)), rtol=0, atol=1e-9)
    assert np.allclose(d2[:, 6:] - p2[6:], np.add.outer(np.arange(3) * 1000.0, [4, 1, 4]), rtol=0, atol=1e-9)


def test_seed_none_draws_64_bits():
    p = _Fake(_Mod(), _MF([_Field(5), _Field(5)]))
    seeds = {p.conditional_draws_arrays(0, _pc(4), 2)[4] for _ in range(4)}
    assert len(seeds) == 4 and all(0 <= s < 2 ** 64 for s in seeds)


class _StubTrend:
    def predict(self, X):
        X = np.asarray(X, dtype=float)
        return 0.3 * X[:, 0] - 0.2 * X[:, 1] + 1.0


def test_postprocess_scales_every_draw():
    at = {"scale_fact": 2.5, "spatial_mean": 400.0, "temporal_trend": 1.5, "covariate_means": [0.0, 0.0],
          "covariate_scales": [10.0, 10.0], "spatial_model": _StubTrend()}
    p = _Fake(_Mod(), _MF([_Field(5, at), _Field(5, at)]))
    pc = _pc(8)
    raw, rp, re, _, _ = p.conditional_draws_arrays(0, pc, 4, seed=3)
    out = p.conditional_simulation(0, pc, 4, seed=3, postprocess=True)
    if joint_prediction.xr is None:
        df, draws = out
        assert df.attrs == {"seed": 3, "n_deflated": 1, "jitter": 0.0}
        assert list(df.index.names) == ["lon", "lat"] and list(df.columns) == ["pred", "pred_err"]
        assert draws.shape == (4, 8)
        assert np.allclose(draws - df["pred"].values, 2.5 * (raw - rp), rtol=0, atol=1e-12)
        assert np.allclose(df["pred_err"].values, 2.5 * re)
        df0, d0 = p.conditional_simulation(0, pc, 4, seed=3, postprocess=False)
        assert list(df0.index.names) == ["d1", "d2"] and np.array_equal(d0, raw)
    else:
        assert out.attrs["seed"] == 3 and out["draws"].dims[0] == "draw"
