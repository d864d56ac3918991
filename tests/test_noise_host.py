"""Host side of the per-observation measurement-error variances, without a GPU: Field keeps ``variance_estimate``, the
resolution of ``measurement_error`` / ``noise_scale`` (sif_xco2_cokriging_amd/noise.py) as a pure function, the refusals of the
predictors that need no device, and the two new symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest

from sif_xco2_cokriging_amd import fields, joint_prediction, model, native, point_prediction
from sif_xco2_cokriging_amd.noise import apply_noise, noise_key, resolve_measurement_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(with_var=(True, True)):
    rng = np.random.default_rng(0)
    out = []
    for k, n in enumerate((6, 5)):
        c, v = rng.uniform(0, 1, (n, 2)), rng.standard_normal(n)
        out.append(fields.Field(c, v, variance_estimate=rng.uniform(0.01, 0.1, n) if with_var[k] else None))
    return out


def test_field_keeps_the_variances():
    f = _fields()[0]
    assert f.variance_estimate.shape == (6,) and f.variance_estimate_main is f.variance_estimate
    assert fields.Field(f.coords, f.values).variance_estimate is None
    g = fields.Field(f.coords, f.values, coords_main=f.coords[:4], values_main=f.values[:4], variance_estimate=f.variance_estimate,
                     variance_estimate_main=f.variance_estimate[:4])
    assert g.variance_estimate_main.shape == (4,)
    with pytest.raises(ValueError, match="variance_estimate has 5 values for 6"):
        fields.Field(f.coords, f.values, variance_estimate=np.ones(5))
    with pytest.raises(ValueError, match="variance_estimate_main has 3 values for 4"):
        fields.Field(f.coords, f.values, coords_main=f.coords[:4], values_main=f.values[:4], variance_estimate_main=np.ones(3))


def test_resolution():
    fl = _fields()
    assert resolve_measurement_error(None, (1.0, 1.0), fl) == (None, None)
    var, s = resolve_measurement_error(True, (2.0, 0.5), fl)
    assert s == (2.0, 0.5) and all(np.array_equal(var[k], fl[k].variance_estimate) for k in range(2))
    var, s = resolve_measurement_error([None, np.full(5, 0.2)], None, fl)
    assert var[0] is None and np.array_equal(var[1], np.full(5, 0.2)) and s == (1.0, 1.0)
    assert resolve_measurement_error(True, 3.0, fl)[1] == (3.0, 3.0)
    with pytest.raises(ValueError, match="process 1 has no variance_estimate|field of process 1 has no variance_estimate"):
        resolve_measurement_error(True, None, _fields((True, False)))
    with pytest.raises(ValueError, match=r"measurement_error\[0\] has 4 variances, process 0 has 6"):
        resolve_measurement_error([np.ones(4), None], None, fl)
    with pytest.raises(ValueError, match=r"measurement_error\[1\]\[2\]"):
        resolve_measurement_error([None, [0.1, 0.1, -0.1, 0.1, 0.1]], None, fl)
    with pytest.raises(ValueError, match="1 entries for 2 processes"):
        resolve_measurement_error([np.ones(6)], None, fl)
    with pytest.raises(ValueError, match="noise_scale"):
        resolve_measurement_error(True, (1.0, -2.0), fl)
    with pytest.raises(NotImplementedError, match="one device"):
        resolve_measurement_error(True, None, fl, devices=[0, 1])
    assert resolve_measurement_error(None, None, fl, devices=[0, 1]) == (None, None)   # no noise: the multi-GPU path as it was
    # the reference's field: variance_estimate only, one value per datum
    class RefField:
        pass
    r = RefField()
    r.values_main, r.variance_estimate = np.zeros(6), np.full(6, 0.3)
    assert np.array_equal(resolve_measurement_error(True, None, [r, fl[1]])[0][0], np.full(6, 0.3))
    assert noise_key(None, None) == () and noise_key(*resolve_measurement_error(True, (1.0, 2.0), fl)) != noise_key(
        *resolve_measurement_error(True, (1.0, 1.0), fl))


def test_apply_noise_with_withheld_data():
    calls = []

    class H:
        def set_noise(self, k, d, s):
            calls.append((k, None if d is None else d.copy(), s))
    var, s = resolve_measurement_error(True, (2.0, 0.5), _fields())
    apply_noise(H(), var, s, drop=[np.array([1, 4]), None])
    assert calls[0][0] == 0 and np.array_equal(calls[0][1], np.delete(var[0], [1, 4])) and calls[0][2] == 2.0
    assert np.array_equal(calls[1][1], var[1]) and calls[1][2] == 0.5
    apply_noise(H(), None, None)
    assert len(calls) == 2


def test_predictors_refuse_before_any_device_work():
    mf = fields.MultiField(_fields())
    mod = model.MultivariateMatern(2)
    for cls in (joint_prediction.Predictor, point_prediction.Predictor):
        with pytest.raises(NotImplementedError, match="one device"):
            cls(mod, mf, measurement_error=True, devices=[0, 1])
        with pytest.raises(ValueError, match="no variance_estimate"):
            cls(mod, fields.MultiField(_fields((False, True))), measurement_error=True)
        P = cls(mod, mf, measurement_error=True, noise_scale=(2.0, 0.5))
        assert P._h is None and P.measurement_error is True
    a = joint_prediction.Predictor(mod, mf)._state_key()
    b = joint_prediction.Predictor(mod, mf, measurement_error=True)._state_key()
    c = joint_prediction.Predictor(mod, mf, measurement_error=True, noise_scale=(1.0, 2.0))._state_key()
    assert a != b and b != c and a == joint_prediction.Predictor(mod, mf, measurement_error=None)._state_key()


def test_sim_fields_carry_epsilon_squared():
    import pandas as pd
    from sif_xco2_cokriging_amd import sim
    f = sim.BivariateRandomField.__new__(sim.BivariateRandomField)
    samples = []
    for j, eps in enumerate((0.1, 0.0)):
        df = pd.DataFrame({"x": [1.0, 0.0, 2.0], "y": [0.0, 1.0, 2.0], f"Z{j}": [1.0, 2.0, 3.0]})
        df.attrs["epsilon"] = eps
        samples.append(df)
    mf = f.to_fields(samples)
    assert np.allclose(mf.fields[0].variance_estimate, 0.01) and mf.fields[1].variance_estimate is None


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cokrige.h")).read()
    for name in ("ck_set_noise", "ck_loglik_noise_grad"):
        assert re.search(rf"\bint {name}\(ck_handle\*", hdr) and name in native.exported_names()
    assert hasattr(native.Handle, "set_noise") and hasattr(native.Handle, "loglik_noise_grad")
