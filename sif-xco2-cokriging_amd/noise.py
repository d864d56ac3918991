"""Per-observation measurement-error variances: what ``measurement_error=`` / ``noise_scale=`` of the predictors and of the
likelihood mean, resolved on the host before any device work (include/cokrige.h: ck_set_noise).

    Sigma_noise = Sigma + diag(s_k d_a)

``measurement_error``: None (no noise: the calls are bit for bit what they are without the argument), True (every field's
``variance_estimate``, the reference's attribute: src/fields.py:88) or a list with one array or None per process.
"""
from __future__ import annotations

import numpy as np


def field_variance(field, k=None):
    """The variances that go with ``values_main``: ``variance_estimate_main`` when the field has it, else
    ``variance_estimate`` if it has one value per main datum (the reference keeps it per row of ``values``)."""
    n = len(np.asarray(field.values_main))
    for name in ("variance_estimate_main", "variance_estimate"):
        v = getattr(field, name, None)
        if v is not None:
            v = np.asarray(v, dtype=np.float64).ravel()
            if len(v) == n:
                return v
    which = "" if k is None else f" of process {k}"
    raise ValueError(f"measurement_error=True: the field{which} has no variance_estimate with one value per datum of "
                     f"values_main ({n}); build it with Field(..., variance_estimate=...) or pass the arrays as a list")


def resolve_measurement_error(measurement_error, noise_scale, fields, devices=None):
    """(variances, scales): a list with one float64 array or None per process, and one scale per process.  Raises
    ValueError / NotImplementedError before any device work; (None, None) when ``measurement_error`` is None."""
    n_procs = len(fields)
    if measurement_error is None or measurement_error is False:
        return None, None
    if devices is not None and len(devices) > 1:
        raise NotImplementedError("measurement_error runs on one device; the multi-GPU path has no per-observation noise")
    if measurement_error is True:
        var = [field_variance(fields[k], k) for k in range(n_procs)]
    else:
        try:
            items = list(measurement_error)
        except TypeError:
            raise ValueError("measurement_error must be None, True or a list with an array or None per process") from None
        if len(items) != n_procs:
            raise ValueError(f"measurement_error has {len(items)} entries for {n_procs} processes")
        var = []
        for k, d in enumerate(items):
            if d is None:
                var.append(None)
                continue
            d = np.ascontiguousarray(d, dtype=np.float64).ravel()
            n = len(np.asarray(fields[k].values_main))
            if len(d) != n:
                raise ValueError(f"measurement_error[{k}] has {len(d)} variances, process {k} has {n} data")
            if not np.all(np.isfinite(d)) or np.any(d < 0.0):
                bad = int(np.flatnonzero(~(np.isfinite(d) & (d >= 0.0)))[0])
                raise ValueError(f"measurement_error[{k}][{bad}] = {d[bad]!r}: variances must be finite and >= 0")
            var.append(d)
    if noise_scale is None:
        noise_scale = (1.0,) * n_procs
    s = np.atleast_1d(np.asarray(noise_scale, dtype=np.float64)).ravel()
    if s.size == 1:
        s = np.repeat(s, n_procs)
    if s.size < n_procs:
        raise ValueError(f"noise_scale has {s.size} entries for {n_procs} processes")
    s = s[:n_procs]
    if not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError(f"noise_scale = {tuple(s.tolist())}: scales must be finite and >= 0")
    return var, tuple(float(x) for x in s)


def apply_noise(h, var, scales, drop=None):
    """Set the resolved variances on a handle whose data are loaded; ``drop[k]``: indices of process k removed from its data
    (the refactor-each forms of cross-validation)."""
    if var is None:
        return
    for k, d in enumerate(var):
        if d is not None and drop is not None and drop[k] is not None:
            d = np.delete(d, drop[k])
        h.set_noise(k, d, scales[k])


def noise_key(var, scales):
    """What a resident factor depends on besides model and data (Predictor._state_key)."""
    if var is None:
        return ()
    return tuple((None if d is None else (d.shape, hash(d.tobytes()))) for d in var) + (tuple(scales),)
