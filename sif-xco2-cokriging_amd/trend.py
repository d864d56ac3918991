"""Trend designs of universal cokriging (``Predictor(trend=...)``, ``log_likelihood(trend=...)``).

A trend names, per process k, the regressors F_k(coords) (n x p_k) of an unknown mean  E[Z_k(s)] = F_k(s) beta_k:

  * ``"constant"``: one column of ones per process (ordinary cokriging);
  * ``"linear"``:   [1, c1, c2] per process, the two coordinate columns centred and scaled by that process's data sites
                    (the prediction sites use the same centring and scale);
  * a callable ``f(k, coords) -> (n, p_k)``, used for the data and the prediction sites alike.

Everything here is host-side validation; the GLS arithmetic runs in the library (include/cokrige.h: ck_set_trend).
"""
from __future__ import annotations

import numpy as np

PMAX = 8   # include/cokrige.h: CK_TREND_PMAX


def check_trend(trend):
    """ValueError unless ``trend`` is None, "constant", "linear" or a callable."""
    if trend is None or callable(trend) or (isinstance(trend, str) and trend in ("constant", "linear")):
        return trend
    raise ValueError(f"trend must be None, 'constant', 'linear' or a callable f(k, coords) -> (n, p_k), not {trend!r}")


class TrendDesign:
    """The regressors of every process for one set of data sites (``data_coords[k]``: (n_k, 2))."""

    def __init__(self, trend, data_coords):
        self.trend = check_trend(trend)
        if trend is None:
            raise ValueError("no trend")
        self.n_procs = len(data_coords)
        self._centre, self._scale = [], []
        for c in data_coords:
            c = np.asarray(c, dtype=np.float64)[:, :2]
            mu = c.mean(axis=0) if len(c) else np.zeros(2)
            sd = c.std(axis=0) if len(c) else np.ones(2)
            self._centre.append(mu)
            self._scale.append(np.where(sd > 0, sd, 1.0))
        self.p = [self._design(k, np.asarray(data_coords[k], dtype=np.float64)[:1, :2]).shape[1]
                  for k in range(self.n_procs)]

    def _design(self, k, coords):
        c = np.atleast_2d(np.asarray(coords, dtype=np.float64))
        n = len(c)
        if self.trend == "constant":
            return np.ones((n, 1))
        if self.trend == "linear":
            return np.column_stack([np.ones(n), (c[:, :2] - self._centre[k]) / self._scale[k]])
        F = np.asarray(self.trend(k, c), dtype=np.float64)
        if F.ndim == 1:
            F = F[:, None]
        if F.ndim != 2 or F.shape[0] != n:
            raise ValueError(f"the trend callable returned shape {F.shape} for {n} sites of process {k}; expected (n, p_k)")
        return F

    def __call__(self, k, coords):
        """(n, p_k) regressors of process k at ``coords``; NaN / inf entries are allowed here (prediction sites)."""
        F = self._design(k, coords)
        if F.shape[1] > PMAX:
            raise ValueError(f"{F.shape[1]} regressors for process {k}; at most {PMAX} per process")
        if hasattr(self, "p") and F.shape[1] != self.p[k]:
            raise ValueError(f"the trend gave {F.shape[1]} regressors for process {k} here and {self.p[k]} at its data sites")
        return np.ascontiguousarray(F)

    def data(self, k, coords):
        """The regressors at the data sites of process k: finite, at most as many columns as sites."""
        F = self(k, coords)
        if not np.all(np.isfinite(F)):
            bad = int(np.flatnonzero(~np.all(np.isfinite(F), axis=1))[0])
            raise ValueError(f"the trend regressors of process {k} are not finite at data site {bad}")
        if F.shape[1] > len(F):
            raise ValueError(f"process {k} has {len(F)} data sites for {F.shape[1]} regressors")
        return F
