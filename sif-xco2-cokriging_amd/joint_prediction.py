"""Global ("joint") cokriging -- same call signatures as the reference's
``joint_prediction`` module (src/joint_prediction.py), numeric core in HIP.

    from sif_xco2_cokriging_amd import joint_prediction as prediction
    cokrig = prediction.Predictor(mod, mf, fast_dist=False, dist_units=None)
    ds = cokrig(1, pcoords, postprocess=False)

``mod`` / ``mf`` may be this package's ``model.MultivariateMatern`` / ``fields.MultiField``
or the reference's own objects: only ``mod.n_procs``, ``mod.params.<p>.values``,
``mf.n_procs`` and ``mf.fields[k].coords_main / values_main / timestamp / ds.attrs``
are read.

What runs on the GPU (include/cokrige.h): assembly of Sigma and c0, blocked FP64-MFMA
Cholesky, forward substitution fused with the prediction / variance reductions.  The
factor is kept on the device, so further calls with new ``pcoords`` or another ``i`` cost
one substitution sweep each.

Deviations from the reference, all outside the arithmetic:
  * the reference's ``_verify_model`` factorises the (m+N)x(m+N) stacked matrix to decide
    whether to warn (src/joint_prediction.py:60-66,260-274).  Sigma is positive definite at
    that point, so the stacked matrix is positive definite iff the m x m Schur complement
    C_pp - c0^T Sigma^-1 c0 is: ``ck_verify_model`` factorises THAT, from the solved
    right-hand sides the prediction left on the device (see ``_verify``).  Where the stacked
    matrix is exactly singular (duplicate prediction sites; a site on a datum of the predicted
    process) the reference's own outcome hangs on rounding; here those cases always warn.
  * without xarray installed the result is a pandas DataFrame indexed by the coordinate
    columns instead of an ``xarray.Dataset`` (same columns ``pred``, ``pred_err``).
"""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd
from numpy.linalg import LinAlgError

from . import native
from .fields import metric_of
from .model import configure_handle
from .noise import apply_noise, noise_key, resolve_measurement_error
from .trend import TrendDesign, check_trend

try:  # the reference returns xarray objects; keep that when xarray exists
    import xarray as xr
except Exception:  # pragma: no cover - absent in the build image
    xr = None


class Predictor:
    """Multivariate prediction framework (src/joint_prediction.py:13-33)."""

    def __init__(self, mod, mf, covariates=None, dist_units: str = "km", fast_dist: bool = True,
                 device: int = 0, devices=None, trend=None, measurement_error=None, noise_scale=(1.0, 1.0)) -> None:
        """``devices=[0, 1, ...]``: the multi-GPU form (BASELINE configs[3]) -- one worker process per entry, Sigma
        block-column-cyclic over them, panels exchanged over RCCL/xGMI at each Cholesky step, prediction points sharded
        (workers.RankPool + distributed.DistributedJoint; the same ordinal twice rehearses it on one GPU over gloo).
        The reference's parallel entry is likewise a keyword on the predictor (src/point_prediction.py:45-52,69-81).
        Same results as ``device=`` to rounding; ``cross_validation`` and the exact ``_verify_model`` check are
        single-device paths and run on ``devices[0]``.

        ``trend``: None (simple cokriging, the data have a known zero mean), ``"constant"`` (ordinary cokriging),
        ``"linear"`` ([1, c1, c2] per process, coordinates centred and scaled by that process's data sites) or a callable
        ``f(k, coords) -> (n, p_k)``: universal cokriging, the trend estimated by GLS jointly with the kriging and its
        uncertainty added to ``pred_err`` (include/cokrige.h: ck_predict_universal).  After a call ``trend_coef`` holds
        the GLS coefficients and ``trend_cov`` their covariance.  A prediction site whose regressors are not finite gets
        NaN.  The universal forms of ``predict_blocks``, ``conditional_simulation``, ``cross_validation`` and the
        multi-GPU path are not available.

        ``measurement_error``: per-observation measurement-error variances d_a, added to the true diagonal of Sigma as
        ``noise_scale[k] * d_a`` (include/cokrige.h: ck_set_noise).  None: none, today's behaviour; True: every field's
        ``variance_estimate``; a list with an array or None per process.  The predictions filter the measurement error out
        (c0 and the prior variance are the field's); ``cross_validation`` predicts the withheld OBSERVATION, so its
        ``pred_err`` contains the datum's own noise.  Single-device only."""
        if mod.n_procs != mf.n_procs:
            raise ValueError("Number of theoretical processes different from empirical processes.")
        self.measurement_error, self.noise_scale = measurement_error, noise_scale
        resolve_measurement_error(measurement_error, noise_scale, mf.fields, devices)   # refusals before any device work
        self.trend = check_trend(trend)
        if self.trend is not None and devices is not None and len(devices) > 1:
            raise NotImplementedError("universal cokriging (trend=...) runs on one device; the multi-GPU path is simple "
                                      "cokriging only")
        self.trend_coef, self.trend_cov = None, None
        self.n_procs = mod.n_procs
        self.mod = mod
        self.mf = mf
        self.covariates = covariates
        self.dist_units = dist_units
        self.fast_dist = fast_dist
        self.devices = None if devices is None else [int(d) for d in devices]
        self.device = device if self.devices is None else self.devices[0]
        self._pool, self._pool_key = None, None
        self.comm = {}
        self.timings = {}
        self.rhs_budget_bytes = 48 << 30   # device memory for the right-hand sides of one ck_predict call
        # _verify_model: None = exact check (Cholesky of the m x m Schur complement on the device) for up to
        # `verify_max_points` prediction sites and the variance test beyond; True / False force it on / off
        self.verify_model = None
        self.verify_max_points = 16384
        self._h = None
        self._key = None
        self._verdict = None

    # -- device state -------------------------------------------------------------------------
    def _new_handle(self, drop=None):
        """Handle with model, metric and data loaded; ``drop=(i, ix)`` withholds datum ix of
        process i (LOOCV, src/joint_prediction.py:56-58,112-113,140-146)."""
        h = native.Handle(self.device)
        configure_handle(h, self.mod)
        h.set_metric(metric_of(self.dist_units, self.fast_dist))
        for k in range(self.n_procs):
            c = np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)
            v = np.asarray(self.mf.fields[k].values_main, dtype=np.float64)
            if drop is not None and drop[0] == k:
                c = np.delete(c, drop[1], axis=0)
                v = np.delete(v, drop[1], axis=0)
            h.set_data(k, c, v)
        self._set_noise(h, None if drop is None else [drop[1] if k == drop[0] else None for k in range(self.n_procs)])
        return h

    def _noise(self):
        return resolve_measurement_error(getattr(self, "measurement_error", None), getattr(self, "noise_scale", None),
                                         self.mf.fields, self.devices)

    def _set_noise(self, h, drop=None):
        """``measurement_error`` on a handle whose data are loaded; ``drop[k]``: the data of process k that were left out."""
        var, scales = self._noise()
        apply_noise(h, var, scales, drop)

    @staticmethod
    def _factor(h):
        h.assemble_joint()
        info = h.factor()
        if info != 0:
            # scipy.linalg.cho_factor's message (raised uncaught at src/joint_prediction.py:69)
            raise LinAlgError(f"{info}-th leading minor of the array is not positive definite")

    @staticmethod
    def _factor_predict(h, i, pc):
        """cho_factor + the solve of src/joint_prediction.py:67-78 in one library call: the factorisation and the forward
        substitution run as two overlapped sweeps (include/cokrige.h: ck_factor_predict); the factor stays resident."""
        h.assemble_joint()
        info, pred, err = h.factor_predict(i, pc)
        if info != 0:
            raise LinAlgError(f"{info}-th leading minor of the array is not positive definite")
        return pred, err

    def _state_key(self):
        """What the resident factor depends on: the model's parameters, the metric, and the data arrays.  The
        reference re-reads `mod.params` and `mf` on every __call__ (src/joint_prediction.py:50-55); here the factor
        is reused only while none of them has changed (mod.fit(...), params.set_values(...), new fields -> refactor)."""
        from .model import model_arrays
        n, sig, nu, ls, nug, rho = model_arrays(self.mod)
        key = [n, sig.tobytes(), nu.tobytes(), ls.tobytes(), nug.tobytes(), float(rho),
               metric_of(self.dist_units, self.fast_dist)]
        for k in range(self.n_procs):
            f = self.mf.fields[k]
            c = np.ascontiguousarray(f.coords_main, dtype=np.float64)
            v = np.ascontiguousarray(f.values_main, dtype=np.float64)
            key += [c.shape, hash(c.tobytes()), hash(v.tobytes())]
        if getattr(self, "measurement_error", None) is not None:
            key.append(noise_key(*resolve_measurement_error(self.measurement_error, getattr(self, "noise_scale", None),
                                                           self.mf.fields, self.devices)))
        return tuple(key)

    def invalidate(self):
        """Drop the resident factor (it is rebuilt on the next call)."""
        if self._h is not None:
            self._h.close()
        self._h, self._key = None, None
        self._pool_key = None

    def close(self):
        """Release the device state; with ``devices=`` also end the worker processes."""
        self.invalidate()
        if self._pool is not None:
            self._pool.close()
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _predict_on_ranks(self, i, pc):
        """The multi-GPU form: ship model and data to the ranks when they have changed, predict on the resident factor
        otherwise."""
        from . import workers
        from .model import model_arrays
        key = self._state_key()
        if self._pool is None:
            self._pool = workers.RankPool(self.devices)
        reuse = key == self._pool_key
        if not reuse:
            self._pool.load(model_arrays(self.mod), metric_of(self.dist_units, self.fast_dist),
                            [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64) for k in range(self.n_procs)],
                            [np.asarray(self.mf.fields[k].values_main, dtype=np.float64) for k in range(self.n_procs)])
            self._pool_key = None
        pred, err = self._pool.predict_joint(i, pc, reuse_factor=reuse)
        self._pool_key = key
        self.timings, self.comm = self._pool.last_timings, self._pool.last_comm
        return pred, err

    def _factored_handle(self):
        key = self._state_key()
        if self._h is not None and key != self._key:
            self.invalidate()
        if self._h is None:
            h = self._new_handle()
            self._factor(h)
            self._h, self._key = h, key
        return self._h

    def predict_arrays(self, i: int, pcoords, cv_ix: int = None):
        """(pred, pred_err) as arrays -- the numeric body of ``__call__``
        (src/joint_prediction.py:49-78)."""
        pc = np.ascontiguousarray(np.atleast_2d(np.asarray(pcoords, dtype=np.float64)))
        if self.trend is not None:
            return self._predict_universal(i, pc, cv_ix)
        if cv_ix is None and self.devices is not None and len(self.devices) > 1:
            self._verdict = None     # the exact _verify_model check is a single-device path: the variance test stands in
            return self._predict_on_ranks(i, pc)
        if cv_ix is None:
            key = self._state_key()
            if self._h is not None and key != self._key:
                self.invalidate()
            fresh = self._h is None
            h = self._new_handle() if fresh else self._h
            # The right-hand sides take (m + 1) x N doubles on the device: very large grids go through the
            # resident factor in batches (one forward sweep each), sized by `rhs_budget_bytes`.
            n_pad = h.num_panels()[2]
            chunk = max(1024, int(self.rhs_budget_bytes // (8 * max(n_pad, 1))))
            self._verdict = None
            try:
                if fresh and len(pc) > chunk:
                    self._factor(h)
                if len(pc) <= chunk:
                    # first call on this model and data: factorisation and substitution overlapped
                    pred, err = self._factor_predict(h, i, pc) if fresh else h.predict(i, pc)
            except Exception:
                if fresh:
                    h.close()
                raise
            self._h, self._key = h, key
            if len(pc) <= chunk:
                self._verdict = self._verify(h, i, pc, err)
            else:
                parts = [h.predict(i, pc[a:a + chunk]) for a in range(0, len(pc), chunk)]
                pred = np.concatenate([p for p, _ in parts])
                err = np.concatenate([e for _, e in parts])
            self.timings = h.timings()
        else:
            h = self._new_handle(drop=(i, cv_ix))
            try:
                pred, err = self._factor_predict(h, i, pc)
            finally:
                h.close()
        return pred, err

    def _trend_design(self):
        return TrendDesign(self.trend, [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)[:, :2]
                                        for k in range(self.n_procs)])

    def _predict_universal(self, i, pc, cv_ix=None):
        """Universal cokriging (``trend``): the regressors are validated on the host before any device work, then the
        trend is set on the resident factor's handle (the factor does not depend on it) and the sites with finite
        regressors go through ``ck_predict_universal`` in chunks of ``rhs_budget_bytes``."""
        if not 0 <= int(i) < self.n_procs:
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        design = self._trend_design()
        F = [design.data(k, np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)[:, :2]) for k in range(self.n_procs)]
        if cv_ix is not None:
            F[i] = np.delete(F[i], cv_ix, axis=0)
        pc = np.ascontiguousarray(pc[:, :2])
        F0 = design(i, pc)
        ok = np.all(np.isfinite(F0), axis=1)
        self._verdict = None   # the exact _verify_model check is the simple-kriging one: the variance test stands in
        if cv_ix is None:
            h = self._factored_handle()
        else:
            h = self._new_handle(drop=(i, cv_ix))
        try:
            if cv_ix is not None:
                self._factor(h)
            for k in range(self.n_procs):
                h.set_trend(k, F[k])
            m = len(pc)
            pred, err = np.full(m, np.nan), np.full(m, np.nan)
            idx = np.flatnonzero(ok)
            n_pad = h.num_panels()[2]
            chunk = max(1024, int(self.rhs_budget_bytes // (8 * max(n_pad, 1))))
            beta, cov = None, None
            for a in range(0, max(len(idx), 1), chunk):
                sub = idx[a:a + chunk]
                p_, e_, beta, cov = h.predict_universal(i, pc[sub], F0[sub])
                pred[sub], err[sub] = p_, e_
            self.trend_coef, self.trend_cov = beta, cov
            if cv_ix is None:
                self.timings = h.universal_timings()
        finally:
            if cv_ix is not None:
                h.close()
        return pred, err

    def _no_trend(self, what):
        if self.trend is not None:
            raise NotImplementedError(f"{what} is simple cokriging only; it has no universal form (this predictor has "
                                      f"trend={self.trend!r})")

    def _verify(self, h, i, pc, pred_err):
        """True: the joint covariance of the data and these prediction sites is NOT positive definite
        (the reference's _verify_model raises LinAlgError, src/joint_prediction.py:260-274); False: it is;
        None: not checked exactly (switched off, or more than `verify_max_points` sites)."""
        want = self.verify_model
        if want is False or (want is None and len(pc) > self.verify_max_points):
            return None
        # exactly singular stacked matrices: two identical rows of pcoords, or a prediction site on a datum of
        # process i (h == 0 puts the nugget into c0 as well, src/model.py:195-196) -- decided on the coordinates
        rows = np.ascontiguousarray(pc).view([("a", np.float64), ("b", np.float64)]).ravel()
        if len(np.unique(rows)) < len(rows):
            return True
        data = np.ascontiguousarray(np.asarray(self.mf.fields[i].coords_main, dtype=np.float64)[:, :2])
        if np.isin(rows, data.view([("a", np.float64), ("b", np.float64)]).ravel()).any():
            return True
        return h.verify_model() != 0

    def _warn_if_invalid(self, pred_err):
        bad = self._verdict
        if bad is None:
            # not checked exactly: the necessary condition the variances give (a non-positive Schur diagonal)
            bad = bool(np.any(pred_err <= 0.0))
        if bad:
            warnings.warn("Prediction joint covariance matrix is not positive definte; model"
                          " technically invalid.")

    # -- reference call signature ----------------------------------------------------------------
    def __call__(self, i: int, pcoords: pd.DataFrame, postprocess: bool = True, cv_ix: int = None):
        """Prediction and standard error of process ``i`` at ``pcoords`` (format [[lat, lon]])
        (src/joint_prediction.py:35-92)."""
        self.i = i
        if cv_ix is not None:
            p = np.asarray(pcoords, dtype=np.float64).ravel()
            pcoords = pd.DataFrame({"d1": p[0], "d2": p[1]}, index=[0])
        elif not isinstance(pcoords, pd.DataFrame):
            a = np.atleast_2d(np.asarray(pcoords, dtype=np.float64))
            pcoords = pd.DataFrame({"d1": a[:, 0], "d2": a[:, 1]})
        pred, err = self.predict_arrays(i, pcoords.values[:, :2], cv_ix=cv_ix)
        if cv_ix is None:
            self._warn_if_invalid(err)
        df_pred = pcoords.copy()
        df_pred["pred"] = pred
        df_pred["pred_err"] = err
        if postprocess:
            df_pred = df_pred.rename(columns={"d1": "lat", "d2": "lon"})
            return self._postprocess_predictions(df_pred)
        out = df_pred.set_index(pcoords.columns.values.tolist())
        if xr is None:
            return out
        ds = out.to_xarray()
        ts = self.mf.fields[self.i].timestamp
        try:
            np.isnan(ts)
            return ds
        except TypeError:
            return ds.assign_coords(coords={"time": np.datetime64(ts)})

    def _postprocess_predictions(self, df: pd.DataFrame):
        """Back to the scale of the original data: undo the standardisation, add the OLS
        spatial trend and the temporal trend (src/joint_prediction.py:155-205).  O(m) host
        work on the attributes src/fields.py:345-375 stored."""
        at = self.mf.fields[self.i].ds.attrs
        out = df[["lon", "lat"]].copy()
        out["pred"] = df["pred"].values * at["scale_fact"] + at["spatial_mean"]
        out["pred_err"] = df["pred_err"].values * at["scale_fact"]
        out["pred"] = out["pred"] + self._spatial_trend(df) + at["temporal_trend"]
        out = out.set_index(["lon", "lat"])
        if xr is None:
            return out
        ds = out.to_xarray()
        return ds.assign_coords(coords={"time": np.datetime64(self.mf.fields[self.i].timestamp)})

    def _spatial_trend(self, df: pd.DataFrame) -> np.ndarray:
        """The OLS spatial trend of process ``self.i`` at the sites of ``df`` (columns lon, lat); NaN where a covariate is
        missing (src/joint_prediction.py:170-200)."""
        at = self.mf.fields[self.i].ds.attrs
        if self.covariates is None:
            cov = df[["lon", "lat"]].copy()
            keep = np.ones(len(df), dtype=bool)
        else:
            if xr is None:
                raise RuntimeError("covariates are xarray objects in the reference; xarray is not installed")
            sel = self.covariates.sel(time=self.mf.fields[self.i].timestamp)
            vals = sel.to_dataframe(name="covariates").reset_index()
            merged = df[["lon", "lat"]].merge(vals[["lon", "lat", "covariates"]], on=["lon", "lat"], how="left")
            keep = merged["covariates"].notna().values
            cov = merged.loc[keep, ["covariates"]].copy()
        for k, name in enumerate(cov.columns):
            cov[name] = (cov[name] - at["covariate_means"][k]) / at["covariate_scales"][k]
        trend = np.full(len(df), np.nan)
        trend[keep] = at["spatial_model"].predict(cov)
        return trend

    # -- both processes at once -------------------------------------------------------------------
    @staticmethod
    def _sites_frame(pcoords):
        """prediction sites as the frame ``__call__`` works on (columns d1, d2 for an array)"""
        if isinstance(pcoords, pd.DataFrame):
            return pcoords
        a = np.atleast_2d(np.asarray(pcoords, dtype=np.float64))
        if a.ndim != 2 or a.shape[1] < 2:
            raise ValueError("pcoords must be [[lat, lon], ...]")
        return pd.DataFrame({"d1": a[:, 0], "d2": a[:, 1]})

    def predict_pair_arrays(self, pcoords, pcoords1=None, pairs=None):
        """Both processes from one forward sweep per chunk -- the numeric body of ``predict_pair`` (include/cokrige.h:
        ck_predict_pair).  Returns (pred_0, pred_err_0, pred_1, pred_err_1, cov): process 0 at ``pcoords``, process 1 at
        ``pcoords1`` (None: the same sites), cov[t] the posterior covariance between process 0 at site pairs[t, 0] and
        process 1 at site pairs[t, 1] (``pairs=None``: the co-located pairs (k, k) with the same sites, else no covariances
        and cov is None).  Grids beyond ``rhs_budget_bytes`` go through in chunks, both sets cut at the same indices, so every
        default pair stays inside one sweep; explicit ``pairs`` need both sets in one sweep.  Raises ValueError on bad
        arguments before any device work.  Runs on the resident factor of ``__call__``; with ``devices=[...]`` on
        ``devices[0]``."""
        pc0, pc1 = self._pair_sites("joint prediction of both processes", (0, 1), pcoords, pcoords1)
        m0, m1 = len(pc0), len(pc1)
        same = pcoords1 is None
        pr = None
        if pairs is not None:
            pr = np.asarray(pairs)
            if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
                raise ValueError("pairs must be (q, 2) integers: (site of process 0, site of process 1)")
            pr = pr.astype(np.int64)
            if len(pr) and (pr.min() < 0 or pr[:, 0].max() >= m0 or pr[:, 1].max() >= m1):
                raise ValueError(f"pairs index sites outside the {m0} sites of process 0 / the {m1} sites of process 1")
        h = self._factored_handle()
        # a sweep carries roundup(m0, 64) + m1 + 1 right-hand-side rows of n_pad doubles
        n_pad = h.num_panels()[2]
        rows = max(1024, int(self.rhs_budget_bytes // (8 * max(n_pad, 1))))
        step = max(1, (rows - 65) // 2)
        if max(m0, m1) <= step:
            p0, e0, p1, e1, cov = h.predict_pair(pc0, pc1, pr if pr is not None else
                                                 (np.column_stack([np.arange(m0)] * 2) if same else None))
        else:
            if pr is not None:
                raise ValueError(f"explicit pairs need both site sets in one sweep: {m0} + {m1} sites exceed the {rows} "
                                 f"right-hand-side rows of rhs_budget_bytes = {self.rhs_budget_bytes}")
            parts = []
            for a in range(0, max(m0, m1), step):
                s0, s1 = pc0[a:a + step], pc1[a:a + step]
                parts.append(h.predict_pair(s0, s1, np.column_stack([np.arange(len(s0))] * 2) if same else None))
            p0, e0, p1, e1 = (np.concatenate([p[j] for p in parts]) for j in range(4))
            cov = np.concatenate([p[4] for p in parts]) if same else None
        self.timings = h.pair_timings()
        return p0, e0, p1, e1, cov

    def predict_pair(self, pcoords, pcoords1=None, pairs=None, postprocess: bool = True):
        """Prediction and standard error of BOTH processes with the covariance of their prediction errors.

        Two ``__call__``s give two marginal posteriors; whatever needs both fields at once (a SIF / XCO2 ratio or
        regression, anomaly co-occurrence, a flux inversion fed with both maps) also needs how their errors are correlated.
        ``pcoords1=None``: the same sites for both processes.  The result has the shape of ``__call__``'s (Dataset, or
        DataFrame without xarray) with ``pred_0``, ``pred_err_0``, ``pred_1``, ``pred_err_1`` and, per site, ``pred_cov`` --
        the posterior covariance between the two processes there -- and ``pred_corr = pred_cov / (pred_err_0 pred_err_1)``
        (NaN where an error is 0).  With ``pcoords1`` the two processes have their own site sets: the result is a pair
        ``(out_0, out_1)``, each as ``__call__`` returns it for its process.  ``pairs`` (q, 2): explicit (site of process 0,
        site of process 1) pairs; their covariances come back as an array beside the result, ``(result, cov)``.
        ``postprocess`` transforms each process as ``__call__`` does and scales the covariances by the product of the two
        ``scale_fact``s (the correlation is scale-free).  Simple cokriging only (``trend=`` raises NotImplementedError)."""
        f0 = self._sites_frame(pcoords)
        f1 = f0 if pcoords1 is None else self._sites_frame(pcoords1)
        p0, e0, p1, e1, cov = self.predict_pair_arrays(f0.values[:, :2], None if pcoords1 is None else f1.values[:, :2], pairs)
        return self._pair_output(f0, None if pcoords1 is None else f1, p0, e0, p1, e1, cov, pairs, postprocess)

    def _pair_output(self, f0, f1, p0, e0, p1, e1, cov, pairs, postprocess):
        """What ``predict_pair`` returns from the arrays of both processes at the site frames f0 / f1 (f1 None: the same
        sites); shared with the local predictor's ``predict_pair``."""
        pcoords1 = f1
        scale = [self.mf.fields[k].ds.attrs["scale_fact"] for k in range(2)] if postprocess else [1.0, 1.0]
        if cov is not None:
            cov = cov * (scale[0] * scale[1])

        def one(k, f, pred, err):
            """the frame of process k as __call__ builds it"""
            self.i = k
            df = f.copy()
            df["pred"], df["pred_err"] = pred, err
            if postprocess:
                df = df.rename(columns={"d1": "lat", "d2": "lon"})
                at = self.mf.fields[k].ds.attrs
                out = df[["lon", "lat"]].copy()
                out["pred"] = pred * at["scale_fact"] + at["spatial_mean"] + self._spatial_trend(df) + at["temporal_trend"]
                out["pred_err"] = err * at["scale_fact"]
                out = out.set_index(["lon", "lat"])
            else:
                out = df.set_index(f.columns.values.tolist())
            return out

        def finish(out, k):
            if xr is None:
                return out
            ds = out.to_xarray()
            ts = self.mf.fields[k].timestamp
            try:
                np.isnan(ts)
                return ds
            except TypeError:
                return ds.assign_coords(coords={"time": np.datetime64(ts)})

        if pcoords1 is None:
            a, b = one(0, f0, p0, e0), one(1, f0, p1, e1)
            out = a.rename(columns={"pred": "pred_0", "pred_err": "pred_err_0"})
            out["pred_1"], out["pred_err_1"] = b["pred"].values, b["pred_err"].values
            if pairs is None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    den = e0 * e1 * (scale[0] * scale[1])
                    out["pred_cov"], out["pred_corr"] = cov, np.where(den > 0, cov / den, np.nan)
            res = finish(out, 0)
        else:
            res = (finish(one(0, f0, p0, e0), 0), finish(one(1, f1, p1, e1), 1))
        return (res, cov) if pairs is not None else res

    # -- regional means ---------------------------------------------------------------------------
    @staticmethod
    def _block_layout(pcoords, blocks, weights=None):
        """Host side of ``predict_blocks``: validated coordinates of the sites that belong to a block, their compact
        block codes (0 .. r - 1, in the order of the sorted labels), their weights (default 1 / n_b) and the labels.
        Raises ValueError before any device work."""
        pc = np.atleast_2d(np.asarray(pcoords.values if isinstance(pcoords, pd.DataFrame) else pcoords, dtype=np.float64))
        if pc.ndim != 2 or pc.shape[1] < 2:
            raise ValueError("pcoords must be [[lat, lon], ...]")
        pc = np.ascontiguousarray(pc[:, :2])
        m = len(pc)
        if isinstance(blocks, (np.ndarray, pd.Series, pd.Index)):
            lab = pd.Series(np.asarray(blocks))
        else:
            lab = pd.Series(list(blocks), dtype=object)
        if len(lab) != m:
            raise ValueError(f"blocks has {len(lab)} entries for {m} prediction sites")
        codes, labels = pd.factorize(lab, sort=True)   # NaN / None -> -1: the site is in no block
        labels = pd.Index(list(labels))
        inside = codes >= 0
        if not inside.any():
            raise ValueError("no prediction site belongs to a block")
        codes = codes[inside].astype(np.int32)
        r = len(labels)
        if weights is None:
            n_b = np.bincount(codes, minlength=r)
            w = 1.0 / n_b[codes]
        else:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if len(w) != m:
                raise ValueError(f"weights has {len(w)} entries for {m} prediction sites")
            w = w[inside]
            if not np.all(np.isfinite(w)):
                raise ValueError("weights must be finite for every site in a block")
        return pc[inside], codes, np.ascontiguousarray(w, dtype=np.float64), labels, inside

    def predict_blocks(self, i: int, pcoords, blocks, weights=None, postprocess: bool = True, return_cov: bool = False):
        """Weighted regional means of process ``i`` and their joint uncertainty (block cokriging).

        ``blocks[a]`` names the block of site ``pcoords[a]`` (any hashable; NaN / None leaves the site out), ``weights[a]``
        its weight (default: 1 / n_b, the plain mean of the block).  A block's prediction is the weighted sum of the joint
        point predictions of its sites, pred_b = sum_a w_a pred_a, and its standard error is sqrt(w^T S w) with S the
        posterior covariance of the point predictions -- not a combination of the sites' ``pred_err``, which are strongly
        correlated.  ``return_cov=True`` also returns the r x r covariance A S A^T of the blocks (``(df, cov)``, rows in
        the frame's order).  Runs on the resident factor of ``__call__`` (include/cokrige.h: ck_predict_blocks); with
        ``devices=[...]`` on ``devices[0]``, as ``cross_validation``.

        Returns a DataFrame indexed by the sorted block labels with ``pred``, ``pred_err``, ``n_sites`` and the weighted
        centroid ``lat`` / ``lon``.  ``postprocess=True`` is ``_postprocess_predictions`` applied to the weighted sum:
        pred = scale_fact pred_b + sum_a w_a (spatial_mean + trend_a + temporal_trend), pred_err and cov scaled by
        scale_fact (cov by its square); a block with a site whose trend is missing (covariate NaN) has pred NaN."""
        self._no_trend("predict_blocks")
        pc, codes, w, labels, _ = self._block_layout(pcoords, blocks, weights)
        r = len(labels)
        h = self._factored_handle()
        pred, err, cov = h.predict_blocks(i, pc, codes, w, r, want_cov=return_cov)
        n_sites = np.bincount(codes, minlength=r)
        sw = np.bincount(codes, weights=w, minlength=r)
        with np.errstate(invalid="ignore", divide="ignore"):
            lat = np.bincount(codes, weights=w * pc[:, 0], minlength=r) / sw
            lon = np.bincount(codes, weights=w * pc[:, 1], minlength=r) / sw
        if postprocess:
            self.i = i
            pred, err, cov = self._postprocess_blocks(pc, codes, w, r, pred, err, cov)
        index = labels.copy()
        if index.nlevels == 1:
            index.name = "block"
        df = pd.DataFrame({"pred": pred, "pred_err": err, "n_sites": n_sites, "lat": lat, "lon": lon}, index=index)
        return (df, cov) if return_cov else df

    def _postprocess_blocks(self, pc, codes, w, r, pred, err, cov):
        """``_postprocess_predictions`` of a weighted sum (process ``self.i``)."""
        at = self.mf.fields[self.i].ds.attrs
        sf = at["scale_fact"]
        trend = self._spatial_trend(pd.DataFrame({"lon": pc[:, 1], "lat": pc[:, 0]}))
        offset = at["spatial_mean"] + trend + at["temporal_trend"]
        missing = np.bincount(codes, weights=np.isnan(offset).astype(np.float64), minlength=r) > 0
        add = np.bincount(codes, weights=w * np.where(np.isnan(offset), 0.0, offset), minlength=r)
        pred = pred * sf + add
        pred[missing] = np.nan
        return pred, err * sf, (cov * (sf * sf) if cov is not None else None)

    # -- conditional simulation -------------------------------------------------------------------
    MAX_DRAW_SITES = 65536   # include/cokrige.h: ck_conditional_draws

    @staticmethod
    def _draw_sites(pcoords, name="pcoords"):
        pc = np.atleast_2d(np.asarray(pcoords.values if isinstance(pcoords, pd.DataFrame) else pcoords, dtype=np.float64))
        if pc.ndim != 2 or pc.shape[1] < 2 or len(pc) < 1:
            raise ValueError(f"{name} must be [[lat, lon], ...] with at least one site")
        return np.ascontiguousarray(pc[:, :2])

    @staticmethod
    def _draw_args(n_draws, tol, jitter, noise, m):
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or n_draws < 1:
            raise ValueError(f"n_draws must be an integer >= 1, not {n_draws!r}")
        n_draws = int(n_draws)
        if not (np.isfinite(tol) and tol >= 0.0) or not (np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError(f"tol and jitter must be finite and >= 0 (tol={tol!r}, jitter={jitter!r})")
        if noise is not None:
            noise = np.asarray(noise, dtype=np.float64)
            if noise.shape != (n_draws, m):
                raise ValueError(f"noise has shape {noise.shape}, expected (n_draws, m) = {(n_draws, m)}")
        return n_draws, noise

    @staticmethod
    def _first_occurrences(pc):
        """(keep, where): the first occurrences of the rows of pc in the caller's order, and every row's index among them"""
        rows = pc.view([("a", np.float64), ("b", np.float64)]).ravel()
        _, first, inv = np.unique(rows, return_index=True, return_inverse=True)
        order = np.argsort(first)
        keep = first[order]
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        return keep, rank[np.asarray(inv).ravel()]

    @staticmethod
    def _draw_seed(seed):
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        return seed

    def _pair_sites(self, what, i, pcoords, pcoords1):
        """The argument checks the joint forms share: the two site sets (pcoords1=None: the same sites for both)."""
        self._no_trend(what)
        if tuple(i) != (0, 1) or any(isinstance(k, bool) for k in i):
            raise ValueError(f"process index {i!r}: the joint form is i=(0, 1)")
        if self.n_procs != 2:
            raise ValueError(f"{what} needs a model of two processes, not {self.n_procs}")
        pc0 = self._draw_sites(pcoords)
        pc1 = pc0 if pcoords1 is None else self._draw_sites(pcoords1, "pcoords1")
        return pc0, pc1

    def _conditional_draws_pair(self, i, pcoords, pcoords1, n_draws, seed, noise, tol, jitter):
        """``conditional_draws_arrays`` for i=(0, 1): joint draws of both processes (include/cokrige.h:
        ck_conditional_draws_pair).  Everything is STACKED: columns [0, m0) are process 0 at ``pcoords``, [m0, m0 + m1)
        process 1 at ``pcoords1`` (None: the same sites); ``noise`` is (n_draws, m0 + m1) in that order.  Repeated sites
        are removed per process -- the two processes at one location are two random variables.  The Philox stream is
        keyed on the stacked index among the de-duplicated sites."""
        pc0, pc1 = self._pair_sites("joint conditional simulation", i, pcoords, pcoords1)
        m0, m1 = len(pc0), len(pc1)
        n_draws, noise = self._draw_args(n_draws, tol, jitter, noise, m0 + m1)
        (keep0, where0), (keep1, where1) = self._first_occurrences(pc0), self._first_occurrences(pc1)
        if len(keep0) + len(keep1) > self.MAX_DRAW_SITES:
            raise ValueError(f"{len(keep0)} + {len(keep1)} distinct prediction sites; conditional draws are limited to "
                             f"{self.MAX_DRAW_SITES}")
        seed = self._draw_seed(seed)
        e = None if noise is None else np.ascontiguousarray(np.hstack([noise[:, keep0], noise[:, m0 + keep1]]))
        h = self._factored_handle()
        draws, pred, err, defl, info = h.conditional_draws_pair(pc0[keep0], pc1[keep1], n_draws, seed=seed, noise=e, tol=tol,
                                                                jitter=jitter)
        if info != 0:
            k = 0 if info - 1 < len(keep0) else 1
            site = int((keep0, keep1)[k][info - 1 - k * len(keep0)])
            raise LinAlgError(f"the posterior covariance of the prediction sites is not positive definite at site {site} "
                              f"{tuple((pc0, pc1)[k][site])} of process {k}; a small jitter (e.g. jitter=1e-10) regularises "
                              f"nearly coincident sites")
        self.timings = h.pair_timings()
        where = np.concatenate([where0, len(keep0) + where1])
        return draws[:, where], pred[where], err[where], defl[where], seed

    def conditional_draws_arrays(self, i, pcoords, n_draws: int, seed=None, noise=None, tol: float = 1e-10,
                                 jitter: float = 0.0, pcoords1=None):
        """Draws from the posterior of process ``i`` at ``pcoords`` -- the numeric body of ``conditional_simulation``.

        draws[d] = pred + L_S eps_d, S = C_pp - c0^T Sigma^-1 c0 the posterior covariance of the point predictions
        (include/cokrige.h: ck_conditional_draws).  A site on a datum of process ``i`` has zero posterior variance; it is
        deflated (its draws equal pred).  Rows of ``pcoords`` that repeat a site are one random variable: they are removed
        before the device call and get the draws of their first occurrence.  ``noise`` (n_draws, m) in the caller's sites
        replaces the device's Philox stream (a duplicated site uses the column of its first occurrence); that stream is
        keyed on ``seed`` and on the index in the de-duplicated sites.  ``seed=None`` takes 64 bits from
        ``numpy.random.SeedSequence()``.  Runs on the resident factor of ``__call__``; with ``devices=[...]`` on
        ``devices[0]``.

        Returns (draws (n_draws, m), pred, pred_err, deflated (bool, m), seed).  Raises ValueError on bad arguments
        before any device work, and numpy.linalg.LinAlgError when S cannot be factored.

        ``i=(0, 1)``: joint draws of both processes, stacked (``_conditional_draws_pair`` has the layout); ``pcoords1``
        then gives process 1 its own sites."""
        self._no_trend("conditional simulation")
        if isinstance(i, tuple):
            return self._conditional_draws_pair(i, pcoords, pcoords1, n_draws, seed, noise, tol, jitter)
        if pcoords1 is not None:
            raise ValueError("pcoords1 belongs to the joint form i=(0, 1)")
        if isinstance(i, bool) or not (isinstance(i, (int, np.integer)) and 0 <= int(i) < self.n_procs):
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        pc = self._draw_sites(pcoords)
        m = len(pc)
        n_draws, noise = self._draw_args(n_draws, tol, jitter, noise, m)
        keep, where = self._first_occurrences(pc)
        if len(keep) > self.MAX_DRAW_SITES:
            raise ValueError(f"{len(keep)} distinct prediction sites; conditional draws are limited to {self.MAX_DRAW_SITES}")
        seed = self._draw_seed(seed)
        e = None if noise is None else np.ascontiguousarray(noise[:, keep])
        h = self._factored_handle()
        draws, pred, err, defl, info = h.conditional_draws(int(i), pc[keep], n_draws, seed=seed, noise=e, tol=tol,
                                                           jitter=jitter)
        if info != 0:
            site = int(keep[info - 1])
            raise LinAlgError(f"the posterior covariance of the prediction sites is not positive definite at site {site} "
                              f"{tuple(pc[site])}; a small jitter (e.g. jitter=1e-10) regularises nearly coincident sites")
        self.timings = h.draws_timings()
        return draws[:, where], pred[where], err[where], defl[where], seed

    def conditional_simulation(self, i, pcoords, n_draws: int = 100, seed=None, postprocess: bool = True, noise=None,
                               tol: float = 1e-10, jitter: float = 0.0, pcoords1=None):
        """Ensembles of maps drawn from the posterior of process ``i`` at ``pcoords`` (conditional simulation).

        Nonlinear quantities -- exceedance probabilities, areas above a threshold, maxima, ratios, inputs to downstream
        models -- need joint draws: neighbouring prediction errors are strongly correlated, so ``pred +- pred_err`` per site
        cannot give them.  Returns an object shaped like ``__call__``'s output: an xarray Dataset with ``pred``,
        ``pred_err`` and ``draws`` (a leading ``draw`` dimension), ``attrs`` holding ``seed``, ``n_deflated`` and
        ``jitter``.  ``postprocess=True`` applies ``_postprocess_predictions``' transform to every draw (scale, spatial
        mean, OLS trend, temporal trend).  Without xarray: ``(DataFrame, draws)`` -- the frame as ``__call__`` returns it
        (with the attrs in ``DataFrame.attrs``) and the (n_draws, m) array in its row order.  See
        ``conditional_draws_arrays`` for the arguments.

        ``i=(0, 1)``: co-simulation -- draw d of both processes comes from ONE draw of their joint posterior (the SIF / XCO2
        ratio of draw d is a draw of the ratio).  Returns a pair ``(out_0, out_1)``, each shaped as above for its process
        (process 1 at ``pcoords1``, default the same sites), with the same ``seed`` and ``jitter`` and its own ``n_deflated``;
        ``noise`` is (n_draws, m0 + m1), process 0's columns first."""
        pcoords = self._sites_frame(pcoords)
        if isinstance(i, tuple):
            pcoords1 = pcoords if pcoords1 is None else self._sites_frame(pcoords1)
            draws, pred, err, defl, seed = self.conditional_draws_arrays(i, pcoords.values[:, :2], n_draws, seed=seed, noise=noise,
                                                                         tol=tol, jitter=jitter, pcoords1=pcoords1.values[:, :2])
            m0 = len(pcoords)
            cols = [slice(0, m0), slice(m0, None)]
            return tuple(self._draws_output(k, (pcoords, pcoords1)[k], draws[:, cols[k]], pred[cols[k]], err[cols[k]],
                                            {"seed": seed, "n_deflated": int(defl[cols[k]].sum()), "jitter": float(jitter)},
                                            postprocess) for k in range(2))
        draws, pred, err, defl, seed = self.conditional_draws_arrays(i, pcoords.values[:, :2], n_draws, seed=seed,
                                                                     noise=noise, tol=tol, jitter=jitter, pcoords1=pcoords1)
        return self._draws_output(i, pcoords, draws, pred, err, {"seed": seed, "n_deflated": int(defl.sum()), "jitter": float(jitter)},
                                  postprocess)

    def _draws_output(self, i: int, pcoords: pd.DataFrame, draws, pred, err, attrs: dict, postprocess: bool):
        """What a conditional simulation returns, from its arrays (also borrowed by ``point_prediction.Predictor``): the frame of
        ``__call__`` with ``attrs``, every draw transformed as ``pred`` is, the xarray Dataset with a leading ``draw`` dimension
        (without xarray: ``(DataFrame, draws)``)."""
        self.i = i
        df = pcoords.copy()
        df["pred"], df["pred_err"] = pred, err
        if postprocess:
            df = df.rename(columns={"d1": "lat", "d2": "lon"})
            at = self.mf.fields[i].ds.attrs
            offset = at["spatial_mean"] + self._spatial_trend(df) + at["temporal_trend"]
            draws = draws * at["scale_fact"] + offset
            out = df[["lon", "lat"]].copy()
            out["pred"] = pred * at["scale_fact"] + offset
            out["pred_err"] = err * at["scale_fact"]
            out = out.set_index(["lon", "lat"])
        else:
            out = df.set_index(pcoords.columns.values.tolist())
        out.attrs.update(attrs)
        if xr is None:
            return out, draws
        ds = out.to_xarray()
        st = pd.DataFrame(draws.T, index=out.index, columns=pd.RangeIndex(draws.shape[0], name="draw")).stack()
        ds["draws"] = st.to_xarray().transpose("draw", *ds["pred"].dims)
        ds.attrs.update(attrs)
        if postprocess:
            return ds.assign_coords(coords={"time": np.datetime64(self.mf.fields[i].timestamp)})
        ts = self.mf.fields[i].timestamp
        try:
            np.isnan(ts)
            return ds
        except TypeError:
            return ds.assign_coords(coords={"time": np.datetime64(ts)})

    def cross_validation(self, i: int, postprocess: bool = True, refactor_each: bool = False, folds=None,
                         also_withhold=None, seed: int = 0) -> pd.DataFrame:
        """Leave-one-out cross-validation at each data location of process ``i``
        (src/joint_prediction.py:207-257).  The reference withholds one datum and re-assembles
        and re-factorises everything, n times; here all n leave-one-out predictions come from
        ONE factorisation (``ck_loocv``: the Gaussian conditional of z_q given the rest,
        pred_q = z_q - (Sigma^-1 z)_q / (Sigma^-1)_qq, var_q = 1 / (Sigma^-1)_qq -- the same
        numbers).  ``refactor_each=True`` runs the reference's n-solve loop instead.

        ``folds``: leave-GROUP-out cross-validation, still from the one resident factor (``ck_cv_folds``).  An array of n_i
        labels -- any hashable values, numbered in order of first appearance; ``None`` / NaN / -1 mean "never withheld" -- or
        an int K: a random K-fold drawn from ``seed``.  Every datum is predicted from the data outside its fold.
        ``also_withhold``: n_other labels from the same label set: the other process's data that leave together with a fold
        (the co-located partner, the same track).  The frame gains a ``fold`` column and loses the rows of never-withheld
        data; ``cv_folds_`` holds one row per fold: label, n_withheld, nlpd (the joint negative log predictive density of
        the withheld values) and failed.  ``refactor_each=True`` with folds runs the slow truth: a fresh factorisation per
        fold with that fold's data removed."""
        self._no_trend("cross_validation")
        if folds is not None or also_withhold is not None:
            return self._cv_folds(i, postprocess, refactor_each, folds, also_withhold, seed)
        names = ["lat", "lon"] if postprocess else ["d1", "d2"]
        f = self.mf.fields[i]
        data = pd.DataFrame(np.hstack((f.coords_main, np.atleast_2d(f.values_main).T)), columns=names + ["data"])
        if refactor_each:
            pred = np.empty(len(data))
            err = np.empty(len(data))
            for ix in range(len(data)):
                p, e = self.predict_arrays(i, f.coords_main[ix], cv_ix=ix)
                pred[ix], err[ix] = p[0], e[0]
        else:
            pred, err = self._factored_handle().loocv(i, len(data))
        return self._cv_frame(i, postprocess, data, names, pred, err)

    def _cv_frame(self, i, postprocess, data, names, pred, err, fold=None):
        f = self.mf.fields[i]
        if postprocess:
            tmp = pd.DataFrame({"lat": data["lat"], "lon": data["lon"], "pred": pred, "pred_err": err})
            self.i = i
            pp = self._postprocess_predictions(tmp)
            pp = pp.to_dataframe().reset_index() if xr is not None and not isinstance(pp, pd.DataFrame) else pp.reset_index()
            data = data.merge(pp.dropna(subset=["pred"]), on=names, how="outer")
        else:
            data["pred"], data["pred_err"] = pred, err
        data["residual"] = data["data"] - data["pred"]
        # the reference's xr.merge(...).to_dataframe() + outer merge hands the rows back sorted by the coordinates
        # (src/joint_prediction.py:248-254)
        data = data.sort_values(names, kind="stable").reset_index(drop=True)
        cols = names + ["data", "pred", "residual", "pred_err"]
        return data[cols] if fold is None else data[cols + ["fold"]]

    def _cv_folds(self, i, postprocess, refactor_each, folds, also_withhold, seed):
        """The ``folds=`` form of ``cross_validation``: everything is validated on the host before any device work."""
        if self.devices is not None and len(self.devices) > 1:
            raise ValueError(f"cross_validation(folds=...) runs on a single device; this predictor has devices={self.devices}")
        if not 0 <= int(i) < self.n_procs:
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        f = self.mf.fields[i]
        n_i = len(np.asarray(f.values_main))
        n_o = len(np.asarray(self.mf.fields[1 - i].values_main)) if self.n_procs == 2 else 0
        codes, codes_o, labels = fold_codes(folds, also_withhold, n_i, n_o if self.n_procs == 2 else None, seed)
        names = ["lat", "lon"] if postprocess else ["d1", "d2"]
        data = pd.DataFrame(np.hstack((f.coords_main, np.atleast_2d(f.values_main).T)), columns=names + ["data"])
        K = len(labels)
        sizes = np.bincount(codes[codes >= 0], minlength=K) + (0 if codes_o is None else np.bincount(codes_o[codes_o >= 0], minlength=K))
        if refactor_each:
            pred, err = np.full(n_i, np.nan), np.full(n_i, np.nan)
            nlpd, failed = np.full(K, np.nan), np.zeros(K, dtype=bool)
            for k in range(K):
                sel = np.flatnonzero(codes == k)
                drop = [sel if q == i else (np.flatnonzero(codes_o == k) if codes_o is not None else np.empty(0, dtype=int))
                        for q in range(self.n_procs)]
                h = native.Handle(self.device)
                try:
                    configure_handle(h, self.mod)
                    h.set_metric(metric_of(self.dist_units, self.fast_dist))
                    for q in range(self.n_procs):
                        c = np.asarray(self.mf.fields[q].coords_main, dtype=np.float64)
                        v = np.asarray(self.mf.fields[q].values_main, dtype=np.float64)
                        h.set_data(q, np.delete(c, drop[q], axis=0), np.delete(v, drop[q], axis=0))
                    self._set_noise(h, drop)
                    pred[sel], err[sel] = self._factor_predict(h, i, np.ascontiguousarray(np.asarray(f.coords_main, dtype=np.float64)[sel]))
                finally:
                    h.close()
        else:
            h = self._factored_handle()
            info, pred, err, stats = h.cv_folds(i, codes, codes_o, n_folds=K, want_stats=True)
            self.timings = h.cv_folds_timings()
            failed = np.isnan(stats[:, 1])
            nlpd = 0.5 * (stats[:, 0] * np.log(2.0 * np.pi) - stats[:, 1] + stats[:, 2])
            if info != 0:
                bad = [labels[k] for k in np.flatnonzero(failed)]
                warnings.warn(f"cross_validation: the withheld data of {len(bad)} fold(s) have no positive definite conditional "
                              f"precision (first: fold {labels[info - 1]!r}); their rows are NaN")
        self.cv_folds_ = pd.DataFrame({"label": pd.Series(labels, dtype=object), "n_withheld": sizes.astype(int), "nlpd": nlpd,
                                       "failed": failed})
        data["fold"] = pd.Series([labels[c] if c >= 0 else None for c in codes], dtype=object)
        keep = codes >= 0
        if postprocess:
            out = self._cv_frame(i, True, data, names, pred, err, fold=True)
            return out[out["fold"].notna()].reset_index(drop=True)
        data = data[keep].reset_index(drop=True)
        return self._cv_frame(i, False, data, names, pred[keep], err[keep], fold=True)


CK_FOLD_MAX = 4096   # include/cokrige.h


def _is_missing(x):
    if x is None:
        return True
    try:
        if x != x:   # NaN
            return True
        return bool(x == -1) and not isinstance(x, (str, bytes))
    except Exception:
        return False


def fold_codes(folds, also_withhold, n_i, n_other, seed=0, fold_max=CK_FOLD_MAX):
    """(codes_i, codes_other or None, labels): the fold labels of ``cross_validation(folds=...)`` as the int32 codes of
    ``ck_cv_folds``.  Labels are numbered in order of first appearance in ``folds``; None / NaN / -1 -> -1 (never withheld).
    An int K draws a random K-fold from ``seed``: a permutation of the data cut into K nearly equal parts.  Raises
    ValueError for wrong lengths, ``also_withhold`` labels that are no label of ``folds``, an empty fold set and folds of
    more than ``fold_max`` data (CK_FOLD_MAX, the dense call's cap; None: no cap -- the local predictor has none).  Host only."""
    if folds is None:
        raise ValueError("also_withhold needs folds")
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
        K = int(folds)
        if not 1 <= K <= n_i:
            raise ValueError(f"folds={K}: a K-fold of {n_i} data needs 1 <= K <= {n_i}")
        perm = np.random.default_rng(seed).permutation(n_i)
        codes = np.empty(n_i, dtype=np.int32)
        codes[perm] = (np.arange(n_i) * K // n_i).astype(np.int32)
        labels = list(range(K))
    else:
        raw = list(folds) if not isinstance(folds, np.ndarray) else folds.tolist()
        if len(raw) != n_i:
            raise ValueError(f"folds has {len(raw)} labels, the predicted process has {n_i} data")
        index, labels = {}, []
        codes = np.empty(n_i, dtype=np.int32)
        for a, x in enumerate(raw):
            if _is_missing(x):
                codes[a] = -1
                continue
            if x not in index:
                index[x] = len(labels)
                labels.append(x)
            codes[a] = index[x]
    if not labels:
        raise ValueError("folds withholds nothing: every label is None / NaN / -1")
    codes_o = None
    if also_withhold is not None:
        if n_other is None:
            raise ValueError("also_withhold needs a second process")
        raw = list(also_withhold) if not isinstance(also_withhold, np.ndarray) else also_withhold.tolist()
        if len(raw) != n_other:
            raise ValueError(f"also_withhold has {len(raw)} labels, the other process has {n_other} data")
        index = {x: k for k, x in enumerate(labels)}
        codes_o = np.empty(n_other, dtype=np.int32)
        for a, x in enumerate(raw):
            if _is_missing(x):
                codes_o[a] = -1
            elif x in index:
                codes_o[a] = index[x]
            else:
                raise ValueError(f"also_withhold label {x!r} (datum {a}) is no label of folds")
    sizes = np.bincount(codes[codes >= 0], minlength=len(labels))
    if codes_o is not None:
        sizes = sizes + np.bincount(codes_o[codes_o >= 0], minlength=len(labels))
    big = np.flatnonzero(sizes > fold_max) if fold_max is not None else []
    if len(big):
        raise ValueError(f"fold {labels[big[0]]!r} withholds {int(sizes[big[0]])} data; the cap is CK_FOLD_MAX = {fold_max} per fold")
    return codes, codes_o, labels


def prediction_coords(extents: tuple = (-125, -65, 22, 58), lon_res: float = 0.5, lat_res: float = 0.5,
                      land_only: bool = True) -> pd.DataFrame:
    """Prediction grid [lat, lon] (src/joint_prediction.py:277-283).  The reference keeps land
    cells only, through regionmask's Natural Earth polygons; where regionmask is not
    installed ask for the full rectangle with ``land_only=False``."""
    lon = np.arange(extents[0], extents[1] + 0.5 * lon_res, lon_res)
    lat = np.arange(extents[2], extents[3] + 0.5 * lat_res, lat_res)
    if land_only:
        try:
            import regionmask  # noqa: F401
        except Exception as e:
            raise RuntimeError("land masking needs regionmask (as in the reference); "
                               "use land_only=False for the full rectangle") from e
        land = regionmask.defined_regions.natural_earth_v5_0_0.land_110
        mask = land.mask(lon, lat)
        la, lo = np.meshgrid(lat, lon, indexing="ij")
        ok = ~np.isnan(np.asarray(mask))
        return pd.DataFrame({"lat": la[ok], "lon": lo[ok]})
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    return pd.DataFrame({"lat": la.ravel(), "lon": lo.ravel()})
