"""Local-neighbourhood cokriging -- same call signatures as the reference's ``point_prediction``
module (src/point_prediction.py), one GPU workgroup per prediction point.

    from sif_xco2_cokriging_amd import point_prediction as prediction
    P = prediction.Predictor(mod, mf)
    ds = P(0, pcoords, max_dist=1e3, postprocess=False)

Differences from the reference, none in the arithmetic:
  * no global ``Sigma`` blocks are precomputed or gathered (src/point_prediction.py:98-113,
    153-181): each workgroup assembles the covariance of its own neighbours;
  * ``partitions`` (a ``multiprocessing.Pool`` in the reference, :69-81) is accepted and ignored:
    the prediction points are already processed in parallel;
  * the reference warns once per affected point (:219-221, 230-232); here one warning per
    call and kind, carrying the number of points;
  * ``trend=`` (not in the reference): ordinary / universal cokriging in the moving neighbourhood -- the unknown mean is
    estimated by GLS in every neighbourhood and its uncertainty is part of ``pred_err``;
  * ``max_neighbours=`` (not in the reference): a nearest-neighbour cap per process inside ``max_dist``, so that the radius
    can be chosen for coverage of sparse regions instead of for cost;
  * ``predict_blocks`` (not in the reference): weighted means over blocks of sites with the standard error of the mean,
    from the neighbourhood of each block's search centre; no covariance between blocks;
  * ``predict_pair`` (not in the reference): both processes at every site from one local system, with the covariance of
    their two prediction errors there; no covariance between sites.
"""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd

from . import native
from .fields import metric_of
from .joint_prediction import Predictor as _JointPredictor
from .joint_prediction import fold_codes, prediction_coords, xr  # noqa: F401  (same helpers, same signatures)
from .model import configure_handle
from .noise import apply_noise, resolve_measurement_error
from .trend import TrendDesign, check_trend


def check_max_neighbours(max_neighbours, n_procs):
    """None, an int (every process) or one int per process -> a pair of caps (0 = none), or None."""
    if max_neighbours is None:
        return None
    vals = [max_neighbours] * n_procs if np.isscalar(max_neighbours) else list(max_neighbours)
    if len(vals) != n_procs:
        raise ValueError(f"max_neighbours needs one value per process ({n_procs}), got {len(vals)}")
    for v in vals:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"max_neighbours must be integers, got {v!r}")
        if v < 0:
            raise ValueError(f"max_neighbours must be >= 0 (0 = no cap), got {v!r}")
    return tuple(int(v) for v in vals) + (0,) * (2 - n_procs)


class Predictor:
    """Multivariate prediction framework (src/point_prediction.py:21-43)."""

    def __init__(self, mod, mf, covariates=None, dist_units: str = "km", fast_dist: bool = True, device: int = 0,
                 devices=None, reserve_scratch=None, trend=None, measurement_error=None, noise_scale=(1.0, 1.0),
                 max_neighbours=None):
        """``devices=[0, 1, ...]``: the prediction points are sharded over one worker process per GPU (observations
        replicated, no exchange inside the computation) -- what ``partitions`` is to the reference's CPU pool
        (src/point_prediction.py:45-52, 69-81).

        ``trend``: None (simple cokriging: a known zero mean in every neighbourhood), ``"constant"`` (ordinary cokriging in
        the moving window), ``"linear"`` or a callable ``f(k, coords) -> (n, p_k)``, as for the joint predictor.  The trend
        is estimated by GLS in every neighbourhood (include/cokrige.h: ck_predict_local_universal); a site whose
        neighbourhood cannot carry it (rank deficient), or whose regressors are not finite, gets NaN.  After a call
        ``trend_coef`` holds the (m, p) local coefficients.

        ``measurement_error`` / ``noise_scale``: as for the joint predictor -- every neighbour's ``noise_scale[k] * d_a``
        goes on the diagonal of its local system (include/cokrige.h: ck_set_noise).  Single-device only.

        ``max_neighbours``: None, an int (applies to every process) or one int per process: of the sites of a process within
        ``max_dist`` only the nearest so many are used -- with every site tied at the cut distance, so a neighbourhood may hold
        a few more (include/cokrige.h: ck_set_local_neighbours); 0 = no cap for that process.  The cap is per process because
        the denser process would otherwise crowd the other out of the list.  After a call ``info["n_capped"]`` is the number
        of points where a cap was binding.  Single-device only."""
        if mod.n_procs != mf.n_procs:
            raise ValueError("Number of theoretical processes different from empirical processes.")
        self.measurement_error, self.noise_scale = measurement_error, noise_scale
        resolve_measurement_error(measurement_error, noise_scale, mf.fields, devices)   # refusals before any device work
        self.trend = check_trend(trend)
        if self.trend is not None and devices is not None and len(devices) > 1:
            raise NotImplementedError("universal cokriging (trend=...) runs on one device; the multi-GPU path is simple "
                                      "cokriging only")
        self.max_neighbours = check_max_neighbours(max_neighbours, mod.n_procs)
        if self.max_neighbours is not None and devices is not None and len(devices) > 1:
            raise NotImplementedError("the neighbour cap (max_neighbours=...) runs on one device; the multi-GPU path has none")
        self.trend_coef = None
        self.n_procs = mod.n_procs
        self.mod, self.mf, self.covariates = mod, mf, covariates
        self.dist_units, self.fast_dist = dist_units, fast_dist
        self.devices = None if devices is None else [int(d) for d in devices]
        self.device = device if self.devices is None else self.devices[0]
        self._pool, self._pool_key = None, None
        self.cv = False  # placeholder for cross-validation (src/point_prediction.py:43)
        self.info = {}
        self._h = None
        self._key = None
        # The reference builds its state -- the full Sigma blocks -- here, once (src/point_prediction.py:24-43).  Ours is the
        # scratch slab of the large-neighbourhood paths: reserve_scratch = bytes, or "auto" for the library's budget (a quarter
        # of the free device memory, at most 32 GiB), allocates it now so that no later call pays a hipMalloc of tens of GiB
        # (up to seconds: include/cokrige.h, ck_local_reserve); None (default): grown by the first call that needs it.
        self.reserve_scratch = reserve_scratch
        if reserve_scratch is not None and (self.devices is None or len(self.devices) <= 1):
            self._handle()

    def _handle(self):
        key = _JointPredictor._state_key(self)   # model parameters, metric, data: a change rebuilds the device state
        if self._h is not None and key != self._key:
            self._h.close()
            self._h = None
        self._key = key
        if self._h is None:
            h = native.Handle(self.device)
            configure_handle(h, self.mod)
            h.set_metric(metric_of(self.dist_units, self.fast_dist))
            for k in range(self.n_procs):
                h.set_data(k, self.mf.fields[k].coords_main, self.mf.fields[k].values_main)
            apply_noise(h, *resolve_measurement_error(self.measurement_error, self.noise_scale, self.mf.fields, self.devices))
            if self.reserve_scratch is not None:
                h.local_reserve(0 if self.reserve_scratch == "auto" else int(self.reserve_scratch))
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
        if self._pool is not None:
            self._pool.close()
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _predict_on_ranks(self, i, pcoords, max_dist):
        from . import workers
        from .model import model_arrays
        key = _JointPredictor._state_key(self)
        if self._pool is None:
            self._pool = workers.RankPool(self.devices)
        if key != self._pool_key:
            self._pool.load(model_arrays(self.mod), metric_of(self.dist_units, self.fast_dist),
                            [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64) for k in range(self.n_procs)],
                            [np.asarray(self.mf.fields[k].values_main, dtype=np.float64) for k in range(self.n_procs)])
            self._pool_key = key
        return self._pool.predict_local(i, pcoords, max_dist=max_dist, cv=self.cv)

    def _capped_handle(self):
        """The handle with this predictor's neighbour cap on it (set before every local call: it is handle state)."""
        h = self._handle()
        h.set_local_neighbours(*(self.max_neighbours or (0, 0)))
        return h

    def _predict_universal(self, i, pcoords, max_dist):
        """The regressors of the data and the prediction sites are validated on the host, then set on the handle (a new
        trend needs no new device state)."""
        if not 0 <= int(i) < self.n_procs:
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        coords = [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)]
        design = TrendDesign(self.trend, coords)
        F = [design.data(k, coords[k]) for k in range(self.n_procs)]
        pc = np.ascontiguousarray(np.atleast_2d(np.asarray(pcoords, dtype=np.float64))[:, :2])
        F0 = design(i, pc)
        h = self._capped_handle()
        for k in range(self.n_procs):
            h.set_trend(k, F[k])
        pred, err, info = h.predict_local_universal(i, pc, F0, max_dist=max_dist, cv=self.cv, want_beta=True)
        self.trend_coef = info.pop("beta")
        return pred, err, info

    def predict_arrays(self, i: int, pcoords, max_dist: float = 1e3):
        if self.trend is not None:
            pred, err, info = self._predict_universal(i, pcoords, max_dist)
        elif self.devices is not None and len(self.devices) > 1:
            pred, err, info = self._predict_on_ranks(i, pcoords, max_dist)
        else:
            pred, err, info = self._capped_handle().predict_local(i, pcoords, max_dist=max_dist, cv=self.cv)
        info["n_capped"] = int(self._h.timings()["local_n_capped"]) if self.max_neighbours is not None else 0
        self.info = info
        if info["n_empty"]:
            warnings.warn(f"No data within maximum distance {max_dist} at {info['n_empty']} location(s).")
        if info["n_not_pd"]:
            warnings.warn(f"Local covariance matrix not positive definte at {info['n_not_pd']} location(s);"
                          " returning NaN.")
        if info.get("n_rank_def"):
            warnings.warn(f"Trend not estimable from the data within maximum distance {max_dist} at {info['n_rank_def']}"
                          " location(s); returning NaN. Use a larger max_dist or a smaller trend.")
        return pred, err

    def __call__(self, i: int, pcoords: pd.DataFrame, max_dist: float = 1e3, partitions: int = None,
                 postprocess: bool = True):
        """src/point_prediction.py:45-96."""
        self.i = i
        if not isinstance(pcoords, pd.DataFrame):
            a = np.atleast_2d(np.asarray(pcoords, dtype=np.float64))
            pcoords = pd.DataFrame({"d1": a[:, 0], "d2": a[:, 1]})
        pred, err = self.predict_arrays(i, pcoords.values[:, :2], max_dist=max_dist)
        df = pcoords.copy()
        df["pred"], df["pred_err"] = pred, err
        if postprocess:
            return _JointPredictor._postprocess_predictions(self, df)
        out = df.set_index(pcoords.columns.values.tolist())
        if xr is None:
            return out
        ds = out.to_xarray()
        ts = self.mf.fields[self.i].timestamp
        try:
            np.isnan(ts)
            return ds
        except TypeError:
            return ds.assign_coords(coords={"time": np.datetime64(ts)})

    # -- both processes at once ----------------------------------------------------------------------
    def predict_pair_arrays(self, pcoords, max_dist: float = 1e3):
        """Both processes at every site from ONE neighbourhood, local Sigma and Cholesky per site -- the numeric body of
        ``predict_pair`` (include/cokrige.h: ck_predict_local_pair).  Returns (pred_0, pred_err_0, pred_1, pred_err_1, cov):
        cov[t] the covariance of the two prediction errors at site t.  pred / pred_err carry the bits of ``predict_arrays``
        (cross-validation off) for either process; ``info`` and the warnings are its.  Runs on one device: with several
        ``devices=[...]`` it raises NotImplementedError, as ``predict_blocks`` does."""
        if self.devices is not None and len(self.devices) > 1:
            raise NotImplementedError(f"predict_pair runs on one device; this predictor has devices={self.devices}")
        if self.trend is not None:
            raise NotImplementedError("the joint prediction of both processes in the moving neighbourhood is simple cokriging "
                                      "only (trend=None)")
        if self.n_procs != 2:
            raise ValueError(f"the joint prediction of both processes needs a model of two processes, not {self.n_procs}")
        if isinstance(max_dist, bool) or not np.isfinite(max_dist) or max_dist < 0:
            raise ValueError(f"max_dist must be finite and >= 0, got {max_dist!r}")
        pc = np.atleast_2d(np.asarray(pcoords, dtype=np.float64))
        if pc.ndim != 2 or pc.shape[1] < 2 or len(pc) < 1:
            raise ValueError("pcoords must be [[lat, lon], ...] with at least one site")
        h = self._capped_handle()
        p0, e0, p1, e1, cov, info = h.predict_local_pair(np.ascontiguousarray(pc[:, :2]), max_dist=max_dist)
        self.timings = h.local_pair_timings()
        info["n_capped"] = int(h.timings()["local_n_capped"]) if self.max_neighbours is not None else 0
        self.info = info
        if info["n_empty"]:
            warnings.warn(f"No data within maximum distance {max_dist} at {info['n_empty']} location(s).")
        if info["n_not_pd"]:
            warnings.warn(f"Local covariance matrix not positive definte at {info['n_not_pd']} location(s);"
                          " returning NaN.")
        return p0, e0, p1, e1, cov

    def predict_pair(self, pcoords, max_dist: float = 1e3, postprocess: bool = True, pcoords1=None):
        """Prediction and standard error of BOTH processes at ``pcoords`` with the covariance of their prediction errors, for
        data beyond the size of the joint predictor.  Both processes at a site share one neighbourhood (with cross-validation
        off it does not depend on the predicted process), so (pred_0, pred_1) is the simple-cokriging predictor from one data
        subset and [[pred_err_0^2, pred_cov], [pred_cov, pred_err_1^2]] a genuine conditional covariance.  Returns what
        ``joint_prediction.Predictor.predict_pair`` returns for one site set: ``pred_0``, ``pred_err_0``, ``pred_1``,
        ``pred_err_1``, ``pred_cov`` and ``pred_corr`` (NaN where an error is 0); ``postprocess`` transforms each process as
        ``__call__`` does and scales the covariance by the product of the two ``scale_fact``s.

        A second site set (``pcoords1``) is refused: sites apart have different neighbourhoods, and a covariance between
        predictions from different data subsets is the posterior covariance of nothing (the joint predictor has one).
        Honours ``measurement_error=`` and ``max_neighbours=``; ``trend=`` raises NotImplementedError."""
        if pcoords1 is not None:
            raise ValueError("predict_pair in the moving neighbourhood takes one site set: two sites apart have different "
                             "neighbourhoods, which give no posterior covariance between them (joint_prediction.Predictor."
                             "predict_pair on a factored Sigma has one); call it once per site set")
        if self.trend is not None:
            raise NotImplementedError("the joint prediction of both processes in the moving neighbourhood is simple cokriging "
                                      "only (trend=None)")
        f0 = _JointPredictor._sites_frame(pcoords)
        p0, e0, p1, e1, cov = self.predict_pair_arrays(f0.values[:, :2], max_dist=max_dist)
        return _JointPredictor._pair_output(self, f0, None, p0, e0, p1, e1, cov, None, postprocess)

    # -- areal means in the moving neighbourhood ---------------------------------------------------
    _spatial_trend = _JointPredictor._spatial_trend   # what _postprocess_blocks reads of the class it is borrowed from
    _postprocess_predictions = _JointPredictor._postprocess_predictions   # and what _cv_frame does (cross_validation(folds=...))

    def _block_centres(self, pc, codes, labels, centres):
        """(r, 2) search centres in the order of ``labels``.  None: the unweighted mean position of every block's members --
        on the sphere the normalised mean of their unit vectors, else the coordinate mean."""
        r = len(labels)
        if centres is None:
            n_b = np.bincount(codes, minlength=r)
            if metric_of(self.dist_units, self.fast_dist) != 0:   # Euclidean
                return np.column_stack([np.bincount(codes, weights=pc[:, c], minlength=r) / n_b for c in range(2)])
            la, lo = np.radians(pc[:, 0]), np.radians(pc[:, 1])
            u = np.column_stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
            mu = np.column_stack([np.bincount(codes, weights=u[:, c], minlength=r) / n_b for c in range(3)])
            nrm = np.linalg.norm(mu, axis=1)
            if np.any(nrm < 1e-12):
                bad = labels[int(np.flatnonzero(nrm < 1e-12)[0])]
                raise ValueError(f"the members of block {bad!r} have no mean direction on the sphere (their unit vectors "
                                 "cancel); pass its search centre through centres=")
            mu /= nrm[:, None]
            return np.column_stack([np.degrees(np.arcsin(np.clip(mu[:, 2], -1.0, 1.0))), np.degrees(np.arctan2(mu[:, 1], mu[:, 0]))])
        if hasattr(centres, "keys"):
            missing = [lab for lab in labels if lab not in centres]
            if missing:
                raise ValueError(f"centres has no entry for block {missing[0]!r}")
            cc = np.array([np.asarray(centres[lab], dtype=np.float64).ravel()[:2] for lab in labels], dtype=np.float64)
        else:
            cc = np.atleast_2d(np.asarray(centres, dtype=np.float64))
        if cc.shape != (r, 2):
            raise ValueError(f"centres has shape {cc.shape}, expected {(r, 2)}: one (lat, lon) per block, sorted labels' order")
        if not np.all(np.isfinite(cc)):
            bad = labels[int(np.flatnonzero(~np.all(np.isfinite(cc), axis=1))[0])]
            raise ValueError(f"the search centre of block {bad!r} is not finite")
        return np.ascontiguousarray(cc)

    def predict_blocks(self, i: int, pcoords, blocks, weights=None, max_dist: float = 1e3, centres=None,
                       postprocess: bool = True):
        """Weighted means of process ``i`` over blocks of sites, each with the standard error of the mean, from the data
        around the block -- block cokriging in a moving neighbourhood (gstat's ``block=`` with ``nmax`` / ``maxdist``;
        include/cokrige.h: ck_predict_local_blocks).  No Sigma is needed, so this is the areal product for data beyond the
        size of the joint predictor.

        ``blocks[a]`` names the block of site ``pcoords[a]`` (any hashable; NaN / None leaves the site out), ``weights[a]``
        its weight (default 1 / n_b).  The neighbourhood of a block is that of its search centre, a POINT: the data within
        ``max_dist`` of it, under ``max_neighbours`` -- not the union of the members' neighbourhoods.  ``centres``: None (the
        unweighted mean position of the members; on the sphere the normalised mean of their unit vectors), an (r, 2) array
        in the order of the sorted labels, or a mapping label -> (lat, lon).  ``max_dist`` should reach well beyond the
        block's own extent.

        The standard error accounts for the correlation between the members; the ``pred_err`` of a block's points cannot be
        combined into it.  No covariance BETWEEN blocks is offered: different blocks have different neighbourhoods, so such a
        matrix would be the posterior covariance of nothing (``joint_prediction.Predictor.predict_blocks`` has one).

        Honours ``trend=`` (block regressors sum_a w_a f(i, x_a); ``trend_coef`` becomes (r, p)), ``measurement_error=`` /
        ``noise_scale=`` and ``max_neighbours=``; ``info`` and the warnings are those of ``predict_arrays``.  Returns a
        DataFrame indexed by the sorted labels with ``pred``, ``pred_err``, ``n_sites``, ``lat``, ``lon`` (the weighted
        centroid), as the joint method; ``postprocess=True`` is its arithmetic too."""
        if self.devices is not None and len(self.devices) > 1:
            raise NotImplementedError(f"predict_blocks runs on one device; this predictor has devices={self.devices}")
        if isinstance(i, bool) or not (isinstance(i, (int, np.integer)) and 0 <= int(i) < self.n_procs):
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        pc, codes, w, labels, _ = _JointPredictor._block_layout(pcoords, blocks, weights)
        r = len(labels)
        cc = self._block_centres(pc, codes, labels, centres)
        h = self._capped_handle()
        F0 = None
        if self.trend is not None:
            coords = [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)]
            design = TrendDesign(self.trend, coords)
            F = [design.data(k, coords[k]) for k in range(self.n_procs)]
            Fm = design(i, pc)
            F0 = np.column_stack([np.bincount(codes, weights=w * Fm[:, j], minlength=r) for j in range(Fm.shape[1])]) \
                if Fm.shape[1] else np.zeros((r, 0))
            for k in range(self.n_procs):
                h.set_trend(k, F[k])
        pred, err, info = h.predict_local_blocks(i, cc, pc, codes, w, f0=F0, max_dist=max_dist, want_beta=self.trend is not None)
        self.trend_coef = info.pop("beta", None)
        info["n_capped"] = int(h.timings()["local_n_capped"]) if self.max_neighbours is not None else 0
        self.info = info
        if info["n_empty"]:
            warnings.warn(f"No data within maximum distance {max_dist} at {info['n_empty']} location(s).")
        if info["n_not_pd"]:
            warnings.warn(f"Local covariance matrix not positive definte at {info['n_not_pd']} location(s);"
                          " returning NaN.")
        if info.get("n_rank_def"):
            warnings.warn(f"Trend not estimable from the data within maximum distance {max_dist} at {info['n_rank_def']}"
                          " location(s); returning NaN. Use a larger max_dist or a smaller trend.")
        n_sites = np.bincount(codes, minlength=r)
        sw = np.bincount(codes, weights=w, minlength=r)
        with np.errstate(invalid="ignore", divide="ignore"):
            lat = np.bincount(codes, weights=w * pc[:, 0], minlength=r) / sw
            lon = np.bincount(codes, weights=w * pc[:, 1], minlength=r) / sw
        if postprocess:
            self.i = i
            pred, err, _ = _JointPredictor._postprocess_blocks(self, pc, codes, w, r, pred, err, None)
        index = labels.copy()
        if index.nlevels == 1:
            index.name = "block"
        return pd.DataFrame({"pred": pred, "pred_err": err, "n_sites": n_sites, "lat": lat, "lon": lon}, index=index)

    # -- conditional simulation in the moving neighbourhood ----------------------------------------
    def _sim_sites(self, pcoords, what="pcoords"):
        pc = np.atleast_2d(np.asarray(pcoords.values if isinstance(pcoords, pd.DataFrame) else pcoords, dtype=np.float64))
        if pc.ndim != 2 or pc.shape[1] < 2 or len(pc) < 1:
            raise ValueError(f"{what} must be [[lat, lon], ...] with at least one site")
        return np.ascontiguousarray(pc[:, :2])

    def _sim_pins(self, q, pc):
        """The sites of process q that the native call does not simulate: (source, on_datum, datum_value) -- for every row the
        first row with its coordinates, whether it lies on a datum of process q without measurement-error variance, and that
        datum's value (NaN elsewhere)."""
        m = len(pc)
        pair = [("a", np.float64), ("b", np.float64)]
        rows = pc.view(pair).ravel()
        _, first, inv = np.unique(rows, return_index=True, return_inverse=True)
        source = first[np.asarray(inv).ravel()]                 # caller's site -> the first row with its coordinates
        f = self.mf.fields[q]
        dc = np.ascontiguousarray(np.asarray(f.coords_main, dtype=np.float64)[:, :2])
        dv = np.asarray(f.values_main, dtype=np.float64).ravel()
        var, scales = resolve_measurement_error(self.measurement_error, self.noise_scale, self.mf.fields, self.devices)
        exact = np.ones(len(dc), dtype=bool) if var is None or var[q] is None else ~(scales[q] * var[q] > 0.0)
        drows = dc[exact].view(pair).ravel()
        du, dfirst = np.unique(drows, return_index=True)
        at = np.searchsorted(du, rows)
        on_datum = (at < len(du)) & (du[np.minimum(at, max(len(du) - 1, 0))] == rows) if len(du) else np.zeros(m, dtype=bool)
        datum_value = np.where(on_datum, dv[exact][dfirst[np.minimum(at, max(len(du) - 1, 0))]] if len(du) else 0.0, np.nan)
        return source, on_datum, datum_value

    def conditional_draws_arrays(self, i, pcoords, max_dist: float, n_draws: int, seed=None, ordering="random", noise=None,
                                 pcoords1=None):
        """Draws of process ``i`` at ``pcoords`` by sequential simulation in the moving neighbourhood -- the numeric body of
        ``conditional_simulation`` (include/cokrige.h: ck_simulate_local; gstat's ``nsim`` with ``nmax`` / ``maxdist``).

        ``i=(0, 1)``: the co-simulation of BOTH processes (ck_simulate_local_pair) -- process 0 at ``pcoords``, process 1 at
        ``pcoords1`` (None: the same sites), stacked: column k is site k of process 0, column m0 + k site k of process 1.  A
        stacked site is conditioned on the data and on the earlier stacked sites of either process, so every draw is a jointly
        consistent pair of maps; two single calls give two independent ensembles.  ``noise`` is then (n_draws, m0 + m1) with
        process 0's columns first, an array ``ordering`` holds m0 + m1 ranks, and "random" permutes the stacked sites.

        The sites are visited in ``ordering``: "random" (the default, ``np.random.default_rng(seed).permutation``), "hilbert"
        (along the library's Hilbert curve; far more levels of the recursion, so slower) or an array of m distinct integer ranks.
        Every site is conditioned on the data and on the sites visited before it, within ``max_dist`` and under the Predictor's
        ``max_neighbours`` -- the cap counts data and already simulated sites of a process alike.  A conditioning set holds
        at most 64 members: choose the caps or the radius accordingly.

        Set aside before the native call, and counted in ``sim_info["n_pinned"]``: rows of a process's sites that repeat an
        earlier row (one random variable: they get the draws of the first occurrence) and sites on a datum of their process without
        measurement-error variance (every draw is that datum's value).  ``noise`` (n_draws, m) in the caller's sites replaces
        the device's Philox stream (a set-aside site's column is not used); that stream is keyed on ``seed`` and on the index
        among the sites that remain.  ``seed=None`` takes 64 bits from ``numpy.random.SeedSequence()``.

        ``pred`` / ``pred_err`` are ``predict_arrays``' values at the same sites under the same caps.  The mean of the ensemble
        equals ``pred`` only in the full-conditioning limit (every datum and every earlier site in every set): a site's set
        also holds earlier sites, which take places under the cap that data would have had.

        Returns (draws (n_draws, m), pred, pred_err, pinned (bool, m), seed); ``sim_info`` holds seed, ordering, n_levels,
        n_empty, n_pinned, k_max and n_capped, ``timings`` the native call's.  Raises ValueError on bad arguments before any
        device work and numpy.linalg.LinAlgError when a site's local system is not positive definite."""
        from numpy.linalg import LinAlgError

        from .vecchia import check_ordering, ordering_ranks
        if self.devices is not None and len(self.devices) > 1:
            raise NotImplementedError(f"conditional simulation runs on one device; this predictor has devices={self.devices}")
        if self.trend is not None:
            raise NotImplementedError("conditional simulation in the moving neighbourhood is simple cokriging only (trend=None)")
        joint = isinstance(i, (tuple, list))
        if joint:
            if tuple(i) != (0, 1) or any(isinstance(k, bool) for k in i):
                raise ValueError(f"process index {i!r}: the joint form is i=(0, 1)")
            if self.n_procs != 2:
                raise ValueError(f"the co-simulation of both processes needs a model of two processes, not {self.n_procs}")
            procs = [0, 1]
            pcs = [self._sim_sites(pcoords)]
            pcs.append(pcs[0] if pcoords1 is None else self._sim_sites(pcoords1, "pcoords1"))
        else:
            if isinstance(i, bool) or not (isinstance(i, (int, np.integer)) and 0 <= int(i) < self.n_procs):
                raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
            if pcoords1 is not None:
                raise ValueError("pcoords1 belongs to the joint form i=(0, 1)")
            procs, pcs = [int(i)], [self._sim_sites(pcoords)]
        offs = np.concatenate([[0], np.cumsum([len(pc) for pc in pcs])])
        m = int(offs[-1])
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or n_draws < 1:
            raise ValueError(f"n_draws must be an integer >= 1, not {n_draws!r}")
        n_draws = int(n_draws)
        if isinstance(max_dist, bool) or not np.isfinite(max_dist) or max_dist < 0:
            raise ValueError(f"max_dist must be finite and >= 0, got {max_dist!r}")
        if noise is not None:
            noise = np.asarray(noise, dtype=np.float64)
            if noise.shape != (n_draws, m):
                raise ValueError(f"noise has shape {noise.shape}, expected (n_draws, m) = {(n_draws, m)}")
        ordering = check_ordering(ordering)
        if isinstance(ordering, np.ndarray) and ordering.size != m:
            raise ValueError(f"the ordering has {ordering.size} ranks, pcoords {m} sites")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2^64)")
        seed = int(seed)
        # per process: sites that repeat an earlier row, sites on a noise-free datum; everything below in stacked indices
        pins = [self._sim_pins(q, pc) for q, pc in zip(procs, pcs)]
        source = np.concatenate([offs[j] + pins[j][0] for j in range(len(procs))])
        on_datum = np.concatenate([p[1] for p in pins])
        datum_value = np.concatenate([p[2] for p in pins])
        free = np.flatnonzero((source == np.arange(m)) & ~on_datum)   # what the native call simulates, the caller's order
        pinned = np.ones(m, dtype=bool)
        pinned[free] = False
        was_cv, self.cv = self.cv, False   # the sites' ordinary prediction, whatever cross_validation left behind
        try:
            parts = [self.predict_arrays(q, pc, max_dist=max_dist) for q, pc in zip(procs, pcs)]
        finally:
            self.cv = was_cv
        pred, err = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        draws = np.empty((n_draws, m))
        stats = dict(n_levels=0, n_empty=0, k_max=0, n_capped=0)
        if len(free):
            allpc = np.vstack(pcs)
            fq = [free[(free >= offs[j]) & (free < offs[j + 1])] for j in range(len(procs))]   # the free sites by process
            if isinstance(ordering, np.ndarray):
                ranks = ordering[free]
            else:
                ranks = ordering_ranks([allpc[f] for f in fq], ordering, seed % (2 ** 63))
            h = self._capped_handle()
            e = None if noise is None else np.ascontiguousarray(noise[:, free])
            if joint:
                sub, info, stats = h.simulate_local_pair(allpc[fq[0]], allpc[fq[1]], ranks, float(max_dist), n_draws, seed=seed, noise=e,
                                                         terms=False)
            else:
                sub, info, stats = h.simulate_local(procs[0], allpc[free], ranks, float(max_dist), n_draws, seed=seed, noise=e,
                                                    terms=False)
            self.timings = h.simulate_local_timings()
            if info != 0:
                site = int(free[info - 1])
                j = int(np.searchsorted(offs, site, side="right") - 1)
                raise LinAlgError(f"the local system of site {site - int(offs[j])} {tuple(allpc[site])}"
                                  + (f" of process {procs[j]}" if joint else "") + " is not positive definite or leaves no "
                                  "variance: nearly coincident sites, or a site nearly on a noise-free datum")
            draws[:, free] = sub
        on = np.flatnonzero(on_datum)
        draws[:, on] = datum_value[on]
        rest = np.flatnonzero(pinned & ~on_datum)
        draws[:, rest] = draws[:, source[rest]]
        self.sim_info = dict(seed=seed, ordering=ordering if isinstance(ordering, str) else "ranks", n_levels=stats["n_levels"],
                             n_empty=stats["n_empty"], n_pinned=int(pinned.sum()), k_max=stats["k_max"], n_capped=stats["n_capped"])
        return draws, pred, err, pinned, seed

    def conditional_simulation(self, i, pcoords, max_dist: float = 1e3, n_draws: int = 100, seed=None, ordering="random",
                               postprocess: bool = True, noise=None, pcoords1=None):
        """Ensembles of maps of process ``i`` at ``pcoords`` drawn in the moving neighbourhood: the draws that the joint
        predictor's ``conditional_simulation`` gives from the dense factor, for data and grids beyond its size -- exceedance
        probabilities, areas above a threshold, ensembles for downstream models.  Returns what the joint method returns: an
        xarray Dataset with ``pred``, ``pred_err`` and ``draws`` (a leading ``draw`` dimension), ``attrs`` holding ``seed``,
        ``ordering``, ``n_levels``, ``n_empty`` and ``n_pinned``; ``postprocess=True`` applies ``_postprocess_predictions``'
        transform to every draw.  Without xarray: ``(DataFrame, draws)``.  ``i=(0, 1)``: the co-simulation of both processes,
        process 1 at ``pcoords1`` (None: the same sites); the result is the pair ``(out_0, out_1)``, each as for one process,
        draw d of both being one jointly consistent pair of maps.  See ``conditional_draws_arrays`` for the arguments and for
        how the ensemble mean relates to ``pred``."""
        frames = [_JointPredictor._sites_frame(pcoords)]
        joint = isinstance(i, (tuple, list))
        if joint:
            frames.append(frames[0] if pcoords1 is None else _JointPredictor._sites_frame(pcoords1))
        draws, pred, err, _, seed = self.conditional_draws_arrays(i, frames[0].values[:, :2], max_dist, n_draws, seed=seed,
                                                                  ordering=ordering, noise=noise,
                                                                  pcoords1=None if pcoords1 is None else frames[1].values[:, :2])
        attrs = {k: self.sim_info[k] for k in ("seed", "ordering", "n_levels", "n_empty", "n_pinned")}
        if not joint:
            return _JointPredictor._draws_output(self, i, frames[0], draws, pred, err, attrs, postprocess)
        m0 = len(frames[0])
        cut = [slice(0, m0), slice(m0, None)]
        return tuple(_JointPredictor._draws_output(self, q, frames[q], draws[:, cut[q]], pred[cut[q]], err[cut[q]], attrs, postprocess)
                     for q in range(2))

    def cross_validation(self, i: int, max_dist: float = 1e3, partitions: int = None,
                         postprocess: bool = True, folds=None, also_withhold=None, buffer=None, seed: int = 0) -> pd.DataFrame:
        """Leave-one-out at every data location of process ``i`` (src/point_prediction.py:303-346):
        one local prediction per location with the co-located datum withheld.

        ``folds`` / ``also_withhold`` / ``buffer`` (not in the reference): leave-GROUP-out and buffer cross-validation, one
        native call (include/cokrige.h: ck_cv_local_folds) under this predictor's ``max_neighbours``, ``trend`` and
        ``measurement_error``.  ``folds`` and ``also_withhold`` are the joint method's: an array of n_i labels (any hashable
        values; None / NaN / -1 = never withheld) or an int K (a random K-fold drawn from ``seed``), and n_other labels of the
        same label set for the other process's data that leave together with a fold (the co-located partner, the same track).
        A fold may be of any size.  ``buffer``: a radius in the units of ``max_dist`` (both processes) or a pair, an entry of None
        turning that process off: the sites of that process within the radius of the predicted datum are withheld as well.
        ``buffer`` alone predicts every datum and needs a radius for process ``i``.

        The frame is the joint method's, with a ``fold`` column, without the rows of never-withheld data.  ``cv_folds_`` holds one
        row per fold: label, n_withheld (both processes), n_scored, me, rmse, msdr (mean of e^2 / v) and nlpd_marginal =
        1/2 (n log 2 pi + sum log v + sum e^2 / v) with v = pred_err^2 + the datum's own measurement-error variance -- the SUM OF
        MARGINAL densities, not the joint density of the fold that the joint predictor reports as ``nlpd`` (different data have
        different neighbourhoods, which define no joint law).  ``cv_scores_`` holds the same over all predicted data."""
        if folds is not None or also_withhold is not None or buffer is not None:
            return self._cv_local(i, max_dist, postprocess, folds, also_withhold, buffer, seed)
        self.cv = True
        names = ["lat", "lon"] if postprocess else ["d1", "d2"]
        f = self.mf.fields[i]
        data = pd.DataFrame(np.hstack((f.coords_main, np.atleast_2d(f.values_main).T)), columns=names + ["data"])
        out = self.__call__(i, data[names], max_dist=max_dist, partitions=partitions, postprocess=postprocess)
        df = out.to_dataframe().reset_index() if hasattr(out, "to_dataframe") else out.reset_index()
        df = df.dropna(subset=["pred"]).merge(data, on=names, how="outer")
        df["residual"] = df["data"] - df["pred"]
        return df[names + ["data", "pred", "residual", "pred_err"]]

    @staticmethod
    def _cv_scores(n, se, se2, sr, sl):
        """me, rmse, msdr, nlpd_marginal from the five sums of ck_cv_local_folds (NaN where nothing was scored)"""
        n = np.asarray(n, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return se / n, np.sqrt(se2 / n), sr / n, np.where(n > 0, 0.5 * (n * np.log(2.0 * np.pi) + sl + sr), np.nan)

    def _cv_local(self, i, max_dist, postprocess, folds, also_withhold, buffer, seed):
        """The ``folds=`` / ``buffer=`` form of ``cross_validation``: everything is validated on the host before any device work."""
        if self.devices is not None and len(self.devices) > 1:
            raise ValueError(f"cross_validation(folds=... / buffer=...) runs on a single device; this predictor has devices={self.devices}")
        if isinstance(i, bool) or not (isinstance(i, (int, np.integer)) and 0 <= int(i) < self.n_procs):
            raise ValueError(f"process index {i!r} out of range for {self.n_procs} processes")
        if isinstance(max_dist, bool) or not np.isfinite(max_dist) or max_dist < 0:
            raise ValueError(f"max_dist must be finite and >= 0, got {max_dist!r}")
        b2 = None
        if buffer is not None:
            b = [buffer] * 2 if np.isscalar(buffer) else list(buffer)
            if len(b) != max(self.n_procs, 1) and len(b) != 2:
                raise ValueError(f"buffer is a number or one entry per process ({self.n_procs}), got {len(b)} entries")
            b = (b + [None, None])[:2]
            for x in b:
                if x is not None and (isinstance(x, (bool, np.bool_)) or not np.isfinite(x) or x < 0):
                    raise ValueError(f"a buffer radius must be None (off) or finite and >= 0, got {x!r}")
            b2 = [None if x is None else float(x) for x in b]
        f = self.mf.fields[i]
        n_i = len(np.asarray(f.values_main))
        n_o = len(np.asarray(self.mf.fields[1 - i].values_main)) if self.n_procs == 2 else None
        if folds is None and also_withhold is None:
            if b2 is None or b2[i] is None:
                raise ValueError(f"buffer alone predicts every datum of process {i} and needs a radius for that process (0 withholds "
                                 "the co-located data), or every datum would predict itself")
            codes, codes_o, labels = None, None, []
        else:
            codes, codes_o, labels = fold_codes(folds, also_withhold, n_i, n_o, seed, fold_max=None)
        names = ["lat", "lon"] if postprocess else ["d1", "d2"]
        data = pd.DataFrame(np.hstack((f.coords_main, np.atleast_2d(f.values_main).T)), columns=names + ["data"])
        h = self._capped_handle()
        F0 = None
        if self.trend is not None:
            coords = [np.asarray(self.mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)]
            design = TrendDesign(self.trend, coords)
            for k in range(self.n_procs):
                h.set_trend(k, design.data(k, coords[k]))
            F0 = design(i, coords[i])
        pred, err, info = h.cv_local_folds(i, codes, codes_o, n_folds=len(labels), buffer=b2, f0=F0, max_dist=max_dist,
                                           want_beta=self.trend is not None)
        self.trend_coef = info.pop("beta", None)
        self.timings = h.cv_local_timings()
        stats, score = info.pop("fold_stats"), info.pop("score5")
        info["n_capped"] = int(h.timings()["local_n_capped"]) if self.max_neighbours is not None else 0
        self.info = info
        if info["n_empty"]:
            warnings.warn(f"No data within maximum distance {max_dist} at {info['n_empty']} location(s).")
        if info["n_not_pd"]:
            warnings.warn(f"Local covariance matrix not positive definte at {info['n_not_pd']} location(s);"
                          " returning NaN.")
        if info.get("n_rank_def"):
            warnings.warn(f"Trend not estimable from the data within maximum distance {max_dist} at {info['n_rank_def']}"
                          " location(s); returning NaN. Use a larger max_dist or a smaller trend.")
        me, rmse, msdr, nlpd = self._cv_scores(stats[:, 1], stats[:, 2], stats[:, 3], stats[:, 4], stats[:, 5])
        self.cv_folds_ = pd.DataFrame({"label": pd.Series(labels, dtype=object), "n_withheld": stats[:, 0].astype(int),
                                       "n_scored": stats[:, 1].astype(int), "me": me, "rmse": rmse, "msdr": msdr, "nlpd_marginal": nlpd})
        t = self._cv_scores(*score)
        self.cv_scores_ = dict(n_scored=int(score[0]), me=float(t[0]), rmse=float(t[1]), msdr=float(t[2]), nlpd_marginal=float(t[3]))
        if codes is None:
            data["fold"] = pd.Series([None] * n_i, dtype=object)
            return _JointPredictor._cv_frame(self, i, postprocess, data, names, pred, err, fold=True)
        data["fold"] = pd.Series([labels[c] if c >= 0 else None for c in codes], dtype=object)
        if postprocess:
            out = _JointPredictor._cv_frame(self, i, True, data, names, pred, err, fold=True)
            return out[out["fold"].notna()].reset_index(drop=True)
        keep = codes >= 0
        data = data[keep].reset_index(drop=True)
        return _JointPredictor._cv_frame(self, i, False, data, names, pred[keep], err[keep], fold=True)
