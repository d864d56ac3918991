"""Host-side mirror of the covariance part of the reference's ``model`` module
(src/model.py): parameter containers and ``MultivariateMatern`` with the same
attribute and method names the notebooks use.  The numbers come from the HIP
library (``ck_cov_lags``): distance -> Matern auto/cross-covariance with a
device K_nu; nothing is evaluated in numpy/scipy here.

``fit`` (composite weighted least squares, src/model.py:277-317) keeps
the reference's optimiser call -- scipy L-BFGS-B with its finite-difference gradient -- and
evaluates the model variograms of every cost-function call in ONE device launch
(``ck_model_variogram``).

``log_likelihood`` / ``fit_likelihood`` (not in the reference) evaluate and maximise the Gaussian log-likelihood of the
data the joint predictor uses, with its analytic gradient (``ck_loglik``): the factor, the unit-row sweep and the gradient
contraction run on the device.
"""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd
from numpy.linalg import LinAlgError
from scipy.optimize import minimize

from . import native

# fit_likelihood(vecchia=...): the step of the central differences in the [0, 1] coordinates (DESIGN 5d-3 has the table it was
# chosen from: at N = 400 the difference gradient is within 6e-8 of the analytic one, relative to its largest entry)
FD_STEP_DEFAULT = 1e-5
# ... and the optimiser's stopping rules there: differences carry the rounding of two values, so the tolerances of the analytic
# gradient (ftol 1e-13, gtol 1e-9) are below what they can resolve (with a step of 1e-4 the line search gave up under them)
VECCHIA_FIT_OPTIONS = {"maxiter": 1000, "ftol": 1e-10, "gtol": 1e-5}


class _Param:
    """An n_procs x n_procs parameter array, NaN where the parameter does not exist
    (cf. MarginalParam / CrossParam / RhoParam, src/model.py:16-106)."""

    def __init__(self, name, default, bounds, n_procs, where):
        self.name, self.default, self.bounds, self.n_procs = name, default, bounds, n_procs
        self._where = where  # "diag" | "triu" | "striu"
        self.values = np.full((n_procs, n_procs), np.nan)
        self.reset_values()

    def _index(self):
        if self._where == "diag":
            return np.diag_indices(self.n_procs)
        return np.triu_indices(self.n_procs, k=0 if self._where == "triu" else 1)

    def get_names(self):
        r, c = self._index()
        return [f"{self.name}_{i + 1}{j + 1}" for i, j in zip(r, c)]

    def get_values(self):
        return self.values[self._index()]

    def set_values(self, x):
        self.values[self._index()] = x
        return self

    def reset_values(self):
        self.values[self._index()] = self.default
        return self

    def count_params(self):
        return len(self._index()[0])

    def to_dataframe(self):
        return pd.DataFrame({"name": self.get_names(), "value": self.get_values(),
                             "bounds": [self.bounds] * self.count_params()})


class MaternParams:
    """sigma, nu, len_scale, nugget, rho with the reference's defaults, bounds and flat
    order sigma_11 sigma_22 nu_11 nu_12 nu_22 len_11 len_12 len_22 nugget_11 nugget_22 rho_12
    (src/model.py:109-169)."""

    def __init__(self, n_procs: int = 2) -> None:
        self.n_procs = n_procs
        self.sigma = _Param("sigma", 1.0, (0.4, 3.5), n_procs, "diag")
        self.nu = _Param("nu", 1.5, (0.2, 3.5), n_procs, "triu")
        self.len_scale = _Param("len_scale", 5e2, (1e2, 2e3), n_procs, "triu")
        self.nugget = _Param("nugget", 0.0, (0.0, 0.2), n_procs, "diag")
        self.rho = _Param("rho", np.nan if n_procs == 1 else 0.0, (-1.0, 1.0), n_procs, "striu")
        self._params = [self.sigma, self.nu, self.len_scale, self.nugget, self.rho]
        self.n_params = sum(p.count_params() for p in self._params)

    def to_dataframe(self):
        return pd.concat([p.to_dataframe() for p in self._params], ignore_index=True)

    def get_names(self):
        return self.to_dataframe()["name"].values

    def get_values(self):
        return self.to_dataframe()["value"].values

    def get_bounds(self):
        return self.to_dataframe()["bounds"].values

    def set_values(self, x):
        x = np.asarray(x, dtype=float)
        if len(x) != self.n_params:
            raise ValueError("Incorrect number of parameters in input array.")
        at = 0
        for p in self._params:
            k = p.count_params()
            p.set_values(x[at:at + k])
            at += k
        return self

    def reset_values(self):
        for p in self._params:
            p.reset_values()
        return self

    def set_bounds(self, **kwargs):
        for name, bounds in kwargs.items():
            if name not in ("sigma", "nu", "len_scale", "nugget", "rho"):
                raise AttributeError(f"`{name}` is not a valid parameter.")
            getattr(self, name).bounds = bounds
        return self


def model_arrays(mod):
    """(n_procs, sigma, nu3, len3, nugget, rho12) from any object with the reference's
    ``mod.params.<name>.values`` layout (ours or the reference's own MultivariateMatern)."""
    p = mod.params
    n = int(mod.n_procs)
    sig = np.diag(np.asarray(p.sigma.values, dtype=float)).copy()
    nug = np.diag(np.asarray(p.nugget.values, dtype=float)).copy()
    nu = np.asarray(p.nu.values, dtype=float)
    ls = np.asarray(p.len_scale.values, dtype=float)
    if n == 1:
        return 1, sig, np.array([nu[0, 0]] * 3), np.array([ls[0, 0]] * 3), nug, 0.0
    if n != 2:
        raise ValueError("the HIP path supports n_procs = 1 or 2")
    rho = float(np.asarray(p.rho.values, dtype=float)[0, 1])
    return 2, sig, np.array([nu[0, 0], nu[0, 1], nu[1, 1]]), np.array([ls[0, 0], ls[0, 1], ls[1, 1]]), nug, rho


def configure_handle(h: "native.Handle", mod):
    n, sig, nu, ls, nug, rho = model_arrays(mod)
    h.set_model(n, sig, nu, ls, nug, rho)


class MultivariateMatern:
    """Multivariate Matern covariance model (Gneiting et al., 2010) -- same public
    surface as src/model.py:172-222 for the covariance functions."""

    def __init__(self, n_procs: int = 2, params: MaternParams = None, device: int = 0) -> None:
        self.n_procs = n_procs
        self.params = MaternParams(n_procs=n_procs) if params is None else params
        self.fit_result = None
        self._device = device
        self._h = None
        self._lik = None   # (key, handle): the data-loaded handle of log_likelihood

    def _handle(self):
        if self._h is None:
            self._h = native.Handle(self._device)
        configure_handle(self._h, self)   # parameters may have been edited in place
        return self._h

    def _eval(self, i, j, h, use_nugget):
        h = np.atleast_1d(np.asarray(h, dtype=np.float64))
        return self._handle().cov_lags(i, j, h, use_nugget=use_nugget)

    def covariance(self, i: int, h, use_nugget: bool = True) -> np.ndarray:
        """sigma_i^2 rho_ii(h) + nugget_i [h == 0]   (src/model.py:193-197)."""
        return self._eval(i, i, h, use_nugget)

    def cross_covariance(self, i: int, j: int, h) -> np.ndarray:
        """rho_ij prod(sigma) rho^Matern_ij(h)   (src/model.py:199-207)."""
        if i > j:
            i, j = j, i
        return self._eval(i, j, h, False)

    def correlation(self, i: int, j: int, h) -> np.ndarray:
        """Matern correlation with (nu_ij, len_scale_ij) -- src/model.py:188-191; it does not depend on sigma or
        rho, so it is evaluated with unit amplitudes (rho_12 = 0 is a valid model and must not divide by zero)."""
        if i > j:
            i, j = j, i
        n, sig, nu, ls, nug, rho = model_arrays(self)
        if self._h is None:
            self._h = native.Handle(self._device)
        self._h.set_model(n, np.ones_like(sig), nu, ls, np.zeros_like(nug), 1.0)
        h = np.atleast_1d(np.asarray(h, dtype=np.float64))
        return self._h.cov_lags(i, j, h, use_nugget=False)   # the next _handle() call restores the model's amplitudes

    def semivariance(self, i: int, h) -> np.ndarray:
        """src/model.py:209-213."""
        s2 = self.params.sigma.values[i, i] ** 2
        return s2 - self._eval(i, i, h, False) + self.params.nugget.values[i, i]

    def cross_semivariance(self, i: int, j: int, h) -> np.ndarray:
        """src/model.py:215-222."""
        sill = 0.5 * np.nansum(self.params.sigma.values ** 2 + self.params.nugget.values)
        return sill - self.cross_covariance(i, j, h)

    def get_variogram(self, i: int, j: int, h, kind: str) -> pd.DataFrame:
        """src/model.py:224-237."""
        h = np.asarray(h, dtype=np.float64)
        v = self._handle().model_variogram(i, j, h, kind="covariogram" if kind == "covariogram" else "semivariogram")
        df = pd.DataFrame({"distance": h, "variogram": v, "i": i, "j": j})
        return df.set_index(["i", "j", df.index])

    def variograms(self, h, kind: str = "semivariogram") -> pd.DataFrame:
        """Modelled variograms and cross-variogram(s) at the given lags (src/model.py:239-248)."""
        return pd.concat([self.get_variogram(i, j, h, kind)
                          for i in range(self.n_procs) for j in range(self.n_procs) if i <= j])

    @staticmethod
    def _weighted_least_squares(ydata: np.ndarray, yfit: np.ndarray, bin_counts: np.ndarray) -> float:
        """Cressie (1985) weighted least squares with the reference's handling of fit == 0
        (src/model.py:250-264)."""
        ydata, yfit, bin_counts = (np.asarray(a, dtype=np.float64) for a in (ydata, yfit, bin_counts))
        zero = yfit == 0.0
        wls = np.zeros_like(yfit)
        wls[zero] = bin_counts[zero] * ydata[zero] ** 2
        nz = ~zero
        wls[nz] = bin_counts[nz] * ((ydata[nz] - yfit[nz]) / yfit[nz]) ** 2
        return np.sum(wls)

    def _map_fit(self, df_vario: pd.DataFrame) -> pd.DataFrame:
        """New ``fit`` column: the model semivariogram at ``bin_center`` for every (i, j) group
        (src/model.py:266-275), all groups in one device launch; rows come back grouped by (i, j)
        in sorted order like ``groupby(level=[0, 1]).apply``."""
        df = df_vario.sort_index(level=[0, 1], sort_remaining=False, kind="stable").copy()
        i = df.index.get_level_values(0).values.astype(np.int32)
        j = df.index.get_level_values(1).values.astype(np.int32)
        lo, hi = np.minimum(i, j), np.maximum(i, j)   # cross-semivariance is symmetric (:216-218)
        df["fit"] = self._handle().model_variogram(lo, hi, df["bin_center"].values.astype(np.float64))
        return df

    def _composite_wls(self, p, df_vario: pd.DataFrame) -> float:
        """Composite WLS cost (src/model.py:277-283, 389-391)."""
        self.params.set_values(p)
        df = self._map_fit(df_vario)
        ydata, yfit, counts = df[["bin_mean", "fit", "bin_count"]].T.values.astype(np.float64)
        nz = yfit != 0.0
        return np.sum(counts[nz] * ((ydata[nz] - yfit[nz]) / yfit[nz]) ** 2)

    def fit(self, estimate, guess: MaternParams = None, polish: bool = False):
        """Fit the parameters to the empirical (cross-)semivariograms simultaneously by composite
        weighted least squares -- same flow, optimiser and warning as src/model.py:285-317.
        ``polish`` (not in the reference; off by default, so the default call is the reference's): restart the
        optimiser once from its own answer and keep the better of the two -- L-BFGS-B on finite-difference gradients
        stops early on this cost's flat valley floors (the reference's recorded run: 1618.19, restarted: 1608.19)."""
        if estimate.config.n_procs != self.n_procs:
            raise ValueError("Number of theoretical processes different from empirical processes.")
        if guess is None:
            init_params = self.params.reset_values().get_values()
        else:
            init_params = self.params.get_values()
            self.params.set_bounds(**{p.name: p.bounds for p in guess._params})
        bounds = self.params.get_bounds()
        optim_result = minimize(self._composite_wls, init_params, args=(estimate.df,), method="L-BFGS-B", bounds=bounds)
        if polish:
            again = minimize(self._composite_wls, optim_result.x, args=(estimate.df,), method="L-BFGS-B", bounds=bounds)
            if again.fun <= optim_result.fun:
                optim_result = again
        if optim_result.success == False:   # noqa: E712  (as the reference)
            warnings.warn("ERROR: optimization did not converge.")
        self.params.set_values(optim_result.x)
        self.fit_result = FittedVariogram(self, estimate, optim_result.fun)
        return self


    # -- Gaussian log-likelihood -----------------------------------------------------------------
    def _lik_handle(self, mf, dist_units, fast_dist):
        """A handle with the data of ``mf`` loaded, kept on the model and keyed like Predictor._state_key (metric and
        data arrays; the parameters are set again on every evaluation)."""
        from .fields import metric_of
        if mf.n_procs != self.n_procs:
            raise ValueError("Number of theoretical processes different from empirical processes.")
        metric = metric_of(dist_units, fast_dist)
        cs, vs, key = [], [], [metric]
        for k in range(self.n_procs):
            c = np.ascontiguousarray(np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2])
            v = np.ascontiguousarray(mf.fields[k].values_main, dtype=np.float64).ravel()
            cs.append(c)
            vs.append(v)
            key += [c.shape, hash(c.tobytes()), hash(v.tobytes())]
        key = tuple(key)
        if self._lik is None or self._lik[0] != key:
            if self._lik is not None:
                self._lik[1].close()
                self._lik = None
            h = native.Handle(self._device)
            h.set_metric(metric)
            for k in range(self.n_procs):
                h.set_data(k, cs[k], vs[k])
            self._lik = (key, h)
        h = self._lik[1]
        configure_handle(h, self)
        return h

    def log_likelihood(self, mf, dist_units: str = "km", fast_dist: bool = True, gradient: bool = False, trend=None,
                       measurement_error=None, noise_scale=None, vecchia=None, _ranks=None, _free13=None):
        """Gaussian log-likelihood of the data the joint predictor uses (every field's ``coords_main`` / ``values_main``,
        zero mean as in simple cokriging) under the current parameters:
            l = -1/2 (N log 2 pi + log|Sigma| + z^T Sigma^-1 z),
        Sigma assembled as the predictor assembles it.  ``gradient=True``: (l, dl/dtheta) with the gradient in the flat
        order of ``params.get_names()``.  A Sigma that is not positive definite raises LinAlgError with scipy's text.

        ``trend`` (as ``Predictor(trend=...)``: "constant", "linear" or a callable): the restricted likelihood (REML) for an
        unknown trend X beta, ``ck_loglik_reml``:
            l_R = -1/2 ((N - p) log 2 pi + log|Sigma| + log|X^T Sigma^-1 X| + z^T P z),
        without a log|X^T X| term.

        ``measurement_error`` (as ``Predictor(measurement_error=...)``: True or a list with an array or None per process)
        and ``noise_scale`` (one scale per process, default 1): Sigma carries ``noise_scale[k] * d_a`` on its true diagonal
        (``ck_set_noise``).  With ``gradient=True`` the call then returns (l, dl/dtheta, dl/ds): the derivatives in the
        noise scales, one per process (0 for a process without noise), as a third value; without ``measurement_error``
        the result has the shape it always had.

        ``vecchia`` (a ``vecchia.Vecchia``): Vecchia's approximation instead (``ck_loglik_vecchia``) -- every datum
        conditioned on the earlier data of its ordering within ``vecchia.max_dist`` and under its caps; no Sigma is
        assembled, so it reaches data sizes the exact form cannot.  ``measurement_error`` / ``noise_scale`` are honoured;
        ``trend`` is refused (no REML form), and so is ``gradient=True`` unless the configuration says
        ``Vecchia(..., gradient="analytic")``: then the call returns (l, dl/dtheta) -- with ``measurement_error``
        (l, dl/dtheta, dl/ds) -- in the shapes of the dense call, from ``ck_loglik_vecchia_grad`` (conditioning sets of at most
        64 data; a larger one raises the native error).  A datum whose local system is not positive definite raises
        LinAlgError naming it.  A trend belongs to the configuration: with ``Vecchia(trend=...)`` the value is the profile
        likelihood l_P, beta estimated by GLS inside it (``ck_loglik_vecchia_trend``), or with ``trend_likelihood="reml"`` the
        restricted l_R; ``gradient=True`` then needs the profile form (``ck_loglik_vecchia_trend_grad``) and is refused for
        "reml", which the fit differences numerically."""
        if vecchia is not None:
            if trend is not None:
                raise ValueError("log_likelihood(vecchia=...) has no restricted (REML) form: trend must be None -- the trend of "
                                 "a Vecchia likelihood is part of its configuration, Vecchia(trend=..., trend_likelihood=...)")
            if gradient and getattr(vecchia, "gradient", "numeric") != "analytic":
                raise NotImplementedError("the Vecchia likelihood has no analytic gradient yet: call it with gradient=False "
                                          "(fit_likelihood(vecchia=...) differentiates it numerically)")
            if gradient and getattr(vecchia, "reml", False):
                raise NotImplementedError("the restricted (REML) Vecchia likelihood has no analytic gradient: call it with "
                                          "gradient=False (fit_likelihood(vecchia=...) takes the numeric route and differences "
                                          "the value), or use Vecchia(trend_likelihood=\"profile\")")
            if gradient:
                out3, g13, info, var = self._vecchia_grad_eval(mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale,
                                                               _ranks, _free13)
            else:
                out3, info, _ = self._vecchia_eval(mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale, _ranks)
            if info != 0:
                raise LinAlgError(f"the local system of datum {info - 1} (stacked order) is not positive definite, or its "
                                  "conditional variance is not positive")
            if not gradient:
                return out3[0]
            g = g13[:len(self.params.get_names())].copy()
            return (out3[0], g, g13[11:11 + self.n_procs].copy()) if var is not None else (out3[0], g)
        h, var = self._lik_assembled(mf, dist_units, fast_dist, trend, measurement_error, noise_scale)
        info, out3, g = h.loglik_reml(gradient) if trend is not None else h.loglik(gradient)
        if info != 0:
            raise LinAlgError(f"{info}-th leading minor of the array is not positive definite")
        if gradient and var is not None:
            return out3[0], g, h.loglik_noise_grad()[:self.n_procs]
        return (out3[0], g) if gradient else out3[0]

    def _vecchia_eval(self, mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale, ranks=None, terms=False):
        """(out3, info, stats) of ``ck_loglik_vecchia`` on the likelihood's handle -- noise set, no trend, nothing assembled."""
        from .vecchia import Vecchia
        if not isinstance(vecchia, Vecchia):
            raise ValueError(f"vecchia must be a vecchia.Vecchia, got {type(vecchia).__name__}")
        caps = vecchia.caps(self.n_procs)
        h, _ = self._lik_assembled(mf, dist_units, fast_dist, vecchia.trend, measurement_error, noise_scale, assemble=False)
        if ranks is None:
            ranks = vecchia.ranks([np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)])
        h.set_local_neighbours(*caps)
        if vecchia.trend is not None:   # (out5, info, stats): beta and beta_cov ride in stats
            out5, beta, cov, info, st = self._vecchia_native(lambda: h.loglik_vecchia_trend(ranks, vecchia.max_dist,
                                                                                           reml=vecchia.reml, terms=terms),
                                                             "trend form")
            st.update(beta=beta, beta_cov=cov)
            return out5, info, st
        return h.loglik_vecchia(ranks, vecchia.max_dist, terms=terms)

    @staticmethod
    def _vecchia_native(call, what):
        """``call()``; a conditioning set beyond the LDS class is reported with the way out"""
        try:
            return call()
        except native.NativeError as exc:
            if "conditioning set of more than" in str(exc):
                raise native.NativeError(f"{exc}.  The {what} of the Vecchia likelihood is for sets of at most 64 data: use "
                                         "smaller max_neighbours") from None
            raise

    def _vecchia_grad_eval(self, mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale, ranks=None, free13=None):
        """(out3, grad13, info, variances) of ``ck_loglik_vecchia_grad`` on the likelihood's handle, set up as ``_vecchia_eval``."""
        from .vecchia import Vecchia
        if not isinstance(vecchia, Vecchia):
            raise ValueError(f"vecchia must be a vecchia.Vecchia, got {type(vecchia).__name__}")
        caps = vecchia.caps(self.n_procs)
        h, var = self._lik_assembled(mf, dist_units, fast_dist, vecchia.trend, measurement_error, noise_scale, assemble=False)
        if ranks is None:
            ranks = vecchia.ranks([np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)])
        h.set_local_neighbours(*caps)
        if vecchia.trend is not None:   # the profile form: the gradient at beta-hat
            out5, _, _, g13, info, _ = self._vecchia_native(
                lambda: h.loglik_vecchia_trend_grad(ranks, vecchia.max_dist, free=free13), "trend form")
            return out5, g13, info, var
        try:
            out3, g13, info, _ = h.loglik_vecchia_grad(ranks, vecchia.max_dist, free=free13)
        except native.NativeError as exc:
            if "conditioning set of more than" in str(exc):
                raise native.NativeError(f"{exc}.  The analytic gradient is for sets of at most 64 data: use "
                                         "Vecchia(..., gradient=\"numeric\") or smaller max_neighbours") from None
            raise
        return out3, g13, info, var

    def vecchia_terms(self, mf, vecchia, dist_units: str = "km", fast_dist: bool = True, measurement_error=None,
                      noise_scale=None):
        """One row per datum of the Vecchia likelihood (``vecchia.vecchia_terms``): process, index, mean, variance, n0, n1."""
        from .vecchia import vecchia_terms
        return vecchia_terms(self, mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale)

    def _lik_assembled(self, mf, dist_units, fast_dist, trend, measurement_error, noise_scale, assemble=True):
        """(handle, variances): the likelihood's handle with the current parameters, the noise and the trend set and Sigma
        assembled -- what ``log_likelihood`` and ``information`` evaluate.  ``assemble=False``: everything but Sigma."""
        from .noise import apply_noise, resolve_measurement_error
        from .trend import TrendDesign, check_trend
        check_trend(trend)
        var, scales = resolve_measurement_error(measurement_error, noise_scale, mf.fields)
        h = self._lik_handle(mf, dist_units, fast_dist)
        if var is None:
            for k in range(self.n_procs):
                h.set_noise(k, None)
        else:
            apply_noise(h, [d if d is not None else None for d in var], scales)
            for k in range(self.n_procs):
                if var[k] is None:
                    h.set_noise(k, None)
        if trend is not None:
            cs = [np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)]
            design = TrendDesign(trend, cs)
            F = [design.data(k, cs[k]) for k in range(self.n_procs)]
            for k in range(self.n_procs):
                h.set_trend(k, F[k])
        else:
            for k in range(self.n_procs):
                h.set_trend(k, None)
        if assemble:
            h.assemble_joint()
        return h, var

    def information(self, mf, dist_units: str = "km", fast_dist: bool = True, trend=None, measurement_error=None,
                    noise_scale=None, fixed=None, _at_bound=None, vecchia=None, _ranks=None):
        """Expected (Fisher) information of the likelihood at the current parameters and what follows from it
        (``ParameterInformation``): I_jk = 1/2 tr(Sigma^-1 D_j Sigma^-1 D_k) with D_k = dSigma/dtheta_k, computed on the
        device (``ck_loglik_fisher``); with ``trend`` the information of the restricted likelihood.  The arguments are those
        of ``log_likelihood``.  The noise scales of the processes that have ``measurement_error`` are parameters too
        (``noise_scale_0`` / ``noise_scale_1``).  ``fixed``: names (or flat indices of the model parameters) conditioned on:
        they are left out, and the standard errors are those of the others given them.

        ``vecchia`` (a ``vecchia.Vecchia``): the expected information of the Vecchia likelihood instead
        (``ck_loglik_vecchia_fisher``), for data whose Sigma does not fit: I^V = sum_t [I(S_t) - I(c_t)] over the conditioning
        sets c_t and S_t = c_t + {t} of ``log_likelihood(vecchia=...)`` -- the expected negative Hessian of the Vecchia
        objective under the exact model, what GpGp reports with its fits; not a Godambe sandwich.  It equals the dense
        information when every earlier datum is in every set.  Conditioning sets of at most 64 data (a larger one raises the
        native error); ``trend`` is refused (no REML form).  The call works whatever ``vecchia.information`` says.  With
        ``Vecchia(trend=...)`` in its profile form the same matrix is returned -- under the Gaussian model it does not depend on
        the mean and the theta and beta blocks are orthogonal, so it is computed without the trend -- together with
        ``beta_cov`` = Cov(beta-hat) of the trend call; ``trend_likelihood="reml"`` raises NotImplementedError."""
        if vecchia is not None:
            from .vecchia import Vecchia
            if trend is not None:
                raise ValueError("information(vecchia=...) has no restricted (REML) form: trend must be None -- see "
                                 "Vecchia(trend=...)")
            if not isinstance(vecchia, Vecchia):
                raise ValueError(f"vecchia must be a vecchia.Vecchia, got {type(vecchia).__name__}")
            if vecchia.reml:
                raise NotImplementedError("the restricted (REML) Vecchia likelihood has no expected information: use "
                                          "Vecchia(trend_likelihood=\"profile\")")
            caps = vecchia.caps(self.n_procs)
        h, var = self._lik_assembled(mf, dist_units, fast_dist, trend, measurement_error, noise_scale, assemble=vecchia is None)
        names13 = information_slot_names(self.n_procs)
        model_names = list(self.params.get_names())
        live = np.zeros(13, dtype=bool)
        live[:len(model_names)] = True
        for k in range(self.n_procs):
            live[11 + k] = var is not None and var[k] is not None
        for f in ([] if fixed is None else ([fixed] if isinstance(fixed, (str, int, np.integer)) else fixed)):
            if isinstance(f, str):
                if f not in names13 or f == "":
                    raise ValueError(f"`{f}` is not a parameter name ({[n for n in names13 if n]})")
                live[names13.index(f)] = False
            else:
                if not 0 <= int(f) < len(model_names):
                    raise ValueError(f"parameter index {f} out of range")
                live[int(f)] = False
        bound = np.zeros(13, dtype=bool)
        for f in ([] if _at_bound is None else _at_bound):
            bound[names13.index(f)] = live[names13.index(f)]
        if vecchia is not None:
            ranks = _ranks
            if ranks is None:
                ranks = vecchia.ranks([np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2] for k in range(self.n_procs)])
            h.set_local_neighbours(*caps)
            try:
                fisher, info, _ = h.loglik_vecchia_fisher(ranks, vecchia.max_dist, free=live & ~bound)
            except native.NativeError as exc:
                if "conditioning set of more than" in str(exc):
                    raise native.NativeError(f"{exc}.  The information of the Vecchia likelihood is for sets of at most 64 "
                                             "data: use smaller max_neighbours") from None
                raise
            if info != 0:
                raise LinAlgError(f"the local system of datum {info - 1} (stacked order) is not positive definite, or its "
                                  "conditional variance is not positive")
        else:
            info, fisher = h.fisher(reml=trend is not None, free=live & ~bound)
            if info != 0:
                raise LinAlgError(f"{info}-th leading minor of the array is not positive definite")
        est = np.full(13, np.nan)
        est[:len(model_names)] = self.params.get_values().astype(float)
        if var is not None:
            from .noise import resolve_measurement_error
            scales = resolve_measurement_error(measurement_error, noise_scale, mf.fields)[1]
            for k in range(self.n_procs):
                est[11 + k] = scales[k]
        inf = summarize_information(fisher, self.n_procs, live, est, at_bound=bound)
        if vecchia is not None and vecchia.trend is not None:
            # the profile form: under the Gaussian model I^V does not depend on the mean and the theta and beta blocks are
            # orthogonal, so the matrix above (computed without the trend) stands; Cov(beta-hat) comes from the trend call
            st = self._vecchia_eval(mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale, ranks)[2]
            inf.beta_cov = st["beta_cov"]
        return inf

    def fit_likelihood(self, mf, guess: MaternParams = None, fixed=None, dist_units: str = "km", fast_dist: bool = True,
                       trend=None, measurement_error=None, noise_scale=None, fit_noise_scale: bool = False,
                       std_errors: bool = False, vecchia=None, fd_step: float = FD_STEP_DEFAULT):
        """Maximum-likelihood fit: L-BFGS-B on -l with the analytic gradient, within ``params.get_bounds()``.
        ``guess`` as in ``fit``: None starts from the default parameters, else from the current ones with the bounds of
        ``guess``.  ``fixed``: parameter names or flat indices held at their starting values.
        The optimiser works on every free parameter mapped linearly onto [0, 1] over its bounds (the parameters differ by
        three orders of magnitude in scale).  A step into a region where Sigma is not positive definite does not end the
        fit: the cost there is the largest -l met so far plus 1e6 (1 + |that value|), finite and far above every positive
        definite point, with the gradient of the last positive definite point, so that the line search backtracks; such
        evaluations are counted in ``fit_result.n_not_pd``.  Sets the parameters and ``self.fit_result``
        (FittedLikelihood).  ``trend``: maximise the restricted likelihood (REML) for that trend instead
        (``log_likelihood(trend=...)``); ``fit_result.method`` is then "REML".

        ``measurement_error`` / ``noise_scale``: as ``log_likelihood``.  ``fit_noise_scale=True``: the scales of the processes
        that have noise are estimated too (the reported retrieval uncertainties are known to be too small by a factor):
        they join the optimiser's vector as log s over [log 1e-3, log 1e3], mapped onto [0, 1] like the other parameters,
        starting at ``noise_scale``.  ``fit_result.noise_scale`` holds the scales used or found, and the AIC counts the
        estimated ones.

        ``std_errors=True``: ``fit_result.information`` is the ``ParameterInformation`` at the optimum (``information``: ML
        or REML as fitted, the noise scales included when they were fitted), with the shortcuts ``fit_result.std_error`` and
        ``fit_result.conf_int()``.  Parameters held by ``fixed`` are conditioned on; so is a parameter that ends within 1e-8
        of its bound width from a bound: it is listed in ``fit_result.at_bound`` with a NaN standard error, and one warning
        says so.  With the default False these attributes are None.

        ``vecchia`` (a ``vecchia.Vecchia``): maximise the Vecchia likelihood instead (``log_likelihood(vecchia=...)``), for
        data whose Sigma does not fit; bounds, ``fixed``, the [0, 1] mapping, the noise scales and the not-positive-definite
        penalty are as above.  By default the gradient comes from central differences of the value with the
        step ``fd_step`` in the mapped coordinates, one-sided where a step would leave [0, 1] (2 k evaluations per gradient
        for k free parameters).  With ``Vecchia(..., gradient="analytic")`` value and gradient come from one native call per
        evaluation (``ck_loglik_vecchia_grad``, the slots held fixed masked out), under the dense path's optimiser options;
        ``fd_step`` is then validated and otherwise unused, and a conditioning set beyond 64 data raises the native error.
        The ordering's ranks are computed once per fit.  ``fit_result.method`` is "Vecchia-ML"; ``trend`` is refused.
        ``std_errors=True`` is refused (the Fisher information is not configured) unless the configuration says
        ``Vecchia(..., information="expected")``: then ``fit_result.information``, ``.std_error``, ``.conf_int()`` and
        ``.at_bound`` are filled as after a dense fit, from ``information(vecchia=...)`` at the optimum on the fit's ranks --
        the expected information of the Vecchia objective under the exact model, for conditioning sets of at most 64 data.
        ``Vecchia(trend=...)``: beta is estimated by GLS at every evaluation (``ck_loglik_vecchia_trend``); the profile form with
        the analytic gradient makes one native call per evaluation, ``trend_likelihood="reml"`` is differenced numerically.
        ``fit_result.method`` is "Vecchia-ML" or "Vecchia-REML" and ``fit_result.beta`` / ``.beta_cov`` hold the trend at the
        optimum (None for every other fit); ``std_errors=True`` works with the profile form (``information``) and is refused
        for "reml"."""
        from .noise import resolve_measurement_error
        from .trend import check_trend
        check_trend(trend)
        if vecchia is not None:
            if trend is not None:
                raise ValueError("fit_likelihood(vecchia=...) has no restricted (REML) form: trend must be None -- see "
                                 "Vecchia(trend=..., trend_likelihood=...)")
            if std_errors and getattr(vecchia, "reml", False):
                raise NotImplementedError("std_errors=True needs the Fisher information, which the restricted (REML) Vecchia "
                                          "likelihood does not have: use Vecchia(trend_likelihood=\"profile\")")
            if std_errors and getattr(vecchia, "information", "none") != "expected":
                raise NotImplementedError("std_errors=True needs the Fisher information: configure the expected information of "
                                          "the Vecchia likelihood with Vecchia(..., information=\"expected\"), or fit with "
                                          "vecchia and call information() afterwards")
            if not (isinstance(fd_step, (float, np.floating)) and 0.0 < fd_step < 0.5):
                raise ValueError(f"fd_step must be a float in (0, 0.5), got {fd_step!r}")
            v_ranks = vecchia.ranks([np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2]
                                     for k in range(self.n_procs)])
        var, scales = resolve_measurement_error(measurement_error, noise_scale, mf.fields)
        if fit_noise_scale and var is None:
            raise ValueError("fit_noise_scale=True needs measurement_error")
        s_free = [k for k in range(self.n_procs) if var is not None and var[k] is not None] if fit_noise_scale else []
        s_lo, s_width = np.log(1e-3), np.log(1e3) - np.log(1e-3)
        s_cur = None if scales is None else np.array(scales, dtype=float)
        if guess is None:
            init = self.params.reset_values().get_values().astype(float)
        else:
            init = self.params.get_values().astype(float)
            self.params.set_bounds(**{p.name: p.bounds for p in guess._params})
        names = list(self.params.get_names())
        bounds = np.array([tuple(b) for b in self.params.get_bounds()], dtype=float)
        hold = set()
        for f in ([] if fixed is None else ([fixed] if isinstance(fixed, (str, int, np.integer)) else fixed)):
            if isinstance(f, str):
                if f not in names:
                    raise ValueError(f"`{f}` is not a parameter name ({names})")
                hold.add(names.index(f))
            else:
                if not 0 <= int(f) < len(names):
                    raise ValueError(f"parameter index {f} out of range")
                hold.add(int(f))
        free = np.array([k for k in range(len(names)) if k not in hold], dtype=int)
        if free.size == 0 and not s_free:
            raise ValueError("every parameter is fixed")
        lo, width = bounds[free, 0], bounds[free, 1] - bounds[free, 0]
        width = np.where(width > 0, width, 1.0)
        init = init.copy()
        init[free] = np.clip(init[free], bounds[free, 0], bounds[free, 1])
        state = {"n_eval": 0, "n_not_pd": 0, "worst": None, "grad": np.zeros(free.size + len(s_free))}
        nf = free.size

        def theta_of(u):
            th = init.copy()
            th[free] = lo + width * np.asarray(u, dtype=float)[:nf]
            return th

        def scales_of(u):
            if s_cur is None:
                return None
            s = s_cur.copy()
            for j, k in enumerate(s_free):
                s[k] = np.exp(s_lo + s_width * float(np.asarray(u, dtype=float)[nf + j]))
            return tuple(s.tolist())

        def value_v(u):
            self.params.set_values(theta_of(u))
            return self.log_likelihood(mf, dist_units, fast_dist, measurement_error=measurement_error, noise_scale=scales_of(u),
                                       vecchia=vecchia, _ranks=v_ranks)

        def loglik_v(u):
            """(l, dl/dtheta over all parameters, dl/ds per process) by differences in the mapped coordinates"""
            u = np.asarray(u, dtype=float)
            ll = value_v(u)
            gu = np.zeros(u.size)
            for j in range(u.size):
                up, dn = u.copy(), u.copy()
                up[j] = min(u[j] + fd_step, 1.0)
                dn[j] = max(u[j] - fd_step, 0.0)
                f_up = ll if up[j] == u[j] else value_v(up)
                f_dn = ll if dn[j] == u[j] else value_v(dn)
                gu[j] = (f_up - f_dn) / (up[j] - dn[j])
            self.params.set_values(theta_of(u))
            g = np.zeros(len(names))
            g[free] = gu[:nf] / width            # cost() maps back with the same widths
            gs = np.zeros(self.n_procs)
            if s_free:
                sc = np.array(scales_of(u))
                for j, k in enumerate(s_free):
                    gs[k] = gu[nf + j] / (sc[k] * s_width)
            return ll, g, gs

        # (the restricted form of a trend is value-only: it takes the numeric route whatever the configuration says)
        analytic_v = (vecchia is not None and getattr(vecchia, "gradient", "numeric") == "analytic"
                      and not getattr(vecchia, "reml", False))
        free13 = np.zeros(13, dtype=bool)   # the live slots of ck_loglik_vecchia_grad: the free parameters, the fitted scales
        free13[free] = True
        for k in s_free:
            free13[11 + k] = True

        def loglik(u):
            if analytic_v:   # value and gradient from one native call; the slots held fixed are not computed (exact zeros)
                out = self.log_likelihood(mf, dist_units, fast_dist, gradient=True, measurement_error=measurement_error,
                                          noise_scale=scales_of(u), vecchia=vecchia, _ranks=v_ranks, _free13=free13)
                return out if len(out) == 3 else (out[0], out[1], np.zeros(self.n_procs))
            if vecchia is not None:
                return loglik_v(u)
            out = self.log_likelihood(mf, dist_units, fast_dist, gradient=True, trend=trend, measurement_error=measurement_error,
                                      noise_scale=scales_of(u))
            return out if len(out) == 3 else (out[0], out[1], np.zeros(self.n_procs))

        def cost(u):
            state["n_eval"] += 1
            self.params.set_values(theta_of(u))
            try:
                ll, g, gs = loglik(u)
                if s_free:   # dl/du = dl/ds * ds/du, s = exp(s_lo + s_width u)
                    sc = np.array(scales_of(u))
                    g = np.concatenate([np.asarray(g, dtype=float)[free] * width,
                                        [gs[k] * sc[k] * s_width for k in s_free]])
                else:
                    g = np.asarray(g, dtype=float)[free] * width
            except LinAlgError:
                ll = None
            if ll is None or not np.isfinite(ll) or not np.all(np.isfinite(g)):
                state["n_not_pd"] += 1
                worst = state["worst"]
                if worst is None:
                    raise LinAlgError("the starting point of fit_likelihood is not positive definite")
                return worst + 1e6 * (1.0 + abs(worst)), state["grad"].copy()
            f = -ll
            gu = -g
            state["worst"] = f if state["worst"] is None else max(state["worst"], f)
            state["grad"] = gu
            return f, gu

        u0 = (init[free] - lo) / width
        if s_free:
            u0 = np.concatenate([u0, [(np.log(np.clip(s_cur[k], 1e-3, 1e3)) - s_lo) / s_width for k in s_free]])
        res = minimize(cost, u0, jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * len(u0),
                       options=dict(VECCHIA_FIT_OPTIONS) if vecchia is not None and not analytic_v
                       else {"maxiter": 1000, "ftol": 1e-13, "gtol": 1e-9})
        if res.success == False:   # noqa: E712  (as fit)
            warnings.warn("ERROR: optimization did not converge.")
        theta = theta_of(res.x)
        self.params.set_values(theta)
        ll, g, gs = loglik(res.x)
        self.fit_result = FittedLikelihood(self, ll, g, free, state["n_eval"], state["n_not_pd"], res,
                                           method=("Vecchia-REML" if getattr(vecchia, "reml", False) else "Vecchia-ML")
                                           if vecchia is not None else "ML" if trend is None else "REML",
                                           noise_scale=scales_of(res.x),
                                           noise_gradient=None if var is None else gs, noise_free=s_free)
        if vecchia is not None and getattr(vecchia, "trend", None) is not None:   # the trend at the optimum
            st = self._vecchia_eval(mf, vecchia, dist_units, fast_dist, measurement_error, scales_of(res.x), v_ranks)[2]
            self.fit_result.beta, self.fit_result.beta_cov = st["beta"], st["beta_cov"]
        if std_errors:
            # a parameter within 1e-8 of its bound width from a bound: conditioned on (no normal approximation on a boundary)
            u = np.asarray(res.x, dtype=float)
            at_bound = [names[k] for j, k in enumerate(free) if min(u[j], 1.0 - u[j]) <= 1e-8]
            at_bound += [f"noise_scale_{k}" for j, k in enumerate(s_free) if min(u[nf + j], 1.0 - u[nf + j]) <= 1e-8]
            held = [names[k] for k in sorted(hold)] + [f"noise_scale_{k}" for k in range(self.n_procs) if k not in s_free]
            if at_bound:
                warnings.warn(f"fit_likelihood: {', '.join(at_bound)} ended on a bound; the standard errors are conditional on "
                              "them and their own are NaN")
            inf = self.information(mf, dist_units, fast_dist, trend=trend, measurement_error=measurement_error,
                                   noise_scale=scales_of(res.x), fixed=held, _at_bound=at_bound, vecchia=vecchia,
                                   _ranks=v_ranks if vecchia is not None else None)
            self.fit_result.information = inf
            self.fit_result.at_bound = at_bound
            self.fit_result.std_error = inf.std_error
        return self


class FittedLikelihood:
    """Result of ``MultivariateMatern.fit_likelihood``: the maximised log-likelihood, AIC = 2 k - 2 l over the k free
    parameters, the gradient there, the numbers of evaluations and of evaluations at a Sigma that was not positive
    definite, and the optimiser's message.  ``method``: "ML", or "REML" for a fit with a trend (``loglik`` is then l_R)."""

    def __init__(self, model: MultivariateMatern, loglik: float, gradient, free, n_eval: int, n_not_pd: int, optim,
                 method: str = "ML", noise_scale=None, noise_gradient=None, noise_free=()) -> None:
        self.method = method
        self.params = model.params
        self.names = list(model.params.get_names())
        self.loglik = float(loglik)
        self.gradient = np.asarray(gradient, dtype=float)
        self.free = [self.names[k] for k in free]
        self.n_free = len(free) + len(noise_free)
        # measurement_error: the noise scales used (fit_noise_scale: found), dl/ds there, the processes whose scale was free
        self.noise_scale = noise_scale
        self.noise_gradient = None if noise_gradient is None else np.asarray(noise_gradient, dtype=float)
        self.noise_free = list(noise_free)
        self.aic = 2.0 * self.n_free - 2.0 * self.loglik
        self.n_eval = int(n_eval)
        self.n_not_pd = int(n_not_pd)
        self.success = bool(optim.success)
        self.message = optim.message if isinstance(optim.message, str) else str(optim.message)
        self.n_iter = int(getattr(optim, "nit", 0))
        # fit_likelihood(std_errors=True): the ParameterInformation at the optimum, its standard errors, the parameters that
        # ended on a bound
        self.information = None
        self.std_error = None
        self.at_bound = None
        # fit_likelihood(vecchia=Vecchia(trend=...)): the GLS trend coefficients at the optimum and their covariance A^-1
        self.beta = None
        self.beta_cov = None

    def conf_int(self, level: float = 0.95):
        """``information.conf_int(level)``; None without ``std_errors=True``."""
        return None if self.information is None else self.information.conf_int(level)


INFORMATION_SLOTS = 13


def information_slot_names(n_procs: int):
    """Names of the 13 slots of ``ck_loglik_fisher``: the model parameters in the flat order (one process: 4 of them, the
    other slots ""), then the noise scales."""
    names = list(MaternParams(n_procs=n_procs).get_names())
    names += [""] * (11 - len(names)) + ["noise_scale_0", "noise_scale_1" if n_procs == 2 else ""]
    return names


def summarize_information(fisher, n_procs: int, live=None, estimates=None, at_bound=None):
    """Pure numpy: the 13 x 13 information array of ``ck_loglik_fisher`` -> ``ParameterInformation``.  ``live``: 13 flags,
    the slots that are parameters here (None: every slot that has a name); ``estimates``: 13 values (for ``conf_int``);
    ``at_bound``: 13 flags, live parameters that are conditioned on and reported with NaN.
    The inversion works on the matrix scaled to unit diagonal.  A live parameter with I_kk == 0 is not identified: NaN
    everywhere, named in ``not_identified``, one warning.  If the rest is not positive definite every standard error is
    NaN, with one warning."""
    fisher = np.asarray(fisher, dtype=float)
    if fisher.shape != (INFORMATION_SLOTS, INFORMATION_SLOTS):
        raise ValueError("fisher: the 13 x 13 array of ck_loglik_fisher")
    names13 = information_slot_names(n_procs)
    named = np.array([n != "" for n in names13])
    live = named.copy() if live is None else (np.asarray(live, dtype=bool) & named)
    bound = np.zeros(INFORMATION_SLOTS, dtype=bool) if at_bound is None else (np.asarray(at_bound, dtype=bool) & live)
    idx = np.flatnonzero(live)
    names = [names13[k] for k in idx]
    n = idx.size
    sub = fisher[np.ix_(idx, idx)]
    cov = np.full((n, n), np.nan)
    corr = np.full((n, n), np.nan)
    diag = np.diag(sub)
    is_bound = bound[idx]
    dead = ~is_bound & (diag == 0.0)
    not_identified = [names[j] for j in np.flatnonzero(dead)]
    if not_identified:
        warnings.warn(f"information: {', '.join(not_identified)} not identified at these parameters (zero information); "
                      "reported as NaN")
    keep = np.flatnonzero(~is_bound & ~dead)
    positive_definite = True
    if keep.size:
        d = diag[keep]
        ok = np.all(np.isfinite(sub[np.ix_(keep, keep)])) and np.all(d > 0.0)
        if ok:
            s = 1.0 / np.sqrt(d)
            c = sub[np.ix_(keep, keep)] * np.outer(s, s)
            try:
                lc = np.linalg.cholesky(c)
                li = np.linalg.solve(lc, np.eye(keep.size))
                ci = li.T @ li
                cov[np.ix_(keep, keep)] = ci * np.outer(s, s)
                sd = np.sqrt(np.diag(ci))
                corr[np.ix_(keep, keep)] = ci / np.outer(sd, sd)
            except LinAlgError:
                ok = False
        if not ok:
            positive_definite = False
            warnings.warn("information: the information matrix of the identified parameters is not positive definite; every "
                          "standard error is NaN")
    est = None if estimates is None else np.asarray(estimates, dtype=float)[idx]
    return ParameterInformation(names, sub, cov, corr, est, not_identified, [names[j] for j in np.flatnonzero(is_bound)],
                                positive_definite)


class ParameterInformation:
    """Fisher information of the likelihood and the asymptotic covariance of the estimates: ``names`` (the live parameters;
    noise scales as ``noise_scale_0/1``), ``fisher``, ``cov`` = its inverse over the identified parameters (NaN rows and
    columns for the others), ``std_error`` (a ``pd.Series`` by name), ``correlation``, ``not_identified``, ``at_bound``,
    ``positive_definite`` and ``conf_int(level)`` (normal quantiles)."""

    def __init__(self, names, fisher, cov, correlation, estimates, not_identified, at_bound, positive_definite) -> None:
        self.names = list(names)
        self.fisher = fisher
        self.cov = cov
        self.correlation = correlation
        self.estimates = None if estimates is None else pd.Series(estimates, index=self.names)
        self.std_error = pd.Series(np.sqrt(np.diag(cov)) if len(self.names) else np.zeros(0), index=self.names)
        self.not_identified = list(not_identified)
        self.at_bound = list(at_bound)
        self.positive_definite = bool(positive_definite)
        self.beta_cov = None   # information(vecchia=Vecchia(trend=...)): Cov(beta-hat) = A^-1 of the profiled trend

    def conf_int(self, level: float = 0.95):
        """estimate -+ z std_error with z the normal quantile of (1 + level) / 2: a DataFrame (lower, upper) by name."""
        from scipy.special import ndtri
        if not 0.0 < level < 1.0:
            raise ValueError("level: a probability inside (0, 1)")
        if self.estimates is None:
            raise ValueError("conf_int needs the estimates")
        z = float(ndtri(0.5 * (1.0 + level)))
        return pd.DataFrame({"lower": self.estimates - z * self.std_error, "upper": self.estimates + z * self.std_error},
                            index=self.names)


class FittedVariogram:
    """Model parameters and theoretical variogram for the corresponding empirical variogram
    (src/model.py:320-347)."""

    def __init__(self, model: MultivariateMatern, estimate, cost: float) -> None:
        self.config = estimate.config
        self.timestamp = estimate.timestamp
        self.timedeltas = estimate.timedeltas
        self.df_empirical = estimate.df
        h = np.linspace(0, self.df_empirical["bin_center"].max(), 100)
        self.df_theoretical = model.variograms(h)
        self.params = model.params
        self.cost = cost
        self.cs_valid = self.cs_check()

    def cs_check(self):
        """Placeholder in the reference as well (src/model.py:337-347): always None."""
        return None
