"""Vecchia's approximation of the Gaussian log-likelihood (include/cokrige.h: ck_loglik_vecchia): every datum conditioned on
the data that come earlier in a fixed ordering, within ``max_dist`` and under a nearest-neighbour cap per process.  This module
holds the configuration and the orderings; the evaluation is ``MultivariateMatern.log_likelihood(..., vecchia=Vecchia(...))``,
the fit ``fit_likelihood(..., vecchia=...)``, the per-datum table ``vecchia_terms``."""
import numpy as np
import pandas as pd

from . import native
from .point_prediction import check_max_neighbours
from .trend import check_trend

ORDERINGS = ("random", "hilbert")
GRADIENTS = ("numeric", "analytic")
INFORMATIONS = ("none", "expected")
TREND_LIKELIHOODS = ("profile", "reml")


def check_ordering(ordering):
    """"random", "hilbert" or an explicit array of distinct integer ranks (returned as a flat int64 array)."""
    if isinstance(ordering, str):
        if ordering not in ORDERINGS:
            raise ValueError(f"ordering must be one of {ORDERINGS} or an array of ranks, got {ordering!r}")
        return ordering
    r = np.asarray(ordering)
    if r.ndim != 1 or r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("an explicit ordering is a one-dimensional array of integer ranks")
    r = r.astype(np.int64)
    if np.unique(r).size != r.size:
        raise ValueError("an explicit ordering must not hold the same rank twice")
    return r


def check_seed(seed):
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError(f"seed must be a non-negative integer, got {seed!r}")
    return int(seed)


def ordering_ranks(coords_per_process, ordering="random", seed=0):
    """The stacked int64 ranks (process 0 then 1) of the data at ``coords_per_process`` (one (n_k, 2) array per process):
    a permutation of 0 .. N - 1 for "random" (``np.random.default_rng(seed).permutation(N)``) and for "hilbert" (the rank of a
    datum is its place along the library's Hilbert curve through all N stacked sites, ``ck_hilbert_order``); an explicit array
    is checked (N distinct integers) and returned."""
    cs = [np.asarray(c, dtype=np.float64).reshape(-1, 2) for c in coords_per_process]
    n = int(sum(c.shape[0] for c in cs))
    ordering = check_ordering(ordering)
    if isinstance(ordering, np.ndarray):
        if ordering.size != n:
            raise ValueError(f"the ordering has {ordering.size} ranks, the data {n} sites")
        return ordering
    if ordering == "random":
        return np.random.default_rng(check_seed(seed)).permutation(n).astype(np.int64)
    perm = native.hilbert_order(np.concatenate(cs, axis=0)) if n else np.zeros(0, dtype=np.int64)
    ranks = np.empty(n, dtype=np.int64)
    ranks[np.asarray(perm, dtype=np.int64)] = np.arange(n, dtype=np.int64)
    return ranks


class Vecchia:
    """Configuration of the Vecchia likelihood: ``max_dist`` (in the distance units of the call), ``max_neighbours`` (None,
    an int for every process or one int per process; 0 = no cap), ``ordering`` ("random", "hilbert" or an array of ranks) and
    the ``seed`` of the random ordering.  ``gradient``: "numeric" (the default: ``fit_likelihood`` differences the value) or
    "analytic" (``ck_loglik_vecchia_grad``: value and gradient from one native call, for conditioning sets of at most 64 data --
    ``log_likelihood(..., gradient=True)`` then works and the fit uses it).  ``information``: "none" (the default:
    ``fit_likelihood(..., std_errors=True)`` is refused) or "expected" (``ck_loglik_vecchia_fisher``: the fit reports the expected
    information of the Vecchia objective under the exact model and the standard errors that follow from it, for conditioning
    sets of at most 64 data; it is what GpGp reports, not a Godambe sandwich).  ``trend`` (None, the default: zero mean; or
    "constant", "linear", a callable, as ``Predictor(trend=...)``): an unknown mean X beta estimated by GLS inside the likelihood
    (``ck_loglik_vecchia_trend``, conditioning sets of at most 64 data); ``trend_likelihood``: "profile" (the default: beta
    profiled out of the likelihood, analytic gradient available) or "reml" (the restricted form, value only: the fit differences
    it).  Validated here, before any device work."""

    def __init__(self, max_dist, max_neighbours=None, ordering="random", seed=0, gradient="numeric", information="none",
                 trend=None, trend_likelihood="profile"):
        if isinstance(max_dist, (bool, np.bool_)) or not isinstance(max_dist, (int, float, np.integer, np.floating)):
            raise ValueError(f"max_dist must be a number, got {max_dist!r}")
        if not np.isfinite(max_dist) or max_dist < 0:
            raise ValueError(f"max_dist must be finite and >= 0, got {max_dist!r}")
        self.max_dist = float(max_dist)
        if max_neighbours is not None and not np.isscalar(max_neighbours):
            max_neighbours = tuple(max_neighbours)
            if len(max_neighbours) not in (1, 2):
                raise ValueError(f"max_neighbours needs one value per process, got {len(max_neighbours)}")
        self.max_neighbours = max_neighbours
        if max_neighbours is not None:   # the values; the count is checked against the model's processes in caps()
            check_max_neighbours(max_neighbours, 1 if np.isscalar(max_neighbours) else len(max_neighbours))
        self.ordering = check_ordering(ordering)
        self.seed = check_seed(seed)
        if not isinstance(gradient, str) or gradient not in GRADIENTS:
            raise ValueError(f"gradient must be one of {GRADIENTS}, got {gradient!r}")
        self.gradient = gradient
        if not isinstance(information, str) or information not in INFORMATIONS:
            raise ValueError(f"information must be one of {INFORMATIONS}, got {information!r}")
        self.information = information
        self.trend = check_trend(trend)
        if not isinstance(trend_likelihood, str) or trend_likelihood not in TREND_LIKELIHOODS:
            raise ValueError(f"trend_likelihood must be one of {TREND_LIKELIHOODS}, got {trend_likelihood!r}")
        self.trend_likelihood = trend_likelihood

    @property
    def reml(self):
        """True when the configuration asks for the restricted likelihood of a trend."""
        return self.trend is not None and self.trend_likelihood == "reml"

    def caps(self, n_procs):
        """The pair of caps for a model of ``n_procs`` processes ((0, 0): none)."""
        caps = check_max_neighbours(self.max_neighbours, n_procs)
        return (0, 0) if caps is None else caps

    def ranks(self, coords_per_process):
        return ordering_ranks(coords_per_process, self.ordering, self.seed)


def _coords(mf, n_procs):
    return [np.ascontiguousarray(np.asarray(mf.fields[k].coords_main, dtype=np.float64)[:, :2]) for k in range(n_procs)]


def vecchia_terms(model, mf, vecchia, dist_units="km", fast_dist=True, measurement_error=None, noise_scale=None, ranks=None):
    """One row per datum of the Vecchia likelihood of ``mf`` under ``model``: process, index (within the process), mean and
    variance of the conditional density of the observation, n0 / n1 = the conditioning data of either process.  The frame's
    ``attrs`` hold out3, info and the counters of the call.  With ``Vecchia(trend=...)`` the mean is the native call's
    mu_t + f_t^T beta-hat, out3 is that call's out5 = (l, sum log s^2, log|A|, Q, yy) and ``attrs`` also hold beta and beta_cov."""
    out3, info, st = model._vecchia_eval(mf, vecchia, dist_units, fast_dist, measurement_error, noise_scale, ranks, terms=True)
    ns = [np.asarray(mf.fields[k].values_main).size for k in range(model.n_procs)]
    df = pd.DataFrame({"process": np.repeat(np.arange(model.n_procs), ns),
                       "index": np.concatenate([np.arange(n) for n in ns]),
                       "mean": st["mean"], "variance": st["var"],
                       "n0": st["count"][:, 0].astype(np.int64), "n1": st["count"][:, 1].astype(np.int64)})
    df.attrs.update(out3=out3, info=info, n_empty=st["n_empty"], k_max=st["k_max"], n_capped=st["n_capped"])
    if vecchia.trend is not None:
        df.attrs.update(beta=st["beta"], beta_cov=st["beta_cov"])
    return df
