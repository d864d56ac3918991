"""Fixtures and references of tests/test_gpu_vecchia_edge_sizes.py and tests/test_vecchia_edge_host.py: the Vecchia entry points
(ck_loglik_vecchia, _grad, _fisher, _trend, _trend_grad) at the sizes their kernels index by.

  the ladder   prefixes of vecchia_ref.half_colocated_sites(600) around a run of 8 data (k_vecchia_info), a 64-row strip (the
               process boundary ga >= n0p) and a 256-term tree (k_vecchia_terms, _grad_part, _trend_gram), and one process alone;
  the sums     a call's totals against the exactly rounded sum (math.fsum) of that same call's per-datum outputs, within
               64 u sum |x_t| (u = 2^-53): the device tree is at most ceil(nblk / 256) + 16 additions deep and the per-term log,
               division and product differ from numpy's by a few ulp each;
  the tall     N = 35 000 + 35 001 (274 partial sums: the second trip of every k_*_sum loop) with a reference on a sample of
  case         256 data: the candidates by brute force over all sites, then vecchia_ref.conditioning_sets / vecchia_reference /
               vecchia_grad_reference themselves on the sub-problem of the candidates and the datum;
  the wide     eight polynomial columns per process (p = 16), a process without a trend, unequal blocks.
  designs
Every reference is computed once per case (functools.lru_cache) and left unchanged."""
import functools
import math

import numpy as np
from scipy.linalg import solve_triangular

from oracle import cokrige_oracle as orc
from tests import dense_chains as dc
from tests import vecchia_grad_ref as vgr
from tests import vecchia_info_ref as vir
from tests import vecchia_ref as vr
from tests import vecchia_trend_ref as vtr

HAV, EUC = 0, 1
U = 2.0 ** -53
SUM_FACTOR = 64.0            # the bound of a sum: SUM_FACTOR * U * sum |x_t|
GRAM_RECOVERY = 1e-12        # relative, for G recovered through inv(Cov(beta)) (cond(A) < 1e3 is asserted on the host)

# ---------------------------------------------------------------------------------------------------------------------
# 1. the ladder
# ---------------------------------------------------------------------------------------------------------------------
RUNGS = [(1, 1), (2, 1), (7, 9), (8, 8), (9, 8), (8, 9),          # processes below, on and one past a run of 8; N below one wave
         (64, 64), (63, 65), (65, 63), (64, 1), (1, 64),          # n0p = 64 with and without a gap, n0p = 128, one-site processes
         (128, 129), (255, 1),                                    # N = 257 and N = 256, the boundary on and off a strip
         (256, 256), (257, 255), (300, 213)]                      # N = 512 exactly (two ways), N = 513
UNI = [1, 8, 9, 256, 257]
UNI_PARAMS = [1.0, 1.5, 0.2, 0.02]
LADDER = [f"{a}+{b}" for a, b in RUNGS] + [f"uni{n}" for n in UNI]
MAX_DIST, CAPS = 0.5, (4, 4)
N_SITES = 600


def sizes_of(label):
    return (int(label[3:]),) if label.startswith("uni") else tuple(int(x) for x in label.split("+"))


@functools.lru_cache(maxsize=None)
def _sites(n):
    return vr.half_colocated_sites(n)


def problem(sizes, n_sites=N_SITES, caps=CAPS, max_dist=MAX_DIST):
    """prefixes [:n_k] of half_colocated_sites(n_sites), SET_B_UNIT (one process: UNI_PARAMS), Euclid, ranks
    default_rng(11).permutation(N)"""
    from sif_xco2_cokriging_amd import synth
    coords, values = _sites(n_sites)
    N = sum(sizes)
    return dict(coords=[np.ascontiguousarray(coords[k][:n]) for k, n in enumerate(sizes)],
                values=[np.ascontiguousarray(values[k][:n]) for k, n in enumerate(sizes)],
                params=list(synth.SET_B_UNIT) if len(sizes) == 2 else list(UNI_PARAMS), metric=EUC, max_dist=max_dist,
                caps=tuple(caps[:len(sizes)]), ranks=np.random.default_rng(11).permutation(N).astype(np.int64))


@functools.lru_cache(maxsize=None)
def rung(label):
    return problem(sizes_of(label))


def handle_caps(pb):
    return tuple(pb["caps"]) + (0,) * (2 - len(pb["caps"]))


def npar_of(pb):
    return len(pb["params"])


def value_reference_of(pb, noise=None):
    return vr.vecchia_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], pb["ranks"], pb["max_dist"], pb["caps"],
                                noise=noise)


@functools.lru_cache(maxsize=None)
def value_reference(label):
    return value_reference_of(rung(label))


@functools.lru_cache(maxsize=None)
def _ladder_dS(n_procs):
    """vecchia_grad_ref.derivative_matrices once on the longest prefixes of the ladder; a rung takes its rows and columns
    (every entry depends on its own pair of sites only)"""
    n = [max(sizes_of(lb)[k] for lb in LADDER if len(sizes_of(lb)) == n_procs) for k in range(n_procs)]
    pb = problem(tuple(n))
    return n, vgr.derivative_matrices(pb["params"], pb["coords"], pb["metric"])


def ladder_dS(label):
    sz = sizes_of(label)
    n, dS = _ladder_dS(len(sz))
    ix = np.concatenate([np.arange(m) + (0 if k == 0 else n[0]) for k, m in enumerate(sz)])
    return [D[np.ix_(ix, ix)] for D in dS]


@functools.lru_cache(maxsize=None)
def grad_reference(label):
    pb = rung(label)
    return vgr.vecchia_grad_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], value_reference(label),
                                      dS=ladder_dS(label))


@functools.lru_cache(maxsize=None)
def info_reference(label, scale=1.0):
    pb = rung(label)
    return vir.vecchia_info_reference(pb["params"], pb["coords"], pb["metric"], value_reference(label)["keep"], scale=scale)


# The reference's own floor in the length-scale class per rung: what halving dense_chains._d4's step changes, in
# dense_chains.normalised's measure (tests/test_vecchia_edge_host.py: test_reference_floor measures and prints it, the procedure of
# tests/test_vecchia_info_host.py: test_reference_floor).  Measured on the host, rounded up in the third digit; a rung is listed
# only when its floor exceeds 1e-10.  The bound of the length-scale class is max(1e-9, 10 x the floor).
# (1+1 and uni1 have no length-scale information at all: co-located sites, one site; the length scales are 0.2 under _d4's
# absolute step of 1e-3, as on the fixtures of tests/vecchia_info_ref.py, hence floors of the order 1e-9.)
EDGE_INFO_LEN_FLOOR = {"2+1": 5.48e-9, "7+9": 2.48e-9, "8+8": 2.95e-9, "9+8": 2.94e-9, "8+9": 2.94e-9,
                       "64+64": 3.93e-9, "63+65": 3.89e-9, "65+63": 3.84e-9, "64+1": 4.91e-9, "1+64": 4.61e-9,
                       "128+129": 5.98e-9, "255+1": 8.96e-9, "256+256": 7.64e-9, "257+255": 7.69e-9, "300+213": 7.88e-9,
                       "uni8": 3.94e-9, "uni9": 3.05e-9, "uni256": 8.99e-9, "uni257": 9.03e-9, "info_tall": 8.64e-9}


def info_tol(label):
    return dict(vir.INFO_TOL, len=max(1e-9, 10.0 * EDGE_INFO_LEN_FLOOR.get(label, 0.0)))


def info_live(ref):
    """the slots with information in the reference (a rung of co-located sites alone has none in its length scales and nu)"""
    return np.flatnonzero(np.diag(ref) > 0)


def trend_kinds(sizes):
    """"linear" for a process with at least 8 sites, "constant" for a smaller one"""
    return tuple("linear" if n >= 8 else "constant" for n in sizes)


def trend_design(pb, kinds):
    """(X, [F_k]): the regressors of trend.TrendDesign, the kind chosen per process"""
    from sif_xco2_cokriging_amd.trend import TrendDesign
    F = [TrendDesign(kind, [c]).data(0, c) for kind, c in zip(kinds, pb["coords"])]
    return vtr.block_design(F), F


def trend_reference_of(pb, X, F, noise=None):
    ref = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], X, pb["metric"], pb["ranks"], pb["max_dist"],
                                      pb["caps"], noise=noise)
    ref["F"] = F
    ref["prior"] = np.diag(vtr.joint_cov(pb["params"], pb["coords"], pb["metric"])).copy()
    ref["own"] = np.zeros(len(ref["z"])) if noise is None else np.concatenate(
        [np.zeros(len(c)) if d is None else d for c, d in zip(pb["coords"], noise)])
    return ref


@functools.lru_cache(maxsize=None)
def trend_reference(label):
    """the dict tests/test_gpu_vecchia_trend.py: check_case takes (F, prior and own included)"""
    pb = rung(label)
    X, F = trend_design(pb, trend_kinds(sizes_of(label)))
    return trend_reference_of(pb, X, F)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sums, held to their own terms
# ---------------------------------------------------------------------------------------------------------------------
def exact_sum(terms):
    """(the exactly rounded sum, its bound SUM_FACTOR u sum |x_t|)"""
    t = np.asarray(terms, dtype=float).ravel().tolist()
    return math.fsum(t), SUM_FACTOR * U * math.fsum(abs(x) for x in t)


def value_sums(z, mean, var):
    """[(sum, bound)] of log var and of (z - mean)^2 / var over a value call's own terms"""
    return [exact_sum(np.log(var)), exact_sum((z - mean) ** 2 / var)]


def score_sums(score):
    return [exact_sum(score[:, c]) for c in range(score.shape[1])]


def trend_rows(z, X, prior_own, mu, vv, g):
    """the rows (z_t - mu_t, x_t - g_t) / s_t from debug_vecchia_trend's outputs (an empty set has mu = vv = g = 0)"""
    rs = 1.0 / np.sqrt(prior_own - vv)
    return np.column_stack([(z - mu) * rs, (X - g) * rs[:, None]])


def gram_of_rows(rows):
    """(G, bound): every entry of R^T R exactly rounded, and SUM_FACTOR u sum_t |r_ta r_tb|"""
    w = rows.shape[1]
    G, B = np.zeros((w, w)), np.zeros((w, w))
    for a in range(w):
        for b in range(a + 1):
            G[a, b], B[a, b] = exact_sum(rows[:, a] * rows[:, b])
            G[b, a], B[b, a] = G[a, b], B[a, b]
    return G, B


def recovered_gram(out5, beta, cov):
    """G = [[yy, b], [b, A]] from a trend call's outputs: A = inv(Cov(beta)), b = A beta, yy = out5[4]"""
    p = len(beta)
    G = np.zeros((p + 1, p + 1))
    G[0, 0] = out5[4]
    if p:
        A = np.linalg.inv(cov)
        G[1:, 1:] = A
        G[1:, 0] = G[0, 1:] = A @ beta
    return G


def gram_excess(G_call, G_rows, bound):
    """the largest |G_call - G_rows| / (bound + GRAM_RECOVERY |G_rows|) over the entries: <= 1 passes"""
    return float(np.max(np.abs(G_call - G_rows) / (bound + GRAM_RECOVERY * np.abs(G_rows) + 1e-300)))


# ---------------------------------------------------------------------------------------------------------------------
# 3a. the tall case and the sampled reference
# ---------------------------------------------------------------------------------------------------------------------
TALL_SIZES = (35000, 35001)
TALL_SAMPLE = 256


@functools.lru_cache(maxsize=None)
def tall_problem(sizes=TALL_SIZES, max_dist=0.012, caps=(3, 3)):
    """uniform sites on the unit square (default_rng(7001)), process 1's first sizes[0] // 2 sites co-located with process 0's,
    standard normal values (the likelihood does not need a draw from the model), random ranks"""
    from sif_xco2_cokriging_amd import synth
    rng = np.random.default_rng(7001)
    c0, c1 = rng.random((sizes[0], 2)), rng.random((sizes[1], 2))
    c1[:sizes[0] // 2] = c0[:sizes[0] // 2]
    values = [rng.standard_normal(sizes[0]), rng.standard_normal(sizes[1])]
    return dict(coords=[c0, c1], values=values, params=list(synth.SET_B_UNIT), metric=EUC, max_dist=max_dist, caps=caps,
                ranks=rng.permutation(sum(sizes)).astype(np.int64))


def tall_sample(sizes=TALL_SIZES, count=TALL_SAMPLE):
    """sorted stacked indices: the first and the last datum of each process, 255, 256, 65 535 and 65 536 where they exist, the
    last index, the rest drawn by default_rng(7002)"""
    N = sum(sizes)
    fixed = [0, sizes[0] - 1, sizes[0], N - 1] + [t for t in (255, 256, 65535, 65536) if t < N]
    rest = np.setdiff1d(np.arange(N), fixed)
    extra = np.random.default_rng(7002).choice(rest, size=count - len(set(fixed)), replace=False)
    out = np.sort(np.concatenate([np.array(sorted(set(fixed)), dtype=np.int64), extra]))
    assert len(out) == min(count, N) and len(np.unique(out)) == len(out)
    return out


def sampled_reference(pb, sample, values=None, X=None, scores=True):
    """The terms of the data `sample` (stacked indices) without an N x N matrix.  Per datum t: its distances to ALL sites
    (oracle.distance_matrix on one row: the bits of the full matrix), the candidates = the sites of smaller rank within max_dist,
    then the sub-problem of the candidates and t through vecchia_ref.conditioning_sets (the cap rule), vecchia_reference and
    vecchia_grad_reference, each on the one row of t; with a design X (N, p) also g_t = U^T v in vecchia_trend_reference's form
    (that function itself inverts the sub-problem's normal matrix, which one row does not determine).
    dict(index, mean, var, count (m, 2), gap, capped, score (m, 13), g (m, p)); values: in place of pb["values"] (a residual)."""
    coords, metric, ranks = pb["coords"], pb["metric"], np.asarray(pb["ranks"])
    n_procs = len(coords)
    allc = np.vstack(coords)
    proc = np.concatenate([np.full(len(c), q) for q, c in enumerate(coords)])
    z = np.concatenate([np.asarray(v, dtype=float) for v in (pb["values"] if values is None else values)])
    m = len(sample)
    out = dict(index=np.asarray(sample), mean=np.zeros(m), var=np.zeros(m), count=np.zeros((m, 2), dtype=np.int64),
               gap=np.full(m, np.inf), capped=np.zeros(m, dtype=bool), score=np.zeros((m, 13)),
               g=None if X is None else np.zeros((m, X.shape[1])))
    for i, t in enumerate(sample):
        d = orc.distance_matrix(allc[t:t + 1], allc, metric)[0]
        cand = np.flatnonzero((ranks < ranks[t]) & (d <= pb["max_dist"]))
        ix = np.sort(np.r_[cand, t])                                  # stacked order: process 0 first
        pos = int(np.searchsorted(ix, t))
        sub = [allc[ix[proc[ix] == q]] for q in range(n_procs)]
        subv = [z[ix[proc[ix] == q]] for q in range(n_procs)]
        D = orc.distance_matrix(allc[ix], allc[ix], metric)
        keep, gap, capped = vr.conditioning_sets(D, proc[ix], ranks[ix], pb["max_dist"], pb["caps"])
        only = np.zeros_like(keep)
        only[pos] = keep[pos]                                         # the other rows: empty sets, not looked at
        sets = (only, gap, capped)
        ref = vr.vecchia_reference(pb["params"], sub, subv, metric, None, None, sets=sets)
        assert ref["info"] == 0
        c = np.flatnonzero(only[pos])
        if X is not None and c.size:                                  # g_t = U^T v as vecchia_trend_reference forms it
            S = vtr.joint_cov(pb["params"], sub, metric)
            L = np.linalg.cholesky(S[np.ix_(c, c)])
            out["g"][i] = solve_triangular(L, X[ix][c], lower=True).T @ solve_triangular(L, S[c, pos], lower=True)
        out["mean"][i], out["var"][i], out["count"][i] = ref["mean"][pos], ref["var"][pos], ref["count"][pos]
        out["gap"][i], out["capped"][i] = gap[pos], capped[pos]
        if scores:
            out["score"][i] = vgr.vecchia_grad_reference(pb["params"], sub, subv, metric, ref)["score"][pos]
    return out


def constant_design(pb):
    """(X, [F_k]): one column of ones per process"""
    F = [np.ones((len(c), 1)) for c in pb["coords"]]
    return vtr.block_design(F), F


@functools.lru_cache(maxsize=None)
def tall_reference():
    """sampled_reference of the tall case with the constant design (mean, var, count and the scores are those of the plain
    likelihood; g rides along)"""
    pb = tall_problem()
    return sampled_reference(pb, tall_sample(), X=constant_design(pb)[0])


# ---------------------------------------------------------------------------------------------------------------------
# 3b. the information beyond 256 rows of partial sums
# ---------------------------------------------------------------------------------------------------------------------
INFO_TALL_SIZES = (1030, 1029)           # 129 + 129 = 258 rows of 8 data
INFO_TALL = "info_tall"


@functools.lru_cache(maxsize=None)
def info_tall_problem():
    return problem(INFO_TALL_SIZES, n_sites=1100, caps=(2, 2))


@functools.lru_cache(maxsize=None)
def info_tall_sets():
    return value_reference_of(info_tall_problem())


@functools.lru_cache(maxsize=None)
def info_tall_reference(scale=1.0):
    pb = info_tall_problem()
    return vir.vecchia_info_reference(pb["params"], pb["coords"], pb["metric"], info_tall_sets()["keep"], scale=scale)


# ---------------------------------------------------------------------------------------------------------------------
# 4. trend width
# ---------------------------------------------------------------------------------------------------------------------
def wide_columns(c):
    x, y = (c[:, 0] - 0.5) / 0.29, (c[:, 1] - 0.5) / 0.29
    return np.column_stack([np.ones(len(c)), x, y, x * x - 1.0, x * y, y * y - 1.0, x ** 3, y ** 3])


@functools.lru_cache(maxsize=None)
def wide_trend(p0, p1):
    """the callable trend.TrendDesign takes: per process the first p_k of [1, x, y, x^2 - 1, x y, y^2 - 1, x^3, y^3] at
    x = (c0 - 0.5) / 0.29, y = (c1 - 0.5) / 0.29.  One object per (p0, p1): test_gpu_vecchia_trend.reference keys on it."""
    def trend(k, c):
        return wide_columns(np.atleast_2d(np.asarray(c, dtype=float)))[:, :(p0, p1)[k]]
    return trend


WIDE_CASES = [((8, 8), (32, 32)), ((8, 0), (16, 16)), ((0, 8), (16, 16)), ((1, 7), (16, 16))]
