"""The extended-precision Matern fixture (tests/golden/matern_mp.npz, written by tests/golden/make_matern_mp.py with mpmath
alone) and the bounds an evaluator of csrc/ck_math.h is held to against it -- shared by tests/test_matern_mp_host.py (the
header compiled with g++) and tests/test_gpu_matern_mp.py (the device build), so that the host proves the bounds satisfiable
and the device meets the same ones.

Units.  eps = 2^-52 and, per entry,
    u = eps (1 + |ln M| + s + nu |ln s|):
the evaluator forms the prefactor's exponent lnpref + nu ln s - s term by term and exponentiates it, so the relative error of M
is a few roundings of the size of those terms; s itself carries about three roundings and |d ln M / d ln s| <= s + nu.
    value      |M / M_ref - 1| <= 8 u + 5e-15 where M_ref > 1e-290 (5e-15: the project's K_nu bound, tests/test_host_math.py;
               8: twice the four roundings of the exponent path), 1e-290 absolute below
    gamma      |gamma - sigma^2 (1 - M_ref)| <= sigma^2 M_ref (8 u + 5e-15): the value bound carried through the subtraction
    dM/dlen    the value bound, relative.  Below M_ref = 1e-290: 1e-290 (1 + s / len) absolute -- dM/dlen = (s / len) D and
               D / M = K_(nu-1) / K_nu is 1 to within 1 / s out there
    dM/dnu     against the library's own formula evaluated exactly (stencil): 8 u (18 M / (12 dnu) + |D s / (2 nu)|) -- the
               weights 1 + 8 + 8 + 1 of the four evaluations and the correction term, rounding only; below M_ref = 1e-290 the
               same expression with 1e-290 in place of 8 u M.  Against the true derivative: 1e-7 in the scale
               max(|ref|, 1 % of its largest value), the bound of tests/test_host_matern_grad.py -- the stencil's truncation
"""
import os

import numpy as np

EPS = 2.0 ** -52
TINY = 1e-290
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CK_DNU_REL = 2e-3   # csrc/ck_math.h


def load():
    g = np.load(os.path.join(GOLDEN, "matern_mp.npz"))
    return {k: g[k] for k in g.files}


def lags_of(g, nu, ell):
    """the float64 lags of one (nu, ell), as the generator makes them (h = 0 last)"""
    return g["s_grid"] * ell / np.sqrt(2.0 * nu)


def sym(L):
    """a symmetric matrix from the lower triangle the fixture stores"""
    return L + np.tril(L, -1).T


class Lags:
    """one (nu, ell) of the fixture's lag grid: the lags without h = 0, the references and the bounds"""

    def __init__(self, g, k, e):
        self.nu, self.ell = float(g["nus"][k]), float(g["ells"][e])
        self.h_all = lags_of(g, self.nu, self.ell)
        assert self.h_all[-1] == 0.0 and np.all(self.h_all[:-1] > 0)
        self.h = self.h_all[:-1]
        self.s = np.sqrt(2.0 * self.nu) * (self.h / self.ell)
        for name in ("M", "lnM", "D", "dMdl", "dMdnu", "dMdnu_st"):
            setattr(self, name, g[name][k, e, :-1])
        self.omM = g["omM"][k, e]
        self.big = self.M > TINY
        self.u = EPS * (1.0 + np.abs(self.lnM) + self.s + self.nu * np.abs(np.log(self.s)))
        self.vb = 8.0 * self.u + 5e-15
        self.dnu = CK_DNU_REL * self.nu

    def value(self, M):
        """error of M in units of its bound (largest over the lags)"""
        with np.errstate(all="ignore"):
            e = np.where(self.big, np.abs(M / self.M - 1.0) / self.vb, np.abs(M - self.M) / TINY)
        return float(e.max())

    def gamma(self, gam):
        """error of the semivariogram (sigma = 1, no nugget) at the small lags in units of its bound"""
        n = len(self.omM)
        return float(np.max(np.abs(gam - self.omM) / (self.M[:n] * self.vb[:n])))

    def dlen(self, d):
        with np.errstate(all="ignore"):
            e = np.where(self.big, np.abs(d / self.dMdl - 1.0) / self.vb,
                         np.abs(d - self.dMdl) / (TINY * (1.0 + self.s / self.ell)))
        return float(e.max())

    def dnu_rounding(self, d):
        w = 18.0 / (12.0 * self.dnu)
        corr = self.s / (2.0 * self.nu)
        bound = np.where(self.big, 8.0 * self.u * (w * self.M + np.abs(self.D) * corr), TINY * (w + corr))
        return float(np.max(np.abs(d - self.dMdnu_st) / bound))

    def dnu_truncation(self, d):
        """error against the true derivative in the scale max(|ref|, 1 % of its largest value): the bound is 1e-7"""
        scale = np.maximum(np.abs(self.dMdnu), 1e-2 * np.max(np.abs(self.dMdnu)))
        return float(np.max(np.abs(d - self.dMdnu) / scale))

    def stencil_truncation(self):
        """the method's own truncation, reference against reference, in the same scale"""
        return self.dnu_truncation(self.dMdnu_st)


def check_grad_rows(L, out3_all):
    """(M, dM/dnu, dM/dlen) rows of an evaluator at L.h_all: the exact rows, then the four errors in units of their bounds"""
    assert out3_all[-1].tolist() == [1.0, 0.0, 0.0], (L.nu, L.ell)                       # h == 0
    out = out3_all[:-1]
    zero = out[:, 0] == 0.0
    assert np.all(out[zero, 1] == 0.0) and np.all(out[zero, 2] == 0.0), (L.nu, L.ell)   # M == 0: constant there
    return L.value(out[:, 0]), L.dlen(out[:, 2]), L.dnu_rounding(out[:, 1]), L.dnu_truncation(out[:, 1])


# ---- the gradient and the information from the fixture's matrices ---------------------------------------------------------
def grad_reference(g, tag, stencil):
    """(S, z, {slot: D_slot}) of a gradient case with the nu slots true or as the library's stencil"""
    S, z = sym(g[f"{tag}_S"]), g[f"{tag}_z"]
    D = {k: sym(g[f"{tag}_D"][k]) for k in range(11)}
    if stencil:
        for b in range(3):
            D[2 + b] = sym(g[f"{tag}_Dnu_st"][b])
    return S, z, D


def dense_gradient(S, z, D):
    """1/2 z^T S^-1 D_k S^-1 z - 1/2 tr(S^-1 D_k) over the slots of D"""
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    a = Si @ z
    return np.array([0.5 * a @ D[k] @ a - 0.5 * np.sum(Si * D[k]) for k in sorted(D)])
