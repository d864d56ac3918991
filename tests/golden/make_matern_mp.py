#!/usr/bin/env python3
"""Generate tests/golden/matern_mp.npz: the Matern correlation, its derivatives and whole covariance matrices in extended
precision (mpmath, 40 digits), rounded to float64 once at the end.  Only mpmath and numpy: no scipy, no oracle, nothing of the
reference -- the truth the device evaluator of csrc/ck_math.h is held to by tests/test_matern_mp_host.py (host build of the
header) and tests/test_gpu_matern_mp.py (device build).

Usage:  python tests/golden/make_matern_mp.py            (writes next to itself; deterministic)

Everything is computed from the float64 inputs (nu, h, ell, coordinates in degrees) as exact numbers, so the library's own
rounding of the scaled lag s = sqrt(2 nu) h / ell and of the distances counts as ITS error.

(a) lags    per nu of NUS, ell of ELLS and scaled-lag target of `s_grid` (the lag itself is the float64
            h = s_grid * ell / sqrt(2 nu); h = 0 last):
              M        2^(1-nu) / Gamma(nu) s^nu K_nu(s), 1 at h = 0
              lnM      ln M
              D        2^(1-nu) / Gamma(nu) s^nu K_(nu-1)(s)            (0 stored at h = 0, where it is never read)
              dMdl     dM/d ell = (s / ell) D
              dMdnu    dM/d nu at fixed h, mp.diff
              dMdnu_st the library's formula (ck_matern_grad) evaluated exactly: the fourth-order central difference in the
                       order at the same s with step dnu = fl(CK_DNU_REL * nu), orders the doubles fl(nu + k dnu), minus
                       D s / (2 nu)
              omM      1 - M at the first N_SMALL (small) lags: the semivariogram without the cancellation
(b) Sigma   two cases of 70 + 58 sites (29 co-located across the processes) and 40 prediction sites (6 on data sites):
            "hav" on the 0.05-degree lattice with SET_R, "euc" on the unit square with SET_U -- Sigma (lower triangle) and c0
            of both processes with the nugget rules of oracle/cokrige_oracle.py (covariance / cross_covariance)
(c) grad    two cases of 24 + 16 sites (8 co-located): BIV under haversine, BIV_EUC under Euclid -- Sigma, z and the eleven
            dSigma/dtheta_k in MaternParams' flat order (lower triangles), the three nu slots twice: true and stencil
"""
import math
import os
import sys
import zipfile
from multiprocessing import Pool

import mpmath as mp
import numpy as np
from mpmath import mpf

HERE = os.path.dirname(os.path.abspath(__file__))
DPS = 40
CK_DNU_REL = 2e-3            # csrc/ck_math.h
EARTH_RADIUS_KM = 6371       # csrc/ck_math.h: CK_EARTH_RADIUS_KM
HAV, EUC = 0, 1

NUS_BOX = [0.2, 0.39, 0.4999999, 0.5, 0.5000001, 0.695, 0.75, 0.9986, 1.0, 1.000001, 1.3, 1.4999999, 1.5, 1.5000001, 2.0, 2.2,
           2.4999, 2.5, 3.0, 3.3, 3.4999, 3.499987, 3.5]      # inside MaternParams' default box
NUS_OUT = [0.05, 3.5000001, 4.0, 5.2, 10.0]                    # set_bounds / ck_set_model accept any nu > 0
NUS = NUS_BOX + NUS_OUT
ELLS = [1.0, 460.0]
N_SMALL = 40
S_GRID = np.concatenate([np.geomspace(1e-9, 2.0, N_SMALL), [np.nextafter(2.0, 0.0), np.nextafter(2.0, 3.0)],
                         np.linspace(2.0, 40.0, 24), np.geomspace(40.0, 745.0, 24), [0.0]])

SET_R = [0.988554, 0.813300, 0.390812, 3.499987, 0.998611, 446.350416, 499.967591, 468.516220, 0.0, 0.024783, -0.189985]
SET_U = [1.0, 1.0, 0.8, 1.3, 2.2, 0.25, 0.3, 0.2, 0.01, 0.0, 0.45]
BIV = [0.99, 0.81, 0.39, 0.75, 1.0, 460.0, 460.0, 460.0, 0.02, 0.025, -0.19]        # tests/dense_chains.py PARAMS
BIV_EUC = [0.99, 0.81, 0.7, 1.5, 2.2, 2.5, 2.5, 2.5, 0.02, 0.025, 0.3]


def lags_of(s_grid, nu, ell):
    """the float64 lags of one (nu, ell): plain IEEE multiply, square root and divide"""
    return s_grid * ell / np.sqrt(2.0 * nu)


# ---- the Matern family, every argument an mpf ----------------------------------------------------------------------------
def matern_x(nu, x):
    return mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(x, nu) * mp.besselk(nu, x)


def dlen_x(nu, x):
    return mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(x, nu) * mp.besselk(nu - 1, x)


def scaled(nu, h, ell):
    return mp.sqrt(2 * nu) * h / ell


def stencil_dnu(nu_f, s):
    """ck_matern_grad's nu-derivative in exact arithmetic; nu_f the float64 order, s the exact scaled lag"""
    d_f = CK_DNU_REL * nu_f
    f = [matern_x(mpf(nu_f + k * d_f), s) for k in (-2.0, -1.0, 1.0, 2.0)]
    nu = mpf(nu_f)
    return ((f[0] - f[3]) + 8 * (f[2] - f[1])) / (12 * mpf(d_f)) - dlen_x(nu, s) * s / (2 * nu)


def corr_all(nu_f, ell_f, h, dps=DPS):
    """(M, ln M, D, dM/d ell, dM/d nu true, dM/d nu stencil, 1 - M) as mpf at the exact lag h > 0 (an mpf)"""
    with mp.workdps(dps):
        nu, ell = mpf(nu_f), mpf(ell_f)
        s = scaled(nu, h, ell)
        M = matern_x(nu, s)
        D = dlen_x(nu, s)
        true = mp.diff(lambda v: matern_x(v, scaled(v, h, ell)), nu)
        return M, mp.log(M), D, s / ell * D, true, stencil_dnu(nu_f, s), 1 - M


def lag_entry(nu_f, ell_f, h_f, dps=DPS):
    """the seven float64 values of one lag of part (a)"""
    if h_f == 0.0:
        return (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with mp.workdps(dps):
        return tuple(float(v) for v in corr_all(nu_f, ell_f, mpf(h_f), dps))


# ---- distances from the float64 inputs ---------------------------------------------------------------------------------------
def prep_sites(c, metric):
    """haversine: radians are the float64 x * (pi / 180) first (numpy.radians; csrc: CK_DEG2RAD)"""
    c = np.asarray(c, dtype=np.float64)
    return c * (np.pi / 180.0) if metric == HAV else c


def dist_mp(a, b, metric):
    """exact distance of two prepared sites (float64 pairs); bit-identical sites give exactly 0"""
    a0, a1, b0, b1 = mpf(float(a[0])), mpf(float(a[1])), mpf(float(b[0])), mpf(float(b[1]))
    if metric == HAV:
        s0, s1 = mp.sin((a0 - b0) / 2), mp.sin((a1 - b1) / 2)
        return 2 * mp.asin(mp.sqrt(s0 * s0 + mp.cos(a0) * mp.cos(b0) * s1 * s1)) * EARTH_RADIUS_KM
    return mp.sqrt((a0 - b0) ** 2 + (a1 - b1) ** 2)


def block_params(params, i, j):
    """(nu, ell, amplitude as a function of mpf, nugget) of block (i, j), i <= j, from the flat parameters"""
    b = i + j
    sig = [mpf(params[0]), mpf(params[1])]
    amp = sig[i] * sig[i] if i == j else mpf(params[10]) * sig[0] * sig[1]
    return params[2 + b], params[5 + b], amp, (mpf(params[8 + i]) if i == j else mpf(0))


def cov_entry(params, i, j, a, b, metric, add_nugget, dps=DPS):
    """one float64 covariance entry: amp M(d) (+ the nugget where d == 0 in an auto block that takes it)"""
    with mp.workdps(dps):
        if i > j:
            i, j = j, i
        nu_f, ell_f, amp, nug = block_params(params, i, j)
        d = dist_mp(a, b, metric)
        if d == 0:
            return float(amp + nug if add_nugget else amp)
        nu = mpf(nu_f)
        return float(amp * matern_x(nu, scaled(nu, d, mpf(ell_f))))


def grad_entry(params, i, j, a, b, metric, dps=DPS):
    """one pair of a gradient case: float64 (Sigma, then the 11 derivatives, then the 3 stencil nu derivatives), i <= j"""
    with mp.workdps(dps):
        nu_f, ell_f, amp, nug = block_params(params, i, j)
        s1, s2, rho = mpf(params[0]), mpf(params[1]), mpf(params[10])
        d = dist_mp(a, b, metric)
        if d == 0:
            R, dl, dn, ds = mpf(1), mpf(0), mpf(0), mpf(0)
        else:
            R, _, _, dl, dn, ds, _ = corr_all(nu_f, ell_f, d, dps)
        out = [mpf(0)] * 15
        blk = i + j
        out[0] = amp * R + (nug if d == 0 else 0)
        if blk == 0:
            out[1] = 2 * s1 * R
            out[9] = mpf(1 if d == 0 else 0)
        elif blk == 2:
            out[2] = 2 * s2 * R
            out[10] = mpf(1 if d == 0 else 0)
        else:
            out[1], out[2], out[11] = rho * s2 * R, rho * s1 * R, s1 * s2 * R
        out[3 + blk] = amp * dn
        out[6 + blk] = amp * dl
        out[12 + blk] = amp * ds
        return tuple(float(v) for v in out)


def _task(t):
    return globals()[t[0]](*t[1:])


# ---- sites ---------------------------------------------------------------------------------------------------------------------
def sigma_sites(metric, seed):
    """70 + 58 sites, 29 co-located across the processes; 40 prediction sites, 6 of them on data sites"""
    rng = np.random.default_rng(seed)
    if metric == HAV:   # centres of 0.05-degree cells in a 3 x 4 degree patch: the nearest pairs are one cell (~5 km) apart
        idx = rng.choice(60 * 80, size=99, replace=False)
        pts = np.column_stack([35.0 + 0.025 + 0.05 * (idx // 80), -100.0 + 0.025 + 0.05 * (idx % 80)])
        free = np.column_stack([rng.uniform(35.0, 38.0, 34), rng.uniform(-100.0, -96.0, 34)])
    else:
        pts = rng.random((99, 2))
        free = rng.random((34, 2))
    c0 = pts[:70].copy()
    c1 = np.vstack([pts[41:70], pts[70:99]])
    pc = np.vstack([free[:5], c0[[3, 17, 30]], free[5:20], c0[[50, 69]], free[20:], c1[[40]]])
    return c0, c1, pc


def grad_sites(metric, seed):
    """24 + 16 sites, 8 co-located, spread like tests/dense_chains.py make_data"""
    rng = np.random.default_rng(seed)
    if metric == HAV:
        pts = np.column_stack([rng.uniform(25, 50, 32), rng.uniform(-120, -70, 32)])
    else:
        pts = np.column_stack([rng.uniform(0, 10, 32), rng.uniform(0, 10, 32)])
    return pts[:24].copy(), np.vstack([pts[16:24], pts[24:32]])


def pair_blocks(n0, n1):
    """(row, col, i, j) over the lower triangle of the stacked matrix; the block as (i <= j)"""
    for r in range(n0 + n1):
        for c in range(r + 1):
            yield r, c, int(c >= n0), int(r >= n0)


def mp_draw(S, seed):
    """z = L e with L the 40-digit Cholesky factor of S and e standard normal: a draw from the model, LAPACK-free"""
    e = np.random.default_rng(seed).standard_normal(S.shape[0])
    with mp.workdps(DPS):
        L = mp.cholesky(mp.matrix(S.tolist()))
        return np.array([float(v) for v in L * mp.matrix(e.tolist())])


def build(pool):
    out = dict(nus=np.array(NUS), n_box=np.array(len(NUS_BOX)), ells=np.array(ELLS), s_grid=S_GRID)
    # (a)
    tasks = [("lag_entry", nu, ell, float(h)) for nu in NUS for ell in ELLS for h in lags_of(S_GRID, nu, ell)]
    res = np.array(pool.map(_task, tasks, chunksize=8)).reshape(len(NUS), len(ELLS), len(S_GRID), 7)
    for k, name in enumerate(("M", "lnM", "D", "dMdl", "dMdnu", "dMdnu_st")):
        out[name] = np.ascontiguousarray(res[..., k])
    out["omM"] = np.ascontiguousarray(res[:, :, :N_SMALL, 6])
    # (b)
    for tag, metric, params, seed in (("hav", HAV, SET_R, 11), ("euc", EUC, SET_U, 12)):
        c0, c1, pc = sigma_sites(metric, seed)
        st = np.vstack([prep_sites(c0, metric), prep_sites(c1, metric)])
        pp = prep_sites(pc, metric)
        n0, N = len(c0), len(c0) + len(c1)
        pairs = list(pair_blocks(n0, len(c1)))
        vals = pool.map(_task, [("cov_entry", params, i, j, tuple(st[r]), tuple(st[c]), metric, True) for r, c, i, j in pairs],
                        chunksize=32)
        S = np.zeros((N, N))
        for (r, c, _, _), v in zip(pairs, vals):
            S[r, c] = v
        out.update({f"{tag}_params": np.array(params), f"{tag}_c0": c0, f"{tag}_c1": c1, f"{tag}_pc": pc, f"{tag}_S": S})
        for ip in (0, 1):   # c0 (N x m): the nugget only where the datum is of the predicted process
            t = [("cov_entry", params, ip, int(r >= n0), tuple(st[r]), tuple(pp[q]), metric, int(r >= n0) == ip)
                 for r in range(N) for q in range(len(pc))]
            out[f"{tag}_pcov{ip}"] = np.array(pool.map(_task, t, chunksize=32)).reshape(N, len(pc))
    # (c)
    for tag, metric, params, seed in (("ghav", HAV, BIV, 21), ("geuc", EUC, BIV_EUC, 22)):
        c0, c1 = grad_sites(metric, seed)
        st = np.vstack([prep_sites(c0, metric), prep_sites(c1, metric)])
        N = len(st)
        pairs = list(pair_blocks(len(c0), len(c1)))
        vals = pool.map(_task, [("grad_entry", params, i, j, tuple(st[c]), tuple(st[r]), metric) for r, c, i, j in pairs],
                        chunksize=8)
        A = np.zeros((15, N, N))
        for (r, c, _, _), v in zip(pairs, vals):
            A[:, r, c] = v
        S = A[0] + np.tril(A[0], -1).T
        out.update({f"{tag}_params": np.array(params), f"{tag}_c0": c0, f"{tag}_c1": c1, f"{tag}_S": A[0], f"{tag}_D": A[1:12],
                    f"{tag}_Dnu_st": A[12:15], f"{tag}_z": mp_draw(S, seed + 100)})
    return out


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        out = build(pool)
    path = os.path.join(HERE, "matern_mp.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:   # numpy.savez_compressed with a fixed
        for name, arr in out.items():                                                # time stamp: the same bytes every run
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(zi, "w") as f:
                np.lib.format.write_array(f, np.asarray(arr), allow_pickle=False)
    print(f"matern_mp: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    sys.exit(main())
