"""Host checks of tests/illcond_ref.py: the references themselves, and the conditions that keep tests/test_gpu_illcond.py from
being vacuous or unfair ("Stability of the inverse-based row solves").  No GPU.

  reference      chol_ld and the longdouble substitutions against mpmath (50 digits) at N = 40, in the backward-error bounds of
                 the longdouble format itself; blocks() as the device cuts them
  input strength LAPACK factors every set; cond_2 in [1e8, 1e11] and kappa_blk >= 1e4 on the hard sets, kappa_blk < 100 on WELL
  breakdown      the float64 emulation of the kernels' algorithm factors every set -- in the caller's order and in the library's
                 Hilbert order -- with a normwise backward error <= 0.1 / cond_2(Sigma): a correct kernel cannot report "not
                 positive definite" on these inputs
  gap            the emulation violates Higham's gamma_{N+1} |L||L^T| on NEARDUP and satisfies the block bound; LAPACK satisfies
                 Higham's everywhere; one correction step brings the emulation back under Higham's
  two levels     the same with the inverse built as potrf64_body builds it (illcond_ref.inverse_two_level): up to 150 times the
                 one-level error -- and what the MI355X then showed (tests/test_gpu_illcond.py) --, under the block bound, with a
                 normwise backward error of 0.065 / cond_2 at worst (NEARDUP in the Hilbert order), and cured by the same
                 correction step
Every figure is printed (pytest -s)."""
import numpy as np
import pytest

from tests import illcond_ref as ir

NAMES = list(ir.SETS)


def hilbert_perm(ds):
    """the stacked caller indices in the library's internal order with option site_order = 1: per process the stable sort by
    the Hilbert key on the bounding box of all sites (the restatement tests/test_gpu_joint.py checks the device against)"""
    from tests.test_gpu_joint import _hilbert_keys
    allc = np.vstack(ds.coords)
    lo, hi = allc.min(axis=0), allc.max(axis=0)
    out, off = [], 0
    for c in ds.coords:
        out.append(off + np.argsort(_hilbert_keys(c, lo, hi), kind="stable"))
        off += len(c)
    return np.concatenate(out)


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_blocks_as_the_device_cuts_them():
    b = ir.blocks(130, 126)
    assert [(s.start, s.stop) for s in b] == [(0, 64), (64, 128), (128, 130), (130, 194), (194, 256)]
    b = ir.blocks(513, 511)
    assert len(b) == 9 + 8 and (b[8].start, b[8].stop) == (512, 513) and (b[9].start, b[9].stop) == (513, 577)
    assert (b[-1].start, b[-1].stop) == (961, 1024)
    assert [(s.start, s.stop) for s in ir.blocks(65, 0)] == [(0, 64), (64, 65)]


def test_chol_ld_and_substitutions_against_mpmath():
    """at N = 40 on the worst conditioned set: backward errors measured in 50 digits, bounded by Higham's Theorems 10.3 and 8.5
    with the unit roundoff of the longdouble format"""
    import mpmath as mp
    mp.mp.dps = 50
    n = 40
    S = ir.data_set("NEARDUP").S[:n, :n]
    assert np.linalg.cond(S) > 1e6   # near-duplicates among the first 40 sites already
    L = ir.chol_ld(S)
    u_ld = float(np.finfo(np.longdouble).eps) / 2
    g = (n + 1) * u_ld / (1 - (n + 1) * u_ld)

    def to_mp(A):   # exact: a longdouble is the sum of two doubles
        A = np.atleast_2d(np.asarray(A, dtype=np.longdouble))
        hi = np.asarray(A, dtype=np.float64)
        lo = np.asarray(A - hi, dtype=np.float64)
        assert np.all(np.asarray(hi, dtype=np.longdouble) + np.asarray(lo, dtype=np.longdouble) == A)
        return mp.matrix([[mp.mpf(float(h)) + mp.mpf(float(l)) for h, l in zip(rh, rl)] for rh, rl in zip(hi, lo)])

    Lm, Sm = to_mp(L), to_mp(S)
    R = Sm - Lm * Lm.T
    A = to_mp(np.abs(np.asarray(L, dtype=np.float64)) @ np.abs(np.asarray(L, dtype=np.float64)).T)
    worst = max(abs(R[i, j]) / A[i, j] for i in range(n) for j in range(n))
    print(f"chol_ld N = 40: max |S - L L^T| / (|L||L^T|) = {float(worst):.2e}, gamma_41 (longdouble) = {g:.2e}")
    assert worst <= g
    # and close to mpmath's own factor: the forward error of a backward-stable factor, cond * gamma with a margin of ten
    Lmp = mp.cholesky(Sm)
    fwd = max(abs(Lm[i, j] - Lmp[i, j]) for i in range(n) for j in range(i + 1)) / max(abs(Lmp[i, i]) for i in range(n))
    print(f"   against mpmath.cholesky: {float(fwd):.2e}")
    assert fwd <= 10 * np.linalg.cond(S) * g
    b = np.random.default_rng(1).standard_normal(n)
    for trans in (False, True):
        x = ir.solve_lower_ld(L, b, trans=trans)
        xm, bm = to_mp(x).T, to_mp(b).T
        M = Lm.T if trans else Lm
        r = bm - M * xm
        sc = to_mp(np.abs(np.asarray(L.T if trans else L, dtype=np.float64)) @ np.abs(np.asarray(x, dtype=np.float64))).T
        worst = max(abs(r[i]) / sc[i] for i in range(n))
        print(f"   substitution (trans = {trans}): max |b - L x| / (|L||x|) = {float(worst):.2e}")
        assert worst <= g


@pytest.mark.parametrize("name", NAMES)
def test_input_strength(name):
    ds = ir.data_set(name)
    r = ds.ref
    np.linalg.cholesky(ds.S)   # LAPACK factors it
    print(f"{name}: N = {ds.N} cond_2 = {r.cond2:.2e} kappa_blk = {r.kappa_blk:.2e}")
    if name in ir.HARD:
        assert 1e8 <= r.cond2 <= 1e11
        assert r.kappa_blk >= 1e4
    if name == "WELL":
        assert r.kappa_blk < 100
    if name == "UNI65":   # one row solved against one block, and that block is a hard one
        assert r.kappa_blk >= 1e3 and len(r.blks) == 2


@pytest.mark.parametrize("order", ["caller", "hilbert"])
@pytest.mark.parametrize("name", NAMES)
def test_breakdown_margin(name, order):
    ds = ir.data_set(name)
    if order == "caller":
        ref = ds.ref
    else:
        perm = hilbert_perm(ds)
        assert not np.array_equal(perm, np.arange(ds.N)) and np.array_equal(np.sort(perm), np.arange(ds.N))
        ref = ir.Reference(ds.S[np.ix_(perm, perm)], ir.blocks(ds.n0, ds.n1))
        np.linalg.cholesky(ref.S)
    for two_level in (False, True):
        L = ir.emulate_inverse_blocked(ref.S, ref.blks, two_level=two_level)   # raises where a block does not factor
        comp, norm, _ = ir.factor_errors(ref, L)
        print(f"{name} ({order}'s order): kappa_blk = {ref.kappa_blk:.2e}; emulation ({'two' if two_level else 'one'}-level inverse): "
              f"normwise backward error {norm:.2e} against 0.1 / cond_2 = {0.1 / ref.cond2:.2e}; componentwise / (N u) = "
              f"{comp / (ds.N * ir.U):.3g}")
        assert norm <= 0.1 / ref.cond2   # 1 / cond_2 is the relative distance to a matrix that is not positive definite


@pytest.mark.parametrize("name", NAMES)
def test_gap_between_the_bounds(name):
    ds = ir.data_set(name)
    r = ds.ref
    higham, block = r.bound_b(False), r.bound_b()
    out = {}
    for label, L in (("LAPACK", np.linalg.cholesky(ds.S)), ("inverse-based", ir.emulate_inverse_blocked(ds.S, r.blks)),
                     ("inverse + one correction", ir.emulate_inverse_blocked(ds.S, r.blks, correct=True)),
                     ("two-level inverse", ir.emulate_inverse_blocked(ds.S, r.blks, two_level=True)),
                     ("two-level + one correction", ir.emulate_inverse_blocked(ds.S, r.blks, correct=True, two_level=True))):
        comp, norm, Ra = ir.factor_errors(r, L)
        out[label] = (comp / (ds.N * ir.U), float(np.max(Ra / higham)), float(np.max(Ra / block)))
        print(f"{name} {label}: comp. backward err / (N u) = {out[label][0]:.3g}, / Higham's bound = {out[label][1]:.3g}, "
              f"/ block bound = {out[label][2]:.3g}, normwise {norm:.2e}")
    assert out["LAPACK"][1] <= 1.0
    assert out["inverse + one correction"][1] <= 1.0
    assert out["inverse-based"][2] <= 4e-3   # a correct inverse-based factorisation sits this far below the block bound
    assert out["two-level inverse"][2] <= 1.0   # what the device's inverse adds stays under it too
    if name == "NEARDUP":
        assert out["inverse-based"][1] > 1.0
    if name == "WELL":   # the block bound is Higham's to within 1 + kappa_blk
        assert 1.0 + r.kappa_blk < 100
