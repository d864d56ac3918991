"""The pure planning of the dense likelihood family, without a GPU: the device-memory admission (ck_host_mem_admit), the plan of
ck_loglik_fisher's operands and product groups (ck_host_fisher_plan) and the REML gradient's start vectors (ck_host_reml_start)
of csrc/ck_host.cpp, compiled with g++ (tests/host_lik_plan_shim.cpp) against a restatement in Python / numpy, plus the same
functions in a stand-alone program under -fsanitize=address,undefined (tests/host_lik_plan_sanitize_main.cpp)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
NB, TAIL, NO = 512, 8 * 64 * 64, 13
I64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("likplan") / "libck_host_lik_plan.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_lik_plan_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.shim_tri_bytes.argtypes = lib.shim_schur_bytes.argtypes = [ctypes.c_int64]
    lib.shim_tri_bytes.restype = lib.shim_schur_bytes.restype = ctypes.c_int64
    lib.shim_mem_admit.argtypes = [I64, I64, I64]
    lib.shim_mem_admit.restype = None
    lib.shim_fisher_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte),
                                     ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, I64, I64, I64, I64,
                                     ctypes.POINTER(ctypes.c_int32)]
    lib.shim_fisher_plan.restype = ctypes.c_int
    lib.shim_reml_start.argtypes = [ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp]
    lib.shim_reml_start.restype = None
    return lib


def _i64(a):
    return a.ctypes.data_as(I64)


# ---- the admission ----------------------------------------------------------------------------------------------------------
def tri_bytes(M):
    return sum(((M - K * NB) * NB + TAIL) * 8 for K in range(M // NB))


def schur_bytes(M):
    return tri_bytes(M) + 8 * M * 8 if M > 0 else 0


def admit_ref(free, arena, asize, aused, rhs, order, slab, a_rhs, a_order, a_slab, a_extra):
    """the rule, restated: a buffer that does not grow adds nothing to either side; an arena's rows never count against free memory"""
    need, avail, short = a_extra, free, False
    if a_rhs > rhs:
        if arena:
            short = a_rhs > asize - aused
        else:
            need, avail = need + a_rhs, avail + rhs
    if a_order > 0 and a_order != order:
        need, avail = need + schur_bytes(a_order), avail + schur_bytes(order)
    if a_slab > slab:
        need, avail = need + a_slab, avail + slab
    return need, avail, short


def admit(shim, st, ask):
    out = np.zeros(3, dtype=np.int64)
    shim.shim_mem_admit(_i64(np.array(st, dtype=np.int64)), _i64(np.array(ask, dtype=np.int64)), _i64(out))
    return int(out[0]), int(out[1]), bool(out[2])


def test_triangle_and_schur_bytes(shim):
    for M in (512, 1024, 1536, 5120, 65536):
        assert shim.shim_tri_bytes(M) == tri_bytes(M)
        assert shim.shim_schur_bytes(M) == tri_bytes(M) + 64 * M
    assert shim.shim_schur_bytes(0) == 0 and shim.shim_tri_bytes(0) == 0


def test_admission_every_combination(shim):
    free, held_rhs, held_slab, M = 10 << 30, 3 << 20, 5 << 20, 2048
    arenas = {"none": (0, 0, 0), "room": (1, 64 << 20, 8 << 20), "short": (1, 64 << 20, 62 << 20)}
    rhs_asks = {"grow": 4 << 20, "fit": 3 << 20}
    schurs = {"none": (M, 0), "same": (M, M), "other": (1024, M), "first": (0, M)}   # (held order, asked order)
    slab_asks = {"grow": 6 << 20, "fit": 5 << 20}
    n = 0
    for (ka, ar), (kr, rq), (ks, (ho, ao)), (kl, sq) in itertools.product(arenas.items(), rhs_asks.items(), schurs.items(),
                                                                         slab_asks.items()):
        st = (free, *ar, held_rhs, ho, held_slab)
        ask = (rq, ao, sq, 12345)
        got, ref = admit(shim, st, ask), admit_ref(*st, *ask)
        assert got == ref, (ka, kr, ks, kl, got, ref)
        need, avail, short = got
        assert short == (ka == "short" and kr == "grow")
        want_need = 12345 + (rq if kr == "grow" and ka == "none" else 0) + (schur_bytes(M) if ks in ("other", "first") else 0) + \
            (sq if kl == "grow" else 0)
        want_avail = free + (held_rhs if kr == "grow" and ka == "none" else 0) + (schur_bytes(1024) if ks == "other" else 0) + \
            (held_slab if kl == "grow" else 0)
        assert (need, avail) == (want_need, want_avail), (ka, kr, ks, kl)
        n += 1
    assert n == 48


def test_admission_outcome_changes_are_pinned(shim):
    """the three places where the one rule decides otherwise than the call sites it replaced did"""
    M, rows = 2048, 100 << 20
    # 1. right-hand sides that do not grow are not credited: the gradient's call used to add the held buffer to what is available
    need, avail, _ = admit(shim, (1 << 20, 0, 0, 0, rows, 0, 0), (rows, M, 0, 0))
    assert avail == 1 << 20 and need == schur_bytes(M) and need > avail      # refused up front (before: 101 MiB "available")
    # 2. an arena's rows never count against free memory
    need, avail, short = admit(shim, (1 << 20, 1, 1 << 30, 0, 0, M, 0), (rows, M, 0, 0))
    assert (need, avail, short) == (0, 1 << 20, False)                        # admitted (before: 100 MiB against 1 MiB free)
    # 3. the Schur buffers count with their site arrays, asked and released
    need, avail, _ = admit(shim, (0, 0, 0, 0, rows, 1024, 0), (rows, M, 0, 0))
    assert need == tri_bytes(M) + 64 * M and avail == tri_bytes(1024) + 64 * 1024


# ---- the Fisher plan ------------------------------------------------------------------------------------------------------
def plan(shim, n_procs, Npad, n0p, op_live, room, p=0, ngr=7, cap=0):
    geom, bd, scal = np.zeros(12, dtype=np.int64), np.zeros(NO, dtype=np.int64), np.zeros(7, dtype=np.int64)
    units, gof = np.zeros(4 * 14, dtype=np.int64), np.zeros(NO, dtype=np.int32)
    live = np.array(op_live, dtype=np.uint8)
    rc = shim.shim_fisher_plan(n_procs, Npad, n0p, Npad // NB, live.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), room, p, ngr, cap,
                               _i64(geom), _i64(bd), _i64(scal), _i64(units), gof.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    keys = ("d_total", "b_total", "b_max", "fixed_bytes", "region", "n_units", "n_groups")
    out = dict(zip(keys, (int(x) for x in scal)))
    out.update(rc=rc, geom=geom.reshape(6, 2), b=bd, group_of=gof, units=units[:4 * out["n_units"]].reshape(-1, 4))
    return out


def plan_ref(n_procs, Npad, n0p, op_live, p, ngr):
    """geometry, operand and product doubles and the fixed bytes, restated"""
    nK = Npad // NB
    c0, wpad, nlo, nhi, pK0, npan = [0, 0], [Npad, 0], [0, 0], [Npad, 0], [0, 0], [nK, 0]
    if n_procs == 2:
        wpad[0], nhi[0], npan[0] = -(-n0p // 128) * 128, n0p, -(-n0p // NB)
        c0[1] = n0p // 128 * 128
        wpad[1], nlo[1], nhi[1], pK0[1] = Npad - c0[1], n0p, Npad, n0p // NB
        npan[1] = nK - pK0[1]
    units, b = [], [0] * NO
    for a in range(11):
        if not op_live[a]:
            continue
        if a < 8:
            r = a // 4
            units.append((a, r, r, npan[r] * wpad[r] * NB))
            b[a] = Npad * wpad[r]
        else:
            units += [(a, 0, 1, npan[1] * wpad[0] * NB), (a, 1, 0, npan[0] * wpad[1] * NB)]
            b[a] = Npad * Npad
    d_total = sum(u[3] for u in units)
    thin = nK * 256 * NB + Npad * 256 + Npad * p + 256 * (256 + p) if p > 0 else 0
    fixed = (Npad * Npad + d_total + thin + ngr * 91 + 2 * Npad) * 8 + (1 << 20)
    return np.array([c0, wpad, nlo, nhi, pK0, npan]), units, b, d_total, fixed


ALL2 = [1] * NO
ALL1 = [1, 1, 1, 1] + [0] * 7 + [1, 0]
SHAPES = [(1, 1024, 1024, ALL1), (1, 1536, 1536, ALL1), (2, 1024, 384, ALL2), (2, 1024, 333, ALL2), (2, 2048, 1024, ALL2),
          (2, 2048, 700, ALL2)]   # one and two processes; n0p a multiple of 128 and not, on a panel edge and not


@pytest.mark.parametrize("n_procs,Npad,n0p,live", SHAPES)
@pytest.mark.parametrize("p", [0, 2])
def test_fisher_plan_everything_fits(shim, n_procs, Npad, n0p, live, p):
    geom, units, b, d_total, fixed = plan_ref(n_procs, Npad, n0p, live, p, 7)
    P = plan(shim, n_procs, Npad, n0p, live, fixed + 8 * sum(b), p)      # exactly enough
    assert P["rc"] == 0 and np.array_equal(P["geom"], geom) and list(P["b"]) == b
    assert [tuple(u) for u in P["units"]] == units and P["d_total"] == d_total and P["fixed_bytes"] == fixed
    assert P["b_total"] == sum(b) == P["region"] and P["b_max"] == max(b) and P["n_groups"] == 1
    assert [int(g) for g in P["group_of"]] == [0 if live[a] and a < 11 else -1 for a in range(NO)]
    if n_procs == 2:
        assert P["geom"][0][1] == n0p // 128 * 128 <= n0p and P["geom"][0][1] + P["geom"][1][1] == Npad   # c0[1] rounds DOWN


@pytest.mark.parametrize("n_procs,Npad,n0p,live", SHAPES)
def test_fisher_plan_several_groups(shim, n_procs, Npad, n0p, live):
    _, _, b, _, fixed = plan_ref(n_procs, Npad, n0p, live, 0, 7)
    for room in (16 * max(b), 16 * max(b) + 8 * min(x for x in b if x), 8 * sum(b) - 8):   # two of the largest ... just not all
        P = plan(shim, n_procs, Npad, n0p, live, fixed + room)
        assert P["rc"] == 0 and P["n_groups"] > 1
        sums = [sum(b[a] for a in range(NO) if P["group_of"][a] == g) for g in range(P["n_groups"])]
        assert all(P["group_of"][a] >= 0 for a in range(11) if live[a])       # every live operand in exactly one group (-2: twice)
        assert all(P["group_of"][a] == -1 for a in range(NO) if not live[a] or a >= 11)
        assert all(0 < s <= room // 16 for s in sums) and P["region"] == max(sums)
        order = [int(P["group_of"][a]) for a in range(11) if live[a]]
        assert order == sorted(order)                                          # operands in order, groups consecutive


@pytest.mark.parametrize("n_procs,Npad,n0p,live", SHAPES)
def test_fisher_plan_refusal_and_caps(shim, n_procs, Npad, n0p, live):
    _, units, b, d_total, fixed = plan_ref(n_procs, Npad, n0p, live, 2, 7)
    for room in (fixed + 16 * max(b) - 1, fixed - 1, 0, -(1 << 30)):            # below two of the largest product; below the fixed part
        P = plan(shim, n_procs, Npad, n0p, live, room, p=2)
        assert P["rc"] == 1 and P["n_groups"] == 0
        assert (P["fixed_bytes"], P["d_total"], P["b_max"], P["n_units"]) == (fixed, d_total, max(b), len(units))   # the message's amounts
    big = fixed + (1 << 40)
    assert plan(shim, n_procs, Npad, n0p, live, big, p=2, cap=8 * sum(b))["n_groups"] == 1          # a cap that holds everything
    P = plan(shim, n_procs, Npad, n0p, live, big, p=2, cap=16 * max(b))                            # ... two of the largest
    assert P["rc"] == 0 and P["n_groups"] > 1 and P["region"] <= max(b) * 1
    assert plan(shim, n_procs, Npad, n0p, live, big, p=2, cap=16 * max(b) - 1)["rc"] == 1           # ... less: refused
    assert plan(shim, n_procs, Npad, n0p, live, fixed - 1, p=2, cap=1 << 40)["rc"] == 1            # a cap never adds room


@pytest.mark.parametrize("n_procs,Npad,n0p", [(1, 1024, 1024), (2, 1024, 333)])
def test_fisher_plan_diagonal_operands_only(shim, n_procs, Npad, n0p):
    live = [0] * 11 + [1, 1 if n_procs == 2 else 0]
    for room in (1 << 40, 0, -5):
        P = plan(shim, n_procs, Npad, n0p, live, room)
        assert P["rc"] == (0 if room >= P["fixed_bytes"] else 1)
        assert P["n_units"] == 0 and P["d_total"] == P["b_total"] == P["b_max"] == P["region"] == 0
        assert all(g == -1 for g in P["group_of"]) and P["n_groups"] == (1 if P["rc"] == 0 else 0)


# ---- the REML start vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 16])
def test_reml_start_against_numpy(shim, p):
    rng = np.random.default_rng(p)
    Npad, n, q = 64, 51, 1 + p
    W = rng.standard_normal((q + Npad, q + 1))
    W[q + n:, 1:] = 0.0                      # padding positions: alpha = 0, B = 0
    W[q + n:, 0] = 1.0
    X = rng.standard_normal((3 * p, p))
    R = np.linalg.cholesky(X.T @ X)
    beta = rng.standard_normal(p)
    av = np.full((q, Npad), np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    shim.shim_reml_start(p, Npad, W.ctypes.data_as(dp), beta.ctypes.data_as(dp), np.ascontiguousarray(R).ctypes.data_as(dp),
                         av.ctypes.data_as(dp))
    alpha, B = W[q:, 1], W[q:, 2:]
    assert np.allclose(av[0], alpha - B @ beta, rtol=1e-13, atol=1e-13)
    assert np.allclose(av[1:], np.linalg.solve(R, B.T), rtol=1e-11, atol=1e-12)
    assert np.all(av[:, n:] == 0.0) and not np.isnan(av).any()   # padding passes through: zeros in, zeros out


def test_planning_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_lik_plan_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_lik_plan_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
