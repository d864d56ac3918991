"""Host arithmetic of the dense predictors, without a GPU: csrc/ck_host.cpp's ck_host_block_members, ck_host_prior_pieces,
ck_host_block_chunk, ck_host_draw_chunk, ck_host_coincident_site and ck_host_universal_finish compiled for the host with g++
(tests/host_dense_predict_shim.cpp) against numpy restatements of the expressions ck_api.hip had inline, plus the same functions
in a stand-alone program under -fsanitize=address,undefined (tests/host_dense_predict_sanitize_main.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
CK_PRIOR_PIECE = 512
CK_AUX_ALIGN = 256
OK, LABEL, EMPTY = 0, 1, 2
LL = ctypes.c_longlong


def test_host_constants_are_the_kernels():
    import re
    internal = open(os.path.join(CSRC, "ck_internal.h")).read()
    assert int(re.search(r"#define CK_PRIOR_PIECE (\d+)", internal).group(1)) == CK_PRIOR_PIECE
    assert int(re.search(r"#define CK_AUX_ALIGN (\d+)", internal).group(1)) == CK_AUX_ALIGN


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dense") / "libck_host_dense_predict.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_dense_predict_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for name in ("shim_prior_pieces", "shim_block_chunk", "shim_draw_chunk", "shim_coincident_site"):
        getattr(lib, name).restype = LL
    lib.shim_err_of.restype = ctypes.c_double
    lib.shim_err_of.argtypes = [ctypes.c_double]
    lib.shim_universal_finish.restype = None
    return lib


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))


# ---- block members -------------------------------------------------------------------------------------------------------
def members(lib, block, r):
    """-> (code, off, member, q_max, at)"""
    block = np.ascontiguousarray(block, dtype=np.int32)
    off, mem, out = np.full(r + 1, -7, np.int32), np.full(len(block), -7, np.int64), np.zeros(2, np.int64)
    rc = lib.shim_block_members(_ptr(block, ctypes.c_int), LL(len(block)), r, _ptr(off, ctypes.c_int), _ptr(mem, LL), _ptr(out, LL))
    return rc, off, mem, int(out[0]), int(out[1])


def members_numpy(block, r):
    """stable grouping by label: argsort(kind='stable') IS the counting sort's order"""
    block = np.asarray(block)
    return np.concatenate([[0], np.cumsum(np.bincount(block, minlength=r))]), np.argsort(block, kind="stable")


def test_block_members_smallest_and_interleaved(shim):
    rc, off, mem, q_max, _ = members(shim, [0], 1)
    assert rc == OK and off.tolist() == [0, 1] and mem.tolist() == [0] and q_max == 1
    block = [2, 0, 1, 0, 2, 2, 1, 0, 2]   # interleaved: stability shows
    rc, off, mem, q_max, _ = members(shim, block, 3)
    woff, wmem = members_numpy(block, 3)
    assert rc == OK and np.array_equal(off, woff) and np.array_equal(mem, wmem) and q_max == 4
    assert mem.tolist() == [1, 3, 7, 2, 6, 0, 4, 5, 8]


def test_block_members_faults(shim):
    rc, _, _, _, at = members(shim, [0, 1, 3, 1, -1], 3)   # a label equal to r in front of a label of -1
    assert rc == LABEL and at == 2
    rc, _, _, _, at = members(shim, [0, -1, 3], 3)
    assert rc == LABEL and at == 1
    rc, off, mem, q_max, at = members(shim, [2, 0, 2, 0, 0], 3)   # the middle block is empty: the outputs are complete
    assert rc == EMPTY and at == 1 and off.tolist() == [0, 3, 3, 5] and mem.tolist() == [1, 3, 4, 0, 2] and q_max == 3
    rc, _, _, _, at = members(shim, [3, 3], 4)   # the first empty block is named
    assert rc == EMPTY and at == 0


def test_block_members_whole_call_and_chunks_of_two_agree(shim):
    """ck_predict_blocks groups the whole call for the prior and every chunk for the fold kernel, a chunk's rows through the
    inverse of the chunk's site permutation: per block, the chunks' members in the caller's order are the whole call's"""
    rng = np.random.default_rng(3)
    block = np.array([1, 0, 2, 2, 0, 1, 0, 2, 1], dtype=np.int32)
    r, m = 3, len(block)
    rc, off, mem, _, _ = members(shim, block, r)
    assert rc == OK
    whole = [mem[off[b]:off[b + 1]].tolist() for b in range(r)]
    got = [[] for _ in range(r)]
    for a0 in range(0, m, 2):
        mc = min(2, m - a0)
        pperm = rng.permutation(mc)              # row j of the chunk holds the chunk's site pperm[j]
        inv = np.empty(mc, np.int64)
        inv[pperm] = np.arange(mc)
        rc, coff, cmem, _, _ = members(shim, block[a0:a0 + mc], r)
        assert rc in (OK, EMPTY)                 # a chunk need not meet every block
        crows = inv[cmem]
        for b in range(r):
            got[b] += [a0 + int(pperm[row]) for row in crows[coff[b]:coff[b + 1]]]
    assert got == whole


# ---- prior pieces --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [0, 1])
def test_prior_pieces(shim, full):
    """blocks of 1, CK_PRIOR_PIECE and CK_PRIOR_PIECE + 1 sites, and elements of exactly 1, CK_PRIOR_PIECE and CK_PRIOR_PIECE + 1
    pairs: 1 x 512, 16 x 32 and 1 x 513, 19 x 27 in the full form; the diagonal form has n^2 pairs, 22^2 = 484 below a piece
    and 23^2 = 529 above it"""
    sizes = [1, 1, CK_PRIOR_PIECE, CK_PRIOR_PIECE + 1, 16, 32, 19, 27, 22, 23]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    r = len(sizes)
    pairs = [sizes[R] * sizes[C] for R in range(r) for C in range(R + 1)] if full else [n * n for n in sizes]
    poff = np.full(len(pairs) + 1, -7, np.int64)
    total = shim.shim_prior_pieces(_ptr(off, ctypes.c_int), r, full, _ptr(poff, LL))
    want = [-(-x // CK_PRIOR_PIECE) for x in pairs]
    assert poff[0] == 0 and np.array_equal(np.diff(poff), want) and np.all(np.diff(poff) >= 1) and poff[-1] == total == sum(want)
    pieces = dict(zip(pairs, np.diff(poff).tolist()))
    if full:
        assert [pieces[x] for x in (1, CK_PRIOR_PIECE, CK_PRIOR_PIECE + 1)] == [1, 1, 2]
        assert want[3 * 4 // 2 + 2] == CK_PRIOR_PIECE + 1   # R = 3, C = 2: 513 x 512 pairs
    else:
        assert [pieces[x] for x in (1, 484, 529, CK_PRIOR_PIECE ** 2, (CK_PRIOR_PIECE + 1) ** 2)] == [1, 1, 2, 512, 515]


# ---- chunk rules ---------------------------------------------------------------------------------------------------------
def block_chunk_numpy(option, free_bytes, arena, arena_rest, held_bytes, Npad, m):
    chunk = option
    if chunk <= 0:
        avail = arena_rest if arena else free_bytes // 2
        avail = max(avail, held_bytes) if arena else avail + held_bytes
        chunk = max(avail // (8 * Npad) - CK_AUX_ALIGN, CK_AUX_ALIGN)
    return min(chunk, m)


def draw_chunk_numpy(option, free_bytes, Mp, m, noise, n_draws):
    chunk = option
    if chunk <= 0:
        chunk = (free_bytes // 2) // (8 * (Mp + (2 if noise else 1) * m)) // 128 * 128
        chunk = max(128, min(chunk, 8192))
    return min(chunk, n_draws)


def test_block_chunk(shim):
    G = 1 << 30
    seen = set()
    for option in (0, -1, 100, 10 ** 7):                      # not set, set, set above m
        for arena, rest in ((False, 0), (True, 0), (True, 3 * G), (True, 40 * G)):
            for free in (0, 1000, 5 * G, 200 * G):            # the floor applies ... plenty
                for held in (0, 2 * G):
                    for Npad, m in ((1024, 10 ** 6), (40960, 5000), (512, 3)):
                        want = block_chunk_numpy(option, free, arena, rest, held, Npad, m)
                        got = shim.shim_block_chunk(LL(option), LL(free), LL(rest if arena else -1), LL(held), LL(Npad), LL(m))
                        assert got == want, (option, arena, rest, free, held, Npad, m)
                        seen.add(want)
    assert CK_AUX_ALIGN in seen and 100 in seen and 3 in seen and 10 ** 6 in seen
    assert shim.shim_block_chunk(LL(0), LL(0), LL(-1), LL(0), LL(1024), LL(10 ** 6)) == CK_AUX_ALIGN


def test_draw_chunk(shim):
    G = 1 << 30
    seen = set()
    for option in (0, -5, 100, 10 ** 6):
        for free in (0, 4096, G, 250 * G):
            for Mp, m in ((512, 1), (512, 300), (65536, 65536)):
                for noise in (False, True):
                    for n_draws in (1, 100, 1000, 10 ** 5):
                        want = draw_chunk_numpy(option, free, Mp, m, noise, n_draws)
                        got = shim.shim_draw_chunk(LL(option), LL(free), LL(Mp), LL(m), int(noise), LL(n_draws))
                        assert got == want, (option, free, Mp, m, noise, n_draws)
                        seen.add(want)
    assert {128, 8192, 100, 1, 1000} <= seen
    # the caller's noise takes a second copy: fewer draws fit the same memory
    assert shim.shim_draw_chunk(LL(0), LL(2 * G), LL(65536), LL(65536), 1, LL(10 ** 5)) < \
        shim.shim_draw_chunk(LL(0), LL(2 * G), LL(65536), LL(65536), 0, LL(10 ** 5))


# ---- coincident sites ----------------------------------------------------------------------------------------------------
def coincident(lib, xy, cmap, mask):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    cmap = np.ascontiguousarray(cmap, dtype=np.int32)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    return lib.shim_coincident_site(_ptr(xy, ctypes.c_double), _ptr(cmap, ctypes.c_int), _ptr(mask, ctypes.c_ubyte), LL(len(cmap)))


def coincident_numpy(xy, cmap, mask):
    """the smallest internal position whose site repeats the coordinates of an earlier live position"""
    live = [j for j in range(len(cmap)) if not mask[j]]
    for k, j in enumerate(live):
        if any(tuple(xy[cmap[j]]) == tuple(xy[cmap[u]]) for u in live[:k]):
            return j
    return -1


def test_coincident_site(shim):
    rng = np.random.default_rng(5)
    m = 12
    xy = rng.uniform(0, 1, (m, 2))
    cmap = rng.permutation(m)
    none = np.zeros(m, np.uint8)
    assert coincident(shim, xy, cmap, none) == coincident_numpy(xy, cmap, none) == -1
    one = xy.copy()
    one[cmap[9]] = one[cmap[4]]                       # internal positions 4 and 9
    assert coincident(shim, one, cmap, none) == coincident_numpy(one, cmap, none) == 9
    two = one.copy()
    two[cmap[6]] = two[cmap[1]]                       # and 1 and 6: the smaller of the later indices wins
    assert coincident(shim, two, cmap, none) == coincident_numpy(two, cmap, none) == 6
    defl = none.copy()
    defl[1] = 1                                       # a pair with one member deflated is not reported
    assert coincident(shim, two, cmap, defl) == coincident_numpy(two, cmap, defl) == 9
    defl[9] = 1
    assert coincident(shim, two, cmap, defl) == -1
    half = one.copy()
    half[cmap[9], 1] += 1e-9                          # one coordinate equal is no coincidence
    assert coincident(shim, half, cmap, none) == -1
    assert coincident(shim, xy[:1], [0], [0]) == -1   # m = 1


# ---- the universal epilogue ----------------------------------------------------------------------------------------------
def finish(lib, W, beta, Ai, f0, pperm, c0, m, p, pi, offi):
    pred, err = np.full(m, np.nan), np.full(m, np.nan)
    d = ctypes.c_double
    lib.shim_universal_finish(_ptr(W, d), _ptr(beta, d), _ptr(Ai, d), _ptr(f0, d), _ptr(pperm, LL), d(c0), LL(m), p, pi, offi,
                              _ptr(pred, d), _ptr(err, d))
    return pred, err


def finish_numpy(W, beta, Ai, f0, pperm, c0, m, p, pi, offi, order=None):
    """float64; order: a permutation of the p trend columns in which every sum over them is taken"""
    order = np.arange(p) if order is None else order
    pred, err = np.empty(m), np.empty(m)
    for s in range(m):
        c = s if pperm is None else pperm[s]
        r = -W[s, 2:].copy()
        if pi:
            r[offi:offi + pi] += f0[c]
        pr, var = W[s, 1], c0 - W[s, 0]
        for j in order:
            pr += r[j] * beta[j]
            t = 0.0
            for l in order:
                t += Ai[j, l] * r[l]
            var += r[j] * t
        pred[c] = pr
        err[c] = np.sqrt(var) if var >= 0 else 0.0
    return pred, err


@pytest.mark.parametrize("p,pi,offi", [(1, 1, 0), (4, 2, 2), (4, 0, 4), (4, 3, 0)])
@pytest.mark.parametrize("permuted", [False, True])
def test_universal_finish(shim, p, pi, offi, permuted):
    """Tolerance: the restatement in the library's own order of summation against the same restatement with the sums over the
    trend columns reversed and rotated, on these inputs -- what float64 itself leaves open (measured here: 0 for p = 1, up to
    8.9e-16 in pred and 1.8e-15 in pred_err for p = 4, values of order 1 .. 10) -- with one ulp of the largest value as the
    floor where reordering changes nothing."""
    rng = np.random.default_rng(100 * p + 10 * pi + permuted)
    m = 9
    W = np.ascontiguousarray(rng.uniform(0.1, 1.0, (m, p + 2)))
    W[:, 0] = rng.uniform(0.0, 0.3, m)
    B = rng.standard_normal((p, p))
    Ai = np.ascontiguousarray(B @ B.T + np.eye(p))
    beta = rng.standard_normal(p)
    f0 = np.ascontiguousarray(rng.standard_normal((m, pi))) if pi else None
    pperm = rng.permutation(m).astype(np.int64) if permuted else None
    c0 = 1.25
    W[3, 0] = c0 + 1e3                                # one site whose variance is negative: 0.0
    args = (W, beta, Ai, f0, pperm, c0, m, p, pi, offi)
    pred, err = finish(shim, *args)
    want_pred, want_err = finish_numpy(*args)
    spread_p = spread_e = 0.0
    for order in (np.arange(p)[::-1], np.roll(np.arange(p), 1), np.roll(np.arange(p)[::-1], 1)):
        vp, ve = finish_numpy(*args, order=order)
        spread_p = max(spread_p, np.max(np.abs(vp - want_pred)))
        spread_e = max(spread_e, np.max(np.abs(ve - want_err)))
    tol_p = max(spread_p, np.spacing(np.max(np.abs(want_pred))))
    tol_e = max(spread_e, np.spacing(np.max(want_err)))
    print(f"p={p} pi={pi} permuted={permuted}: reordering spread pred {spread_p:.2e} err {spread_e:.2e}; "
          f"library - numpy pred {np.max(np.abs(pred - want_pred)):.2e} err {np.max(np.abs(err - want_err)):.2e}")
    assert np.max(np.abs(pred - want_pred)) <= tol_p and np.max(np.abs(err - want_err)) <= tol_e
    site = 3 if pperm is None else pperm[3]
    assert err[site] == 0.0 and np.all(err[np.arange(m) != site] > 0.0) and not np.any(np.isnan(pred))


def test_err_of(shim):
    assert shim.shim_err_of(4.0) == 2.0 and shim.shim_err_of(0.0) == 0.0 and shim.shim_err_of(-1e-30) == 0.0
    assert shim.shim_err_of(float("nan")) == 0.0 and shim.shim_err_of(float("inf")) == float("inf")


# ---- sanitizers ----------------------------------------------------------------------------------------------------------
def test_dense_predict_host_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_dense_predict_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_dense_predict_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
