"""The member layout of block cokriging in the neighbourhood without a GPU (csrc/ck_host.cpp: ck_host_local_block_layout):
CSR offsets, the stable grouping, the grouped and padded coordinate rows and weights, compiled for the host with g++
(tests/host_local_blocks_shim.cpp) and checked against a restatement in numpy; every refusal with the offender it names; the
same function in a stand-alone program under -fsanitize=address,undefined (tests/host_local_blocks_sanitize_main.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("local_blocks") / "libck_host_local_blocks.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "host_local_blocks_shim.cpp"),
                    os.path.join(CSRC, "ck_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def layout(lib, centres, pc, lab, w, pad=64, r=None):
    """-> dict, or the refusal's text"""
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 2)
    pc = np.ascontiguousarray(pc, dtype=np.float64).reshape(-1, 2)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    r = len(centres) if r is None else r
    m = len(lab)
    mpad = (m + pad - 1) // pad * pad
    sc, off, perm = np.zeros(2, np.int64), np.full(max(r, 0) + 1, -1, np.int32), np.full(m, -1, np.int64)
    xy, ww = np.full((mpad, 2), np.nan), np.full(mpad, np.nan)
    err = ctypes.create_string_buffer(512)
    dp, ll = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)
    rc = lib.shim_local_block_layout(centres.ctypes.data_as(dp), r, pc.ctypes.data_as(dp), ctypes.c_longlong(m),
                                     lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), w.ctypes.data_as(dp), pad,
                                     sc.ctypes.data_as(ll), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), perm.ctypes.data_as(ll),
                                     xy.ctypes.data_as(dp), ww.ctypes.data_as(dp), err, 512)
    if rc != 0:
        return err.value.decode()
    return dict(mpad=int(sc[0]), q_max=int(sc[1]), off=off, perm=perm, xy=xy, w=ww)


def check(lib, r, lab, pad=64, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.asarray(lab)
    m = len(lab)
    centres = rng.uniform(-60, 60, (r, 2))
    pc, w = rng.uniform(-60, 60, (m, 2)), rng.uniform(-1, 2, m)
    L = layout(lib, centres, pc, lab, w, pad)
    assert isinstance(L, dict), L
    perm = np.argsort(lab, kind="stable")                  # the caller's order kept inside a block
    cnt = np.bincount(lab, minlength=r)
    assert np.array_equal(L["off"], np.concatenate([[0], np.cumsum(cnt)]))
    assert np.array_equal(L["perm"], perm)
    assert L["mpad"] == (m + pad - 1) // pad * pad and L["q_max"] == cnt.max()
    assert np.array_equal(L["xy"][:m], pc[perm]) and np.array_equal(L["w"][:m], w[perm])
    assert np.all(L["xy"][m:] == 0.0) and np.all(L["w"][m:] == 0.0)
    return L


def test_layout_against_numpy(shim):
    rng = np.random.default_rng(1)
    for r, m, pad in ((37, 1000, 64), (200, 5000, 64), (5, 129, 256), (64, 4096, 64), (3, 3, 1)):
        lab = np.concatenate([np.arange(r), rng.integers(0, r, m - r)])   # random labels, every block hit
        check(shim, r, lab[rng.permutation(m)], pad, seed=m)


def test_layout_edges(shim):
    check(shim, 1, np.zeros(300, int))                                    # all sites in one block, r = 1
    check(shim, 1, np.zeros(1, int))
    L = check(shim, 129, np.random.default_rng(2).permutation(129))       # every site its own block
    assert L["q_max"] == 1 and L["mpad"] == 192                           # m no multiple of the padding
    L = check(shim, 2, np.array([1] * 64 + [0] * 64))                     # m a multiple: no padding row
    assert L["mpad"] == 128 and np.array_equal(L["perm"], np.concatenate([np.arange(64, 128), np.arange(64)]))


def test_every_refusal_names_the_offender(shim):
    rng = np.random.default_rng(3)
    centres, pc, w = rng.uniform(-60, 60, (4, 2)), rng.uniform(-60, 60, (12, 2)), rng.uniform(0.1, 1, 12)
    lab = np.arange(12) % 4
    assert isinstance(layout(shim, centres, pc, lab, w), dict)

    def changed(a, ix, v):
        a = np.array(a, dtype=np.float64 if a.dtype.kind == "f" else a.dtype)
        a[ix] = v
        return a

    assert "block label 4 of site 9 is outside [0, 4)" in layout(shim, centres, pc, changed(lab, 9, 4), w)
    assert "block label -1 of site 0 is outside [0, 4)" in layout(shim, centres, pc, changed(lab, 0, -1), w)
    assert "block 2 has no site" in layout(shim, centres, pc, np.where(lab == 2, 3, lab), w)
    assert "weight of site 5 is not finite (nan)" in layout(shim, centres, pc, lab, changed(w, 5, np.nan))
    assert "weight of site 11 is not finite (-inf)" in layout(shim, centres, pc, lab, changed(w, 11, -np.inf))
    assert "coordinate 0 of centre 3 is not finite (nan)" in layout(shim, changed(centres, (3, 0), np.nan), pc, lab, w)
    assert "coordinate 1 of centre 0 is not finite (inf)" in layout(shim, changed(centres, (0, 1), np.inf), pc, lab, w)
    assert "coordinate 1 of site 7 is not finite (nan)" in layout(shim, centres, changed(pc, (7, 1), np.nan), lab, w)
    assert "r must be >= 1, got 0" in layout(shim, centres, pc, lab, w, r=0)
    assert "m must be in [1, 2^31), got 0" in layout(shim, centres, pc[:0], lab[:0], w[:0])
    assert isinstance(layout(shim, centres, pc, lab, w), dict)            # the refusals left nothing behind


def test_layout_under_address_and_undefined_behaviour_sanitizers():
    out = os.path.join(ROOT, "tests", "_build", "host_local_blocks_asan")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host_local_blocks_sanitize_main.cpp"),
           os.path.join(CSRC, "ck_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
