"""The random numbers of the conditional simulation (csrc/ck_rng.h: Philox4x32-10 and FP64 Box-Muller, used by
ck_conditional_draws) compiled for the host with g++ (tests/host_rng_shim.cpp) and checked against numpy, without a GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "host_rng_shim.cpp")
u32p = ctypes.POINTER(ctypes.c_uint32)
dp = ctypes.POINTER(ctypes.c_double)

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def _build(name, extra):
    so = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + CSRC] + extra + [SHIM, "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def shim():
    return _build("libck_host_rng.so", [])


def philox_numpy(ctr, key):
    """Philox4x32-10 of Salmon et al. (SC'11) on arrays: ctr (n, 4), key (n, 2) of uint32"""
    c = [ctr[:, q].astype(np.uint64) for q in range(4)]
    k0, k1 = key[:, 0].astype(np.uint32), key[:, 1].astype(np.uint32)
    lo32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r > 0:
            k0 = (k0 + W0).astype(np.uint32)
            k1 = (k1 + W1).astype(np.uint32)
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & lo32
        hi1, lo1 = p1 >> np.uint64(32), p1 & lo32
        c = [hi1 ^ c[1] ^ k0.astype(np.uint64), lo1, hi0 ^ c[3] ^ k1.astype(np.uint64), lo0]
    return np.stack(c, axis=1).astype(np.uint32)


def normals_numpy(seed, n_sites, n_draws):
    """the documented transform: counter (k, d / 2, 0, 0), key = seed; two 53-bit uniforms, Box-Muller"""
    k = np.repeat(np.arange(n_sites, dtype=np.uint32), (n_draws + 1) // 2)
    pair = np.tile(np.arange((n_draws + 1) // 2, dtype=np.uint32), n_sites)
    ctr = np.stack([k, pair, np.zeros_like(k), np.zeros_like(k)], axis=1)
    key = np.tile(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (len(k), 1))
    w = philox_numpy(ctr, key).astype(np.uint64)
    a = (w[:, 0] << np.uint64(21)) | (w[:, 1] >> np.uint64(11))
    b = (w[:, 2] << np.uint64(21)) | (w[:, 3] >> np.uint64(11))
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (b.astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.array([math.log(x) for x in u1]))
    t = 6.283185307179586 * u2
    z = np.empty((n_sites, 2 * ((n_draws + 1) // 2)))
    z[:, 0::2] = (r * np.array([math.cos(x) for x in t])).reshape(n_sites, -1)
    z[:, 1::2] = (r * np.array([math.sin(x) for x in t])).reshape(n_sites, -1)
    return z[:, :n_draws].T.copy()


def shim_philox(lib, ctr, key):
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty((len(ctr), 4), dtype=np.uint32)
    lib.shim_philox(ctr.ctypes.data_as(u32p), key.ctypes.data_as(u32p), ctypes.c_long(len(ctr)), out.ctypes.data_as(u32p))
    return out


def shim_normals(lib, seed, n_sites, n_draws):
    out = np.empty((n_draws, n_sites))
    lib.shim_normals(ctypes.c_uint64(seed), ctypes.c_long(n_sites), ctypes.c_long(n_draws), out.ctypes.data_as(dp))
    return out


def random_sets(n=20000):
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    # edge words: all zero, all ones, the shapes the draws use (k, d / 2, 0, 0)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [5, 7, 0, 0], [65535, 2 ** 31, 0, 0]]
    key[:4] = [[0, 0], [0xFFFFFFFF] * 2, [1, 0], [0xDEADBEEF, 0x12345678]]
    return ctr, key


def test_philox_words_match_numpy(shim):
    ctr, key = random_sets()
    assert np.array_equal(shim_philox(shim, ctr, key), philox_numpy(ctr, key))


def test_philox_known_answers(shim):
    """the published known-answer vectors of Random123 (kat_vectors: philox4x32_10)"""
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], dtype=np.uint32)
    key = np.array([[0, 0], [0xFFFFFFFF] * 2, [0xA4093822, 0x299F31D0]], dtype=np.uint32)
    want = np.array([[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8],
                     [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]], dtype=np.uint32)
    assert np.array_equal(shim_philox(shim, ctr, key), want)


def test_philox_matches_rocrand():
    """an independent implementation: rocRAND's host-callable engine (test shim only; never used by the library)"""
    hdr = "/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"
    if not os.path.exists(hdr):
        pytest.skip("rocRAND headers not installed")
    lib = _build("libck_host_rng_rocrand.so", ["-DCK_SHIM_ROCRAND", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"])
    ctr, key = random_sets(5000)
    out = np.empty((len(ctr), 4), dtype=np.uint32)
    lib.shim_rocrand_philox(ctr.ctypes.data_as(u32p), key.ctypes.data_as(u32p), ctypes.c_long(len(ctr)),
                            out.ctypes.data_as(u32p))
    assert np.array_equal(out, shim_philox(lib, ctr, key))


@pytest.mark.parametrize("seed", [0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1])
def test_normals_match_numpy(shim, seed):
    n_sites, n_draws = 37, 101   # an odd number of draws: the last pair's second normal is not used
    got = shim_normals(shim, seed, n_sites, n_draws)
    want = normals_numpy(seed, n_sites, n_draws)
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    assert np.all(np.isfinite(got))
    assert np.max(ulp) <= 2.0


def test_draw_independent_of_count(shim):
    """draw d does not depend on how many draws are made"""
    a = shim_normals(shim, 5, 20, 100)
    b = shim_normals(shim, 5, 20, 11)
    assert np.array_equal(a[:11], b)


def test_normal_statistics(shim):
    """10^6 normals of one seed: mean, variance, and the Kolmogorov-Smirnov distance below the 1 % critical value"""
    z = shim_normals(shim, 12345, 1000, 1000).ravel()
    n = z.size
    assert abs(z.mean()) < 2.576 / math.sqrt(n)
    assert abs(z.var() - 1.0) < 2.576 * math.sqrt(2.0 / n)
    zs = np.sort(z)
    cdf = 0.5 * (1.0 + np.array([math.erf(x / math.sqrt(2.0)) for x in zs]))
    i = np.arange(1, n + 1)
    D = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    assert D < 1.628 / math.sqrt(n)
