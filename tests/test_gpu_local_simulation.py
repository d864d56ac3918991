"""GPU tests of the conditional simulation in the moving neighbourhood: include/cokrige.h ck_simulate_local and
ck_debug_simulate_local_weights, native.Handle.simulate_local, point_prediction.Predictor.conditional_simulation.

1. per site: the member lists of the weight kernel against tests/local_sim_ref.py exactly (the numpy / device agreement
   condition gap > 1e-9 is asserted for every case), weights, mu^data and s^2 at the local path's own tolerances (rtol 1e-8, atol
   1e-10: tests/test_gpu_local.py), the counts and stats4 exactly -- the issue's rows 1 - 3, i = 1, one haversine case;
2. the recursion alone: a numpy replay on the DEVICE's own weights, means and variances under a given noise;
3. end to end: rows 1 - 3 against the reference's draws, row 4 (full conditioning at the LDS limit) against the dense chain
   pred + eps L_S^T, at rtol 1e-8 and atol 1e-8 sqrt(sigma_i^2 + nugget_i);
4. the generator: the device's Philox normals against the host's (tests/host_rng_shim.cpp), and the bits of draws 0 - 4
   across n_draws, draw_chunk and repeated calls;
5. ragged sizes; 6. the contract: every refusal with its message (the two memory refusals through option "sim_free_bytes"), the
   65-member set, identical sites, state; 7. the Python layer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import cokrige_oracle as orc
from tests import local_sim_ref as ls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAV, EUC = 0, 1
RTOL, ATOL = 1e-8, 1e-10
_cache = {}


@pytest.fixture(scope="module")
def native():
    from sif_xco2_cokriging_amd import native as nat
    assert nat.device_count() >= 1
    return nat


def make_handle(native, pb, caps=None, **options):
    h = native.Handle(0)
    for name, value in options.items():
        h.set_option(name, value)
    pv = list(pb["params"])
    if len(pb["coords"]) == 2:
        h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    else:
        h.set_model(1, pv[0:1], pv[1:2], pv[2:3], pv[3:4])
    h.set_metric(pb["metric"])
    for k in range(len(pb["coords"])):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.set_local_neighbours(*(pb["caps"] if caps is None else caps))
    return h


def case(name):
    """The problems of the tests with their references, computed once: the issue's rows by number, and the extra cases"""
    if name in _cache:
        return _cache[name]
    i, noise = 0, None
    if name in (1, 2, 3, 4):
        pb = ls.row_inputs(name)
    elif name == "i1":                       # row 2 with the sites behind process 1
        pb, i = ls.row_inputs(2), 1
    elif name == "haversine":                # conus_problem(60): 40 sites over the lattice's extent, 800 km, caps (6, 6)
        from sif_xco2_cokriging_amd import synth
        cp = synth.conus_problem(60)
        rng = np.random.default_rng(7)
        sites = np.column_stack([rng.uniform(24, 56, 40), rng.uniform(-123, -67, 40)])
        pb = dict(params=cp["params"], coords=cp["coords"], values=cp["values"], metric=HAV, sites=sites,
                  ranks=rng.permutation(40).astype(np.int64), caps=(6, 6), max_dist=800.0)
    elif name == "m257":                     # row 3's data, 257 sites: one past a 256-site boundary
        pb = dict(ls.row_inputs(3))
        rng = np.random.default_rng(7)
        pb["sites"], pb["ranks"] = rng.random((257, 2)), rng.permutation(257).astype(np.int64)
    elif name == "one_process":              # row 2's process 0 alone
        pb = dict(ls.row_inputs(2))
        pv = pb["params"]
        pb.update(params=[pv[0], pv[2], pv[5], pv[8]], coords=pb["coords"][:1], values=pb["values"][:1], caps=(6, 0))
    elif name == "noise":                    # row 4 with measurement-error variances on both processes
        pb = dict(ls.row_inputs(4))
        rng = np.random.default_rng(21)
        noise = [0.05 + 0.1 * rng.random(20), 0.02 + 0.1 * rng.random(20)]
    else:
        raise KeyError(name)
    ref = ls.local_sim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], i, pb["sites"], pb["ranks"], pb["max_dist"],
                                 pb["caps"], noise=noise)
    assert ref["gap"] > 1e-9, (name, ref["gap"])   # numpy and the device must agree on every set
    assert ref["info"] == 0
    if name in ls.ROWS:
        want = ls.ROWS[name]
        assert (ref["n_empty"], ref["k_max"], ref["ns_max"], ref["n_levels"]) == (want["n_empty"], want["k_max"], want["ns_max"],
                                                                                    want["n_levels"])
    p = orc.Params.from_flat(pb["params"])
    pb = dict(pb, i=i, noise=noise, c0=float(p.sigma[i] ** 2 + p.nugget[i]), N=sum(len(c) for c in pb["coords"]))
    _cache[name] = (pb, ref)
    return _cache[name]


def handle_of(native, pb, **options):
    h = make_handle(native, pb, **options)
    if pb["noise"] is not None:
        for k, d in enumerate(pb["noise"]):
            h.set_noise(k, d, 1.0)
    return h


def padded(rows, fill, dtype):
    out = np.full((len(rows), 64), fill, dtype=dtype)
    for t, r in enumerate(rows):
        out[t, :len(r)] = r
    return out


def eps_for(pb, n_draws, seed=5):
    return np.random.default_rng(seed).standard_normal((n_draws, len(pb["sites"])))


def replay(pb, idx, w, mean, var, eps):
    """the recursion in numpy on given weights: members as stacked caller indices (a site: N + its index)"""
    N, m = pb["N"], len(pb["sites"])
    pos = np.empty(m, dtype=np.int64)
    pos[np.argsort(pb["ranks"], kind="stable")] = np.arange(m)
    Y = np.full(eps.shape, np.nan)
    for t in np.argsort(pos):
        s = idx[t] >= N
        sd = np.sqrt(var[t]) if var[t] > 0 else np.nan
        Y[:, t] = mean[t] + Y[:, idx[t][s] - N] @ w[t][s] + sd * eps[:, t]
    return Y


# ---------------------------------------------------------------------------------------------------------------------
# 1. per site
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [1, 2, 3, "i1", "haversine"])
def test_sets_weights_means_and_variances_per_site(native, name):
    pb, ref = case(name)
    h = handle_of(native, pb)
    idx, w = h.simulate_local_weights(pb["i"], pb["sites"], pb["ranks"], pb["max_dist"])
    assert np.array_equal(idx, padded(ref["members"], -1, np.int64)), name     # the member lists, exactly
    wr = padded(ref["weights"], 0.0, np.float64)
    _, info, st = h.simulate_local(pb["i"], pb["sites"], pb["ranks"], pb["max_dist"], 2, noise=eps_for(pb, 2))
    print(f"{name}: max |dw| {np.max(np.abs(w - wr)):.2e}, max |dmean| {np.max(np.abs(st['mean'] - ref['mean'])):.2e}, "
          f"max rel dvar {np.max(np.abs(st['var'] - ref['var']) / ref['var']):.2e}, k_max {st['k_max']}, levels {st['n_levels']}")
    np.testing.assert_allclose(w, wr, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["mean"], ref["mean"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(st["var"], ref["var"], rtol=RTOL, atol=ATOL)
    assert info == 0
    assert np.array_equal(st["count"], ref["count"])
    assert (st["n_empty"], st["k_max"], st["n_capped"], st["n_levels"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"],
                                                                            ref["n_levels"])
    tm = h.simulate_local_timings()
    assert tm["n_levels"] == ref["n_levels"] and tm["n_solved"] == len(pb["sites"]) - ref["n_empty"]
    assert tm["n_site_neighbours"] == ref["count"][:, 2].sum() and tm["select_ms"] > 0 and tm["weights_ms"] > 0 and tm["total_ms"] > 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the recursion alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [1, 2, 3])
def test_recursion_on_the_devices_own_weights(native, name):
    """At most 66 terms per site and at most 27 levels: <= 1e-11 (1 + max |Y|).  Measured on the MI355X: max |dY| 4.4e-16 (row 1),
    4.4e-16 (row 2), 8.9e-16 (row 3) against bounds of 3.7e-11 .. 4.1e-11."""
    pb, ref = case(name)
    h = handle_of(native, pb)
    eps = eps_for(pb, 7)
    idx, w = h.simulate_local_weights(pb["i"], pb["sites"], pb["ranks"], pb["max_dist"])
    Y, info, st = h.simulate_local(pb["i"], pb["sites"], pb["ranks"], pb["max_dist"], 7, noise=eps)
    want = replay(pb, [r[r >= 0] for r in idx], [w[t][idx[t] >= 0] for t in range(len(idx))], st["mean"], st["var"], eps)
    err, scale = np.max(np.abs(Y - want)), 1.0 + np.max(np.abs(want))
    print(f"row {name}: recursion against its numpy replay: max |dY| {err:.2e}, bound {1e-11 * scale:.2e}")
    assert info == 0 and err <= 1e-11 * scale
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [1, 2, 3, "i1", "haversine"])
def test_draws_against_the_reference(native, name):
    pb, ref = case(name)
    h = handle_of(native, pb)
    eps = eps_for(pb, 6)
    Y, info, _ = h.simulate_local(pb["i"], pb["sites"], pb["ranks"], pb["max_dist"], 6, noise=eps)
    want = ref["draws"](eps)
    print(f"{name}: draws against the reference: max |dY| {np.max(np.abs(Y - want)):.2e}")
    assert info == 0
    np.testing.assert_allclose(Y, want, rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    h.close()


def test_full_conditioning_is_the_dense_posterior(native):
    """Row 4: every datum and every earlier site in every set, the largest set 63 members"""
    pb, ref = case(4)
    h = handle_of(native, pb)
    eps = eps_for(pb, 6)
    Y, info, st = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 6, noise=eps)
    pred, L, order = ls.dense_chain(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, pb["sites"], pb["ranks"])
    want = ls.dense_draws(pred, L, order, eps)
    print(f"row 4: draws against the dense chain: max |dY| {np.max(np.abs(Y - want)):.2e}")
    assert info == 0 and (st["k_max"], st["n_levels"], st["n_empty"], st["n_capped"]) == (63, 24, 0, 0)
    np.testing.assert_allclose(Y, want, rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the generator
# ---------------------------------------------------------------------------------------------------------------------
def host_normals(seed, m, n_draws):
    so = os.path.join(ROOT, "tests", "_build", "libck_host_rng_local_sim.so")
    if "rng" not in _cache:
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "sif-xco2-cokriging_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_rng_shim.cpp"), "-o", so], check=True)
        _cache["rng"] = ctypes.CDLL(so)
    eps = np.empty((n_draws, m))
    _cache["rng"].shim_normals(ctypes.c_uint64(seed), ctypes.c_long(m), ctypes.c_long(n_draws),
                               eps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return eps


def test_device_normals_are_the_hosts_and_draws_do_not_depend_on_the_chunking(native):
    """The device's normals differ from the host's by at most 2 ulp (libm against the device's log / sqrt / cos / sin).  Carried
    through the recursion: b_t = sum_u |w_u| b_u + s_t 2 ulp(eps_t), plus the rounding of a sum of at most 66 terms of either
    run, 66 * 2^-52 * (|mu| + sum_u |w_u Y_u| + s_t |eps_t|)."""
    pb, ref = case(3)
    m, seed = len(pb["sites"]), 2024
    h = handle_of(native, pb)
    eps = host_normals(seed, m, 37)
    Yn, info, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 37, noise=eps)
    Y37, info2, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 37, seed=seed)
    assert info == 0 and info2 == 0
    bound = np.zeros_like(eps)
    for t in np.argsort(ref["pos"]):
        u, wu = ref["nbr_sites"][t], np.abs(ref["weights"][t][ref["members"][t] >= pb["N"]])
        sd = np.sqrt(ref["var"][t])
        size = np.abs(ref["mean"][t]) + np.abs(Yn[:, u]) @ wu + sd * np.abs(eps[:, t])
        bound[:, t] = bound[:, u] @ wu + sd * 2 * np.spacing(np.abs(eps[:, t])) + 66 * 2.0 ** -52 * size
    print(f"device normals against the host's: max |dY| {np.max(np.abs(Y37 - Yn)):.2e}, largest bound {bound.max():.2e}, "
          f"max ratio {np.max(np.abs(Y37 - Yn) / bound):.2f}")
    assert np.all(np.abs(Y37 - Yn) <= bound)
    # draws 0 - 4: the same bits whatever n_draws, the chunk and the call
    Y5, _, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 5, seed=seed)
    assert np.array_equal(Y5, Y37[:5])
    assert np.array_equal(h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 5, seed=seed)[0], Y5)
    h.set_option("draw_chunk", 8)
    Y37c, _, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 37, seed=seed)
    assert np.array_equal(Y37c, Y37)
    assert np.array_equal(h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 5, seed=seed)[0], Y5)
    Ync, _, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 37, noise=eps)
    assert np.array_equal(Ync, Yn)
    other, _, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 5, seed=seed + 1)
    assert not np.array_equal(other, Y5)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ragged sizes
# ---------------------------------------------------------------------------------------------------------------------
def test_one_site_and_one_draw(native):
    pb, ref = case(2)
    h = handle_of(native, pb)
    t = 17
    one = dict(pb, sites=pb["sites"][[t]], ranks=np.array([5], dtype=np.int64))
    r1 = ls.local_sim_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, one["sites"], one["ranks"], pb["max_dist"],
                                pb["caps"])
    assert r1["gap"] > 1e-9 and r1["count"][0, 2] == 0 and r1["n_levels"] == 1
    eps = np.random.default_rng(3).standard_normal((4, 1))
    Y, info, st = h.simulate_local(0, one["sites"], one["ranks"], pb["max_dist"], 4, noise=eps)
    assert info == 0 and Y.shape == (4, 1) and st["n_levels"] == 1 and np.array_equal(st["count"], r1["count"])
    np.testing.assert_allclose(Y, r1["draws"](eps), rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    # the prediction of the same site is the draws' mean term: no earlier site in the set
    pred, err, _ = h.predict_local(0, one["sites"], max_dist=pb["max_dist"])
    np.testing.assert_allclose(st["mean"], pred, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(np.sqrt(st["var"]), err, rtol=RTOL, atol=ATOL)
    # one draw of all sites: the first row of a longer call under the same noise
    e6 = eps_for(pb, 6)
    Y1, info, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 1, noise=e6[:1])
    Y6, _, _ = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 6, noise=e6)
    assert info == 0 and Y1.shape == (1, 50) and np.array_equal(Y1[0], Y6[0])
    np.testing.assert_allclose(Y1, ref["draws"](e6[:1]), rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    h.close()


@pytest.mark.parametrize("name", ["m257", "one_process"])
def test_257_sites_and_a_one_process_model(native, name):
    pb, ref = case(name)
    h = handle_of(native, pb)
    eps = eps_for(pb, 3)
    idx, w = h.simulate_local_weights(0, pb["sites"], pb["ranks"], pb["max_dist"])
    assert np.array_equal(idx, padded(ref["members"], -1, np.int64))
    Y, info, st = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 3, noise=eps)
    assert info == 0 and np.array_equal(st["count"], ref["count"])
    assert (st["n_empty"], st["k_max"], st["n_capped"], st["n_levels"]) == (ref["n_empty"], ref["k_max"], ref["n_capped"],
                                                                            ref["n_levels"])
    if name == "one_process":
        assert not st["count"][:, 1].any()
    np.testing.assert_allclose(Y, ref["draws"](eps), rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    h.close()


def test_noise_under_full_conditioning_is_the_dense_posterior_with_noise(native):
    pb, ref = case("noise")
    h = handle_of(native, pb)
    eps = eps_for(pb, 5)
    Y, info, st = h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 5, noise=eps)
    pred, L, order = ls.dense_chain(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, pb["sites"], pb["ranks"],
                                    noise=pb["noise"])
    want = ls.dense_draws(pred, L, order, eps)
    plain = ls.dense_draws(*ls.dense_chain(pb["params"], pb["coords"], pb["values"], pb["metric"], 0, pb["sites"], pb["ranks"]), eps)
    print(f"noise: draws against the dense chain: max |dY| {np.max(np.abs(Y - want)):.2e}; the noise moves them by "
          f"{np.max(np.abs(want - plain)):.2e}")
    assert info == 0 and st["k_max"] == 63
    assert np.max(np.abs(want - plain)) > 1e-3          # the case tests something
    np.testing.assert_allclose(Y, want, rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    np.testing.assert_allclose(st["var"], ref["var"], rtol=RTOL, atol=ATOL)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the contract
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(native):
    pb, _ = case(2)
    h = handle_of(native, pb)
    s, r, md = pb["sites"], pb["ranks"], pb["max_dist"]
    dup = r.copy()
    dup[40] = dup[3]
    with pytest.raises(native.NativeError, match=r"ck_simulate_local: sites 3 and 40 have the same rank " + str(int(r[3]))):
        h.simulate_local(0, s, dup, md, 2)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(native.NativeError, match="max_dist must be finite and >= 0"):
            h.simulate_local(0, s, r, bad, 2)
    with pytest.raises(native.NativeError, match=r"n_draws = 0; at least 1"):
        h.simulate_local(0, s, r, md, 0)
    with pytest.raises(native.NativeError, match="process index out of range"):
        h.simulate_local(2, s, r, md, 2)
    L = native.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    sc, rc = np.ascontiguousarray(s), np.ascontiguousarray(r)
    draws, st, info = np.zeros((2, 50)), np.zeros(4, dtype=np.int64), ctypes.c_int64(0)
    args = dict(p=native._p(sc), r=rc.ctypes.data_as(i64), d=native._p(draws), s=st.ctypes.data_as(i64), i=ctypes.byref(info))
    for missing in "prdsi":
        a = dict(args, **{missing: None})
        assert L.ck_simulate_local(h._h, 0, a["p"], 50, a["r"], md, 2, 1, None, a["d"], None, None, None, a["s"], a["i"]) == -1
        assert "null pcoords_host / rank_host / draws_host / stats4 / info" in L.ck_last_error().decode()
    assert L.ck_simulate_local(h._h, 0, args["p"], 0, args["r"], md, 2, 1, None, args["d"], None, None, None, args["s"], args["i"]) == -1
    assert "m = 0 sites; at least 1" in L.ck_last_error().decode()
    # every output but the draws, stats4 and info is optional
    assert L.ck_simulate_local(h._h, 0, args["p"], 50, args["r"], md, 2, 1, None, args["d"], None, None, None, args["s"], args["i"]) == 0
    idx, w = np.zeros((50, 64), dtype=np.int64), np.zeros((50, 64))
    assert L.ck_debug_simulate_local_weights(h._h, 0, args["p"], 50, args["r"], md, None, native._p(w)) == -1
    assert "ck_debug_simulate_local_weights: null" in L.ck_last_error().decode()
    h.set_trend(0, np.ones((40, 1)))
    with pytest.raises(native.NativeError, match="a trend of 1 columns is set on the handle"):
        h.simulate_local(0, s, r, md, 2)
    h.set_trend(0, None)
    assert h.simulate_local(0, s, r, md, 2)[1] == 0
    with pytest.raises(ValueError, match="rank has 49 entries"):
        h.simulate_local(0, s, r[:-1], md, 2)
    h.close()
    hp = native.Handle(devices=[0, 0], rank=0)
    hp.set_model(2, pb["params"][0:2], pb["params"][2:5], pb["params"][5:8], pb["params"][8:10], pb["params"][10])
    hp.set_metric(EUC)
    for k in range(2):
        hp.set_data(k, pb["coords"][k], pb["values"][k])
    with pytest.raises(native.NativeError, match=r"single-process form: this handle is partitioned \(world = 2\)"):
        hp.simulate_local(0, s, r, md, 2)
    hp.close()


def test_too_little_device_memory_states_the_amounts(native):
    """Option "sim_free_bytes" stands for what the device reports as free: both memory refusals without filling the device"""
    pb, _ = case(2)
    h = handle_of(native, pb)
    s, r, md, m = pb["sites"], pb["ranks"], pb["max_dist"], 50
    eps = eps_for(pb, 6)
    want = h.simulate_local(0, s, r, md, 6, noise=eps)[0]
    w_bytes = m * (64 * (2 * 4 + 2 * 8) + 2 * 8 + 4)          # members, positions, two weight rows, mu, s^2, the site count
    chunk_bytes = 2 * (2 * m * 8) + 2 * m * 4                   # two draws of Y and of the output, the order and the positions
    h.set_option("sim_free_bytes", w_bytes - 1)
    msg = rf": needs {w_bytes} bytes of device memory for the weights of 50 sites; {w_bytes - 1} bytes are available"
    with pytest.raises(native.NativeError, match="ck_simulate_local" + msg):
        h.simulate_local(0, s, r, md, 6, noise=eps)
    tm = h.simulate_local_timings()
    assert tm["select_ms"] > 0 and tm["weights_ms"] == 0       # refused behind the select pass, before the weight kernel
    with pytest.raises(native.NativeError, match="ck_debug_simulate_local_weights" + msg):
        h.simulate_local_weights(0, s, r, md)
    h.set_option("sim_free_bytes", w_bytes + chunk_bytes - 1)   # the weights fit, the smallest chunk does not
    with pytest.raises(native.NativeError, match=rf"ck_simulate_local: needs {chunk_bytes} bytes of device memory for a chunk of 2 "
                                                 rf"draws at 50 sites; {chunk_bytes - 1} bytes are available"):
        h.simulate_local(0, s, r, md, 6, noise=eps)
    assert h.simulate_local_timings()["weights_ms"] > 0 and h.simulate_local_timings()["recursion_ms"] == 0
    h.simulate_local_weights(0, s, r, md)                       # the debug call needs the weights only
    h.set_option("sim_free_bytes", w_bytes + chunk_bytes)       # exactly enough: chunks of two draws, the same bits
    got, info, _ = h.simulate_local(0, s, r, md, 6, noise=eps)
    assert info == 0 and np.array_equal(got, want)
    with pytest.raises(native.NativeError, match="sim_free_bytes must be >= 0"):
        h.set_option("sim_free_bytes", -1)
    h.set_option("sim_free_bytes", 0)
    assert np.array_equal(h.simulate_local(0, s, r, md, 6, noise=eps)[0], want)
    h.close()


def test_a_set_of_65_is_refused_before_any_solve(native):
    pb, _ = case(4)
    rng = np.random.default_rng(7)
    sites, ranks = rng.random((26, 2)), rng.permutation(26).astype(np.int64)
    h = handle_of(native, pb)
    with pytest.raises(native.NativeError, match=r"ck_simulate_local: 1 sites have a conditioning set of more than 64 data "
                                                 r"\(the largest: 65\); the draws are for sets the LDS solver takes"):
        h.simulate_local(0, sites, ranks, pb["max_dist"], 2)
    tm = h.simulate_local_timings()
    assert tm["select_ms"] > 0 and tm["weights_ms"] == 0 and tm["recursion_ms"] == 0       # the select pass ran, nothing else
    with pytest.raises(native.NativeError, match="conditioning set of more than 64"):
        h.simulate_local_weights(0, sites, ranks, pb["max_dist"])
    h.set_local_neighbours(40, 0)                                     # under a cap the same request is served
    assert h.simulate_local(0, sites, ranks, pb["max_dist"], 2)[1] == 0
    h.close()


def test_identical_sites_are_reported_not_repaired(native):
    pb, ref = case(2)
    h = handle_of(native, pb)
    sites, ranks = pb["sites"].copy(), pb["ranks"].copy()
    a, b = (7, 31) if ranks[7] < ranks[31] else (31, 7)               # b is visited after a
    sites[b] = sites[a]
    eps = eps_for(pb, 3)
    Y, info, st = h.simulate_local(0, sites, ranks, pb["max_dist"], 3, noise=eps)
    print(f"identical sites {a}, {b}: info {info}, s^2 of the later {st['var'][b]!r}, count {st['count'][b]}")
    assert st["count"][b, 2] >= 1                                     # the later conditions on the earlier
    assert info == b + 1
    assert np.all(np.isnan(Y[:, b])) and not np.any(np.isnan(Y[:, a]))
    ok = np.ones(50, dtype=bool)
    ok[b] = False
    assert np.all(np.isfinite(st["mean"][ok])) and np.all(st["var"][ok] > 0)
    h.close()


def test_the_callers_handle_keeps_its_state_and_bits(native):
    pb, _ = case(2)
    h = handle_of(native, pb)
    grid = np.random.default_rng(4).random((70, 2))
    h.assemble_joint()
    assert h.factor() == 0
    j0 = h.predict(0, grid)
    l0 = h.predict_local(0, grid, max_dist=pb["max_dist"])
    h.simulate_local(0, pb["sites"], pb["ranks"], pb["max_dist"], 4, seed=9)
    h.simulate_local_weights(0, pb["sites"], pb["ranks"], pb["max_dist"])
    l1 = h.predict_local(0, grid, max_dist=pb["max_dist"])
    j1 = h.predict(0, grid)                                           # the resident factor: no new assembly, the same bits
    assert np.array_equal(l0[0], l1[0], equal_nan=True) and np.array_equal(l0[1], l1[1], equal_nan=True) and l0[2] == l1[2]
    assert np.array_equal(j0[0], j1[0]) and np.array_equal(j0[1], j1[1])
    assert h.verify_model() == 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------------------------------------------------------
class _Attrs:
    def __init__(self, attrs):
        self.attrs = attrs


class _StubTrend:
    def predict(self, X):
        X = np.asarray(X, dtype=float)
        return 0.3 * X[:, 0] - 0.2 * X[:, 1] + 0.05


def test_predictor_surface(native):
    from sif_xco2_cokriging_amd import fields, model, point_prediction
    pb, ref = case(2)
    at = dict(scale_fact=1.7, spatial_mean=0.25, temporal_trend=-0.4, covariate_means=[0.5, 0.5], covariate_scales=[0.3, 0.3],
              spatial_model=_StubTrend())
    f0, f1 = fields.Field(pb["coords"][0], pb["values"][0]), fields.Field(pb["coords"][1], pb["values"][1])
    for f in (f0, f1):
        f.ds = _Attrs(at)
        f.timestamp = "2020-07-01"
    mod = model.MultivariateMatern(params=model.MaternParams().set_values(pb["params"]))
    P = point_prediction.Predictor(mod, fields.MultiField([f0, f1]), dist_units=None, fast_dist=False, max_neighbours=pb["caps"])
    m = len(pb["sites"])
    # an explicit rank array is the native call
    eps = eps_for(pb, 6)
    draws, pred, err, pinned, seed = P.conditional_draws_arrays(0, pb["sites"], pb["max_dist"], 6, seed=11, ordering=pb["ranks"],
                                                                noise=eps)
    assert seed == 11 and not pinned.any() and P.sim_info["n_pinned"] == 0 and P.sim_info["ordering"] == "ranks"
    assert (P.sim_info["n_levels"], P.sim_info["n_empty"]) == (ref["n_levels"], ref["n_empty"])
    np.testing.assert_allclose(draws, ref["draws"](eps), rtol=1e-8, atol=1e-8 * np.sqrt(pb["c0"]))
    pp, ee = P.predict_arrays(0, pb["sites"], max_dist=pb["max_dist"])
    assert np.array_equal(pred, pp, equal_nan=True) and np.array_equal(err, ee, equal_nan=True)   # (one site has no datum in reach)
    # pinned: a repeated site, a site on a datum of process 0, and the repeat of that
    pcd = np.vstack([pb["sites"], pb["sites"][[3]], pb["coords"][0][[5]], pb["coords"][0][[5]]])
    for ordering in ("random", "hilbert"):
        d2, _, _, pin2, _ = P.conditional_draws_arrays(0, pcd, pb["max_dist"], 8, seed=11, ordering=ordering)
        assert pin2[m:].all() and not pin2[:m].any() and P.sim_info["n_pinned"] == 3 and P.sim_info["ordering"] == ordering
        assert np.array_equal(d2[:, m], d2[:, 3])
        assert np.all(d2[:, m + 1] == pb["values"][0][5]) and np.all(d2[:, m + 2] == pb["values"][0][5])
        assert np.all(np.isfinite(d2)) and P.sim_info["n_levels"] >= 1
        again = P.conditional_draws_arrays(0, pcd, pb["max_dist"], 8, seed=11, ordering=ordering)[0]
        assert np.array_equal(again, d2)
    # pred / pred_err are the ordinary prediction even on a predictor that cross_validation left with cv = True
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = P.predict_arrays(0, pcd, max_dist=pb["max_dist"])
        P.cv = True
        loo = P.predict_arrays(0, pcd, max_dist=pb["max_dist"])
        _, pred_cv, err_cv, _, _ = P.conditional_draws_arrays(0, pcd, pb["max_dist"], 2, seed=11)
    assert P.cv is True and loo[0][m + 1] != plain[0][m + 1]           # the site on a datum: leave-one-out differs there
    assert np.array_equal(pred_cv, plain[0], equal_nan=True) and np.array_equal(err_cv, plain[1], equal_nan=True)
    P.cv = False
    for kw, msg in [(dict(n_draws=0), "n_draws"), (dict(ordering="sweep"), "ordering must be one of"),
                    (dict(ordering=np.arange(m - 1)), "the ordering has"), (dict(noise=np.zeros((3, 3))), "noise has shape"),
                    (dict(seed=-1), "seed")]:
        args = dict(n_draws=4, seed=1, ordering="random", noise=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            P.conditional_draws_arrays(0, pb["sites"], pb["max_dist"], args.pop("n_draws"), **args)
    # the structure of the joint method, and the transform of every draw
    raw = P.conditional_simulation(0, pb["sites"], max_dist=pb["max_dist"], n_draws=12, seed=11, postprocess=False)
    out = P.conditional_simulation(0, pb["sites"], max_dist=pb["max_dist"], n_draws=12, seed=11, postprocess=True)
    keys = {"seed", "ordering", "n_levels", "n_empty", "n_pinned"}
    if point_prediction.xr is None:
        (df_raw, d_raw), (df, d) = raw, out
        assert set(df.attrs) == keys and df.attrs["seed"] == 11 and df.attrs["ordering"] == "random" and df.attrs["n_pinned"] == 0
        assert d.shape == (12, m) and list(df.columns) == ["pred", "pred_err"] and list(df.index.names) == ["lon", "lat"]
        assert np.allclose(d - df["pred"].values, 1.7 * (d_raw - df_raw["pred"].values), rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(df["pred_err"].values, 1.7 * df_raw["pred_err"].values, equal_nan=True)
        offset = 0.25 + _StubTrend().predict((pb["sites"][:, ::-1] - 0.5) / 0.3) - 0.4     # every draw as pred is transformed
        assert np.allclose(d, 1.7 * d_raw + offset, rtol=0, atol=1e-12)
    else:
        assert out["draws"].dims[0] == "draw" and keys <= set(out.attrs) and out.attrs["seed"] == 11
        dd, rr = (out["draws"] - out["pred"]).values, (raw["draws"] - raw["pred"]).values
        assert np.allclose(dd, 1.7 * rr, rtol=0, atol=1e-12, equal_nan=True)
    P.close()
    T = point_prediction.Predictor(mod, fields.MultiField([f0, f1]), dist_units=None, fast_dist=False, trend="constant")
    with pytest.raises(NotImplementedError, match="simple cokriging only"):
        T.conditional_draws_arrays(0, pb["sites"], pb["max_dist"], 2)
    T.close()
