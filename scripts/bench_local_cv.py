"""Cross-validation by folds and buffers in the moving neighbourhood (ck_cv_local_folds): what the call costs, and that the
point calls it shares its search with have not moved.

    python scripts/bench_local_cv.py [--n 20000] [--big 250000] [--reps 5] [--other-lib <libcokrige_hip.so of the parent commit>]
        [--out profiles/<round>_local_cv.json]

regression  ck_predict_local and a capped ck_predict_local (16, 16) at the 8 833 points of the 0.5-degree grid on 2 x n
            observations, 400 km: this library, --other-lib (loaded beside it with ctypes, its own handle) and a copy of
            --other-lib as the control (identical code on a third handle), interleaved in this one process after a warm-up of
            every case; medians, the spread of each handle's own repetitions, this and the control against the parent.
cost        on the same data, caps (16, 16), 400 km, process 0: ck_predict_local(cv = 1) at the data against singleton folds
            (the same neighbour sets), 2-degree spatial blocks with the other process's data of the block withheld too, a random
            10-fold, a 10 km buffer; the same at 2 x --big observations and 60 km beside the Vecchia value call there.
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402
from sif_xco2_cokriging_amd.vecchia import ordering_ranks  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)


class OtherLib:
    """ck_predict_local on another build of the library, through its own handle"""

    def __init__(self, path, pb):
        L = self.L = ctypes.CDLL(path)
        L.ck_last_error.restype = ctypes.c_char_p
        for name in ("ck_create", "ck_set_model", "ck_set_metric", "ck_set_data", "ck_local_reserve", "ck_set_local_neighbours",
                     "ck_predict_local", "ck_timings", "ck_destroy"):
            getattr(L, name).argtypes = native._PROTOS[name]
            getattr(L, name).restype = ctypes.c_int
        self.h = ctypes.c_void_p()
        self.chk(L.ck_create(0, ctypes.byref(self.h)))
        pv = [np.ascontiguousarray(x, dtype=np.float64) for x in (pb["params"][0:2], pb["params"][2:5], pb["params"][5:8], pb["params"][8:10])]
        self.chk(L.ck_set_model(self.h, 2, *(x.ctypes.data_as(_dp) for x in pv), float(pb["params"][10])))
        self.chk(L.ck_set_metric(self.h, int(pb["metric"])))
        for k in range(2):
            c = np.ascontiguousarray(pb["coords"][k], dtype=np.float64)
            v = np.ascontiguousarray(pb["values"][k], dtype=np.float64)
            self.chk(L.ck_set_data(self.h, k, c.ctypes.data_as(_dp), v.ctypes.data_as(_dp), len(v)))
        self.chk(L.ck_local_reserve(self.h, 0))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.ck_last_error().decode())

    def predict_local(self, pc, max_dist, caps):
        pc = np.ascontiguousarray(pc, dtype=np.float64)
        m = len(pc)
        pred, err = np.empty(m), np.empty(m)
        c = [ctypes.c_int64(0) for _ in range(3)]
        self.chk(self.L.ck_set_local_neighbours(self.h, caps[0], caps[1]))
        self.chk(self.L.ck_predict_local(self.h, 0, pc.ctypes.data_as(_dp), m, float(max_dist), 0, pred.ctypes.data_as(_dp),
                                         err.ctypes.data_as(_dp), *(ctypes.byref(x) for x in c)))
        t = np.zeros(16)
        self.chk(self.L.ck_timings(self.h, t.ctypes.data_as(_dp), 16))
        return pred, err, float(t[10])

    def close(self):
        self.L.ck_destroy(self.h)


def make_handle(pb):
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.local_reserve(0)
    return h


def summary(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "ms": [round(float(x), 3) for x in ms]}


def regression(pb, h, other, control, reps, max_dist):
    pc = pb["pcoords"]

    def this(caps):
        h.set_local_neighbours(*caps)
        t0 = time.perf_counter()
        pred, err, _ = h.predict_local(0, pc, max_dist)
        return pred, err, h.timings()["local_ms"], (time.perf_counter() - t0) * 1e3

    def that(lib, caps):
        t0 = time.perf_counter()
        pred, err, dev = lib.predict_local(pc, max_dist, caps)
        return pred, err, dev, (time.perf_counter() - t0) * 1e3

    cases = {}
    for cname, caps in (("uncapped", (0, 0)), ("capped_16_16", (16, 16))):
        cases[cname + "/this"] = lambda caps=caps: this(caps)
        if other is not None:
            cases[cname + "/parent"] = lambda caps=caps: that(other, caps)
            cases[cname + "/control"] = lambda caps=caps: that(control, caps)
    out, res = {k: {"device": [], "wall": []} for k in cases}, {}
    for f in cases.values():
        f()
    for _ in range(reps):
        for k, f in cases.items():
            pred, err, dev, wall = f()
            out[k]["device"].append(dev)
            out[k]["wall"].append(wall)
            res[k] = (pred, err)
    rows = {k: {"device": summary(v["device"]), "wall": summary(v["wall"])} for k, v in out.items()}
    for cname in ("uncapped", "capped_16_16"):
        if other is None:
            continue
        a, b = res[cname + "/this"], res[cname + "/parent"]
        ta, tb, tc = (rows[cname + x]["device"] for x in ("/this", "/parent", "/control"))
        rows[cname + "/compare"] = {"same_bits": bool(np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)),
                                    "median_this_minus_parent_ms": ta["median_ms"] - tb["median_ms"],
                                    "median_control_minus_parent_ms": tc["median_ms"] - tb["median_ms"],
                                    "parent_spread_ms": tb["max_ms"] - tb["min_ms"]}
    h.set_local_neighbours(0, 0)
    return rows


def block_labels(coords, deg):
    """labels of deg x deg spatial blocks, numbered over both processes: (labels per process, number of blocks that hold a datum
    of process 0); a block without one leaves the other process's data there unlabelled"""
    key = [np.floor(c[:, 0] / deg).astype(np.int64) * 100000 + np.floor(c[:, 1] / deg).astype(np.int64) for c in coords]
    u = np.unique(key[0])
    lab0 = np.searchsorted(u, key[0]).astype(np.int32)
    at = np.searchsorted(u, key[1])
    hit = (at < len(u)) & (u[np.minimum(at, len(u) - 1)] == key[1])
    return [lab0, np.where(hit, at, -1).astype(np.int32)], len(u)


def cost(pb, h, reps, max_dist, caps, vecchia):
    n0 = len(pb["values"][0])
    coords = [np.asarray(c, dtype=np.float64)[:, :2] for c in pb["coords"]]
    blocks, n_blocks = block_labels(coords, 2.0)
    rng = np.random.default_rng(1)
    tenfold = (rng.permutation(n0) * 10 // n0).astype(np.int32)
    h.set_local_neighbours(*caps)

    def cv(**kw):
        t0 = time.perf_counter()
        _, _, info = h.cv_local_folds(0, max_dist=max_dist, **kw)
        return dict(h.cv_local_timings(), wall_ms=(time.perf_counter() - t0) * 1e3, k_max=info["k_max"], n_empty=info["n_empty"])

    def loo():
        t0 = time.perf_counter()
        _, _, info = h.predict_local(0, coords[0], max_dist, cv=True)
        return dict(device_ms=h.timings()["local_ms"], wall_ms=(time.perf_counter() - t0) * 1e3, k_max=info["k_max"], n_empty=info["n_empty"])

    cases = {"cv_flag": loo,
             "singleton_folds": lambda: cv(folds_i=np.arange(n0, dtype=np.int32)),
             "blocks_2deg": lambda: cv(folds_i=blocks[0], folds_other=blocks[1], n_folds=n_blocks),
             "tenfold": lambda: cv(folds_i=tenfold),
             "buffer_10km": lambda: cv(buffer=(10.0, 10.0))}
    if vecchia:
        ranks = ordering_ranks(coords, "random", 0)

        def vv():
            t0 = time.perf_counter()
            h.loglik_vecchia(ranks, max_dist)
            return dict(h.vecchia_timings(), wall_ms=(time.perf_counter() - t0) * 1e3)
        cases["vecchia_value"] = vv
    runs = {k: [] for k in cases}
    for f in cases.values():
        f()
    for _ in range(reps):
        for k, f in cases.items():
            runs[k].append(f())
    rows = {}
    for k, rs in runs.items():
        rows[k] = {key: (float(np.median([r[key] for r in rs])) if key.endswith("_ms") else rs[-1][key]) for key in rs[0]}
        rows[k]["wall_ms_all"] = [round(r["wall_ms"], 3) for r in rs]
    h.set_local_neighbours(0, 0)
    return {"n_obs": 2 * n0, "max_dist_km": max_dist, "caps": list(caps), "n_blocks_2deg": n_blocks, "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process")
    ap.add_argument("--big", type=int, default=250000, help="sites per process of the large case (0: skip it)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pb = synth.conus_problem(a.n)
    other = control = None
    native.lib()      # this library and its HIP runtime are mapped first; the handles: the parent's, this library's, the control's
    if a.other_lib:
        import shutil
        import tempfile
        copy = os.path.join(tempfile.mkdtemp(), "libcokrige_control.so")
        shutil.copy(a.other_lib, copy)
        other = OtherLib(a.other_lib, pb)
    h = make_handle(pb)
    if a.other_lib:
        control = OtherLib(copy, pb)
    out = {"reps": a.reps, "regression_400km": regression(pb, h, other, control, a.reps, 400.0)}
    if other is not None:
        other.close()
        control.close()
    out["cost"] = [cost(pb, h, a.reps, 400.0, (16, 16), False)]
    h.close()
    if a.big:
        pb = synth.conus_problem(a.big)
        h = make_handle(pb)
        out["cost"].append(cost(pb, h, max(2, a.reps // 2), 60.0, (16, 16), True))
        h.close()
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
