"""GPU benchmark of the local predictor's nearest-neighbour cap (ck_set_local_neighbours): bench_local.py's inputs (config-3
sites, the full 0.5-degree grid of 8 833 points) at 200 / 400 / 600 km with caps none, (16, 16), (32, 32), (64, 64) -- per cell
device ms (ck_timings [10]), the select pass ([60]), k_max and n_capped; one warm-up per shape, three interleaved repetitions,
the spread reported.

    python scripts/bench_local_nmax.py [sites per process, default 20000] [--out profiles/r06_local_nmax.json] [--parent <library of the parent commit>]

--parent: the gate on the path users already have.  The uncapped call at 400 km from this library against the parent commit's
(a second build, README "CK_BUILD_OUT", loaded into the same process), alternated call by call; the two results must be
array_equal and this library's median no slower than the parent's own repetitions spread."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RADII = [200.0, 400.0, 600.0]
CAPS = [None, (16, 16), (32, 32), (64, 64)]
REPS = 3


def problem(n):
    from sif_xco2_cokriging_amd import native, synth
    pb = synth.conus_problem(n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(0)
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.local_reserve(0)   # the scratch slab once: no timed call grows it
    return h, pb


def spread(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def table(n):
    h, pb = problem(n)
    cells = [(md, caps) for md in RADII for caps in CAPS]
    acc = {c: dict(device_ms=[], select_ms=[]) for c in cells}
    for md, caps in cells:   # warm-up of every shape
        h.set_local_neighbours(*(caps or (0, 0)))
        h.predict_local(0, pb["pcoords"], md)
    for _ in range(REPS):    # interleaved: every cell once per repetition
        for md, caps in cells:
            h.set_local_neighbours(*(caps or (0, 0)))
            pred, err, info = h.predict_local(0, pb["pcoords"], md)
            t = h.timings()
            a = acc[md, caps]
            a["device_ms"].append(t["local_ms"])
            a["select_ms"].append(t["local_select_ms"])
            a.update(k_max=int(info["k_max"]), n_capped=int(t["local_n_capped"]), cand_max=int(t["local_cand_max"]),
                     n_rescan=int(t["local_n_rescan"]), n_empty=int(info["n_empty"]), n_not_pd=int(info["n_not_pd"]),
                     checksum=float(np.nansum(pred)))
    h.close()
    return [dict(max_dist_km=md, caps=list(caps) if caps else None, device_ms=spread(a.pop("device_ms")),
                 select_ms=spread(a.pop("select_ms")), **a) for (md, caps), a in acc.items()]


def bind(path):
    """a second build of the library in this process, bound like native.lib() binds the product one (the parent commit's build
    lacks the newer symbols: only what it exports is bound)"""
    import ctypes
    from sif_xco2_cokriging_amd import native
    L = ctypes.CDLL(os.path.abspath(path))
    L.ck_last_error.restype = ctypes.c_char_p
    L.ck_last_error.argtypes = []
    for name, args in native._PROTOS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype = ctypes.c_int64 if name in native._RET_INT64 else ctypes.c_int
            fn.argtypes = args
    return L


def gate(n, parent_lib, md=400.0):
    """the uncapped call at md from this library and from the parent's, in one process, alternated call by call"""
    from sif_xco2_cokriging_amd import native
    libs = {"this": native.lib(), "parent": bind(parent_lib)}
    hs, pb = {}, None
    for tag in ("parent", "this"):
        native._lib = libs[tag]          # every native call goes through native.lib()
        hs[tag], pb = problem(n)
        hs[tag].predict_local(0, pb["pcoords"], md)   # warm-up
    ms, res = {"parent": [], "this": []}, {}
    for _ in range(2 * REPS):
        for tag in ("parent", "this"):
            native._lib = libs[tag]
            pred, err, _ = hs[tag].predict_local(0, pb["pcoords"], md)
            ms[tag].append(hs[tag].timings()["local_ms"])
            res[tag] = (pred, err)
    for tag in ("parent", "this"):
        native._lib = libs[tag]
        hs[tag].close()
    native._lib = libs["this"]
    same = bool(np.array_equal(res["parent"][0], res["this"][0], equal_nan=True) and
                np.array_equal(res["parent"][1], res["this"][1], equal_nan=True))
    p, t = spread(ms["parent"]), spread(ms["this"])
    return dict(max_dist_km=md, parent_version=int(libs["parent"].ck_version()), this_version=int(libs["this"].ck_version()),
                parent_device_ms=p, this_device_ms=t, parent_all=ms["parent"], this_all=ms["this"], results_array_equal=same,
                within_parent_spread=bool(t["median"] <= p["max"]))


if __name__ == "__main__":
    args = sys.argv[1:]
    n = int(args[0]) if args and args[0].isdigit() else 20000
    out = {"n_per_process": n, "points": 8833, "repetitions": REPS, "table": table(n)}
    for row in out["table"]:
        print(json.dumps(row), flush=True)
    if "--parent" in args:
        out["uncapped_400km_against_parent"] = gate(n, args[args.index("--parent") + 1])
        print(json.dumps(out["uncapped_400km_against_parent"]), flush=True)
    if "--out" in args:
        path = args[args.index("--out") + 1]
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
