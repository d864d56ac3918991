"""The local-neighbourhood predictor with a trend: ck_predict_local against ck_predict_local_universal with "constant" (p = 2)
and "linear" (p = 6) on the workloads of scripts/bench_local.py (config-3 sites, all 8 833 points of the 0.5-degree grid,
process 0) at the 125 / 400 / 600 km rows of profiles/r03c_local_predictor.json.  Interleaved repetitions after a warm-up of
every case, medians; the universal call's per-stage split from ck_timings [48 ..].

    python scripts/bench_local_universal.py [--reps 5] [--radii 125 400 600] [--out profiles/<round>_local_universal.json]
        [--other-lib <libcokrige_hip.so of another commit>]

--other-lib: the no-trend call is also timed on that library (a child process that loads it, before and after this process's
own repetitions), e.g. the parent commit's build, to show that ck_predict_local has not moved.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402
from sif_xco2_cokriging_amd.trend import TrendDesign  # noqa: E402


def other_lib_run(a):
    """the no-trend rows on another build of the library: {radius: [ms, ...]}"""
    env = dict(os.environ, CK_LIB_PATH=a.other_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--simple-only", "--n", str(a.n), "--reps", str(a.reps), "--radii"]
    r = subprocess.run(cmd + [str(x) for x in a.radii], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"the run on {a.other_lib} failed:\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radii", type=float, nargs="+", default=[125.0, 400.0, 600.0])
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--simple-only", action="store_true", help="time predict_local only and print {radius: [ms]} (child mode)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    before = other_lib_run(a) if a.other_lib else None   # before this process opens the GPU
    if a.simple_only:   # the library under CK_LIB_PATH may be an older commit's: bind only what it exports
        import ctypes
        old = ctypes.CDLL(native.LIB_PATH)
        for name in [k for k in native._PROTOS if not hasattr(old, k)]:
            del native._PROTOS[name]
    pb = synth.conus_problem(a.n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.local_reserve(0)   # the scratch slab once, at the automatic budget: no timed call grows it
    pc = pb["pcoords"]
    designs = {t: TrendDesign(t, [np.asarray(c)[:, :2] for c in pb["coords"]]) for t in ("constant", "linear")}
    F = {t: [d.data(k, np.asarray(pb["coords"][k])[:, :2]) for k in range(2)] for t, d in designs.items()}
    F0 = {t: d(0, pc) for t, d in designs.items()}

    def universal(t, md):
        for k in range(2):
            h.set_trend(k, F[t][k])
        return h.predict_local_universal(0, pc, F0[t], max_dist=md)

    cases = {"none": lambda md: h.predict_local(0, pc, md)}
    if not a.simple_only:
        for t in designs:
            cases[t] = (lambda md, t=t: universal(t, md))
    rows = []
    for md in a.radii:
        for f in cases.values():   # warm-up of every case
            f(md)
        wall = {k: [] for k in cases}
        dev = {k: [] for k in cases}
        stages = {k: [] for k in cases}
        info = {}
        for _ in range(a.reps):
            for k, f in cases.items():
                t0 = time.perf_counter()
                res = f(md)
                wall[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(h.timings()["local_ms"])
                info[k] = {x: int(v) for x, v in res[2].items()}
                if k != "none":
                    stages[k].append(h.local_universal_timings())
        row = {"max_dist_km": md, "points": len(pc), "k_max": info["none"]["k_max"], "cases": {}}
        for k in cases:
            c = {"wall_ms_median": float(np.median(wall[k])), "wall_ms": [round(x, 3) for x in wall[k]],
                 "device_ms_median": float(np.median(dev[k])), "info": info[k]}
            if stages[k]:
                c.update({s: float(np.median([x[s] for x in stages[k]])) for s in stages[k][0]})
            if k != "none":
                c["wall_over_none"] = c["wall_ms_median"] / float(np.median(wall["none"]))
            row["cases"][k] = c
        w = np.asarray(wall["none"])
        row["none_spread_rel"] = float((w.max() - w.min()) / np.median(w))   # run-to-run noise of the same call in this run
        rows.append(row)
    h.close()
    if a.simple_only:
        print(json.dumps({str(r["max_dist_km"]): r["cases"]["none"]["wall_ms"] for r in rows}), flush=True)
        return
    out = {"n_obs": 2 * a.n, "reps": a.reps, "p": {"constant": 2, "linear": 6}, "rows": rows}
    if a.other_lib:
        after = other_lib_run(a)
        for r in rows:
            ms = before[str(r["max_dist_km"])] + after[str(r["max_dist_km"])]
            r["other_lib_none"] = {"wall_ms_median": float(np.median(ms)), "wall_ms": ms,
                                   "none_over_other": r["cases"]["none"]["wall_ms_median"] / float(np.median(ms))}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
