"""GPU benchmark of both processes in the moving neighbourhood: ck_predict_local_pair against ck_predict_local(0) +
ck_predict_local(1) on the same handle, and ck_simulate_local_pair against two ck_simulate_local calls.  bench_local.py's inputs:
the 8 833 sites of the 0.5-degree grid on 2 x 20 000 observations; uncapped at 50, 100 and 400 km (the LDS class, a mix, the
tiled class) and at 400 km with caps (16, 16).  The variants are interleaved in one process: one warm-up per shape, then three
repetitions of (pair, single 0, single 1), medians per stage.  The co-simulation (caps (16, 16), 400 km, sets of at most 64)
with 100 and 1 000 draws, both processes at the same sites.

    python scripts/bench_local_pair.py [sites per process, default 20000] [--out profiles/r17_local_pair.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = [(50.0, None), (100.0, None), (400.0, None), (400.0, (16, 16))]
DRAWS = [100, 1000]
REPS = 3


def med(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def wall(f):
    t = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t) * 1e3


def main():
    args = [a for a in sys.argv[1:]]
    out_path = None
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    n = int(args[0]) if args else 20000
    from sif_xco2_cokriging_amd import native, synth
    pb = synth.conus_problem(n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(0)
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.local_reserve(0)   # the scratch slab once: no timed call grows it
    pc = np.ascontiguousarray(pb["pcoords"], dtype=np.float64)
    res = dict(what="ck_predict_local_pair against ck_predict_local(0) + ck_predict_local(1), ck_simulate_local_pair against two "
                    "ck_simulate_local calls, on the MI355X (milliseconds); written by scripts/bench_local_pair.py: one warm-up, "
                    f"{REPS} interleaved repetitions, medians", n_obs=2 * n, m=len(pc), repetitions=REPS, prediction=[], simulation=[])

    def single(i, md):
        (_, _, info), w = wall(lambda: h.predict_local(i, pc, max_dist=md))
        return dict(device_ms=h.timings()["local_ms"], wall_ms=w, k_max=info["k_max"])

    def pair(md):
        (*_, info), w = wall(lambda: h.predict_local_pair(pc, max_dist=md))
        t = h.local_pair_timings()
        return dict(pass_ms=t["pass_ms"], solve_ms=t["solve_ms"], device_ms=t["pass_ms"] + t["solve_ms"], wall_ms=w, n_tiled=t["n_tiled"],
                    k_max=info["k_max"], n_empty=info["n_empty"])

    for md, caps in SHAPES:
        h.set_local_neighbours(*(caps or (0, 0)))
        pair(md), single(0, md), single(1, md)   # warm-up
        rows = [(pair(md), single(0, md), single(1, md)) for _ in range(REPS)]
        cell = dict(max_dist_km=md, caps=caps, k_max=rows[0][0]["k_max"], n_empty=rows[0][0]["n_empty"], n_tiled=rows[0][0]["n_tiled"],
                    pair_pass_ms=med([r[0]["pass_ms"] for r in rows]), pair_solve_ms=med([r[0]["solve_ms"] for r in rows]),
                    pair_device_ms=med([r[0]["device_ms"] for r in rows]), pair_wall_ms=med([r[0]["wall_ms"] for r in rows]),
                    single0_device_ms=med([r[1]["device_ms"] for r in rows]), single1_device_ms=med([r[2]["device_ms"] for r in rows]),
                    singles_device_ms=med([r[1]["device_ms"] + r[2]["device_ms"] for r in rows]),
                    singles_wall_ms=med([r[1]["wall_ms"] + r[2]["wall_ms"] for r in rows]))
        cell["ratio_device"] = cell["pair_device_ms"]["median"] / cell["singles_device_ms"]["median"]
        cell["ratio_wall"] = cell["pair_wall_ms"]["median"] / cell["singles_wall_ms"]["median"]
        res["prediction"].append(cell)
        print(f"{md:5.0f} km caps {caps}: pair {cell['pair_device_ms']['median']:9.2f} ms (pass {cell['pair_pass_ms']['median']:.2f}, "
              f"solve {cell['pair_solve_ms']['median']:.2f}), singles {cell['singles_device_ms']['median']:9.2f} ms, ratio "
              f"{cell['ratio_device']:.3f} device / {cell['ratio_wall']:.3f} wall, k_max {cell['k_max']}, tiled {cell['n_tiled']:.0f}",
              flush=True)

    # co-simulation: both processes at the grid's sites, caps (16, 16) at 400 km
    h.set_local_neighbours(16, 16)
    m = len(pc)
    rng = np.random.default_rng(0)
    ranks2 = rng.permutation(2 * m).astype(np.int64)
    ranks1 = [rng.permutation(m).astype(np.int64) for _ in range(2)]

    def cosim(nd):
        (_, info, st), w = wall(lambda: h.simulate_local_pair(pc, pc, ranks2, 400.0, nd, seed=1, terms=False))
        assert info == 0
        return dict(h.simulate_local_timings(), wall_ms=w, k_max=st["k_max"])

    def sim(i, nd):
        (_, info, st), w = wall(lambda: h.simulate_local(i, pc, ranks1[i], 400.0, nd, seed=1, terms=False))
        assert info == 0
        return dict(h.simulate_local_timings(), wall_ms=w, k_max=st["k_max"])

    stages = ["select_ms", "weights_ms", "levels_ms", "recursion_ms", "total_ms", "wall_ms"]
    for nd in DRAWS:
        cosim(nd), sim(0, nd), sim(1, nd)   # warm-up
        rows = [(cosim(nd), sim(0, nd), sim(1, nd)) for _ in range(REPS)]
        cell = dict(n_draws=nd, max_dist_km=400.0, caps=(16, 16), pair_k_max=rows[0][0]["k_max"], pair_n_levels=rows[0][0]["n_levels"],
                    single_n_levels=[rows[0][1]["n_levels"], rows[0][2]["n_levels"]],
                    pair={s: med([r[0][s] for r in rows]) for s in stages},
                    singles={s: med([r[1][s] + r[2][s] for r in rows]) for s in stages})
        cell["ratio_total"] = cell["pair"]["total_ms"]["median"] / cell["singles"]["total_ms"]["median"]
        res["simulation"].append(cell)
        print(f"{nd:5d} draws: co-simulation {cell['pair']['total_ms']['median']:9.2f} ms, two single calls "
              f"{cell['singles']['total_ms']['median']:9.2f} ms, ratio {cell['ratio_total']:.3f}; levels {cell['pair_n_levels']:.0f} "
              f"against {cell['single_n_levels']}", flush=True)
    h.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
        print("written", out_path)


if __name__ == "__main__":
    main()
