"""GPU measurements of the conditional simulation in the moving neighbourhood (ck_simulate_local; DESIGN 5g-4,
profiles/r13_local_simulation.json).

    python scripts/bench_local_simulation.py [main] [scale] [--out file.json]

main   conus_problem(20000): the 8 833 sites of the 0.5-degree grid on 40 000 observations, 400 km, caps (16, 16), random
       ordering, 100 and 1 000 draws -- per stage (ck_timings [110 ..]) and end to end, against two baselines in the same
       process, interleaved: the local point call with the same caps, and the joint predictor's conditional draws on the same
       sites from its resident factor (the factorisation is timed once, apart).  The Hilbert ordering's level count and time are
       recorded beside the random one's.
scale  the same sites on the 2 x 250 000 observations of conus_problem(250000), 60 km, caps (16, 16), 100 draws
One warm-up, then interleaved repetitions."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

REPS = 3
CAPS = (16, 16)


def spread(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def handle(pb):
    from sif_xco2_cokriging_amd import native
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    return h


def simulate(h, pb, ranks, max_dist, n_draws, rows):
    t0 = time.perf_counter()
    draws, info, st = h.simulate_local(0, pb["pcoords"], ranks, max_dist, n_draws, seed=1, terms=False)
    wall = 1e3 * (time.perf_counter() - t0)
    rows.append(dict(h.simulate_local_timings(), wall_ms=wall))
    return draws, info, st


STAGES = ["select_ms", "weights_ms", "levels_ms", "recursion_ms", "total_ms", "wall_ms"]


def summary(rows, st, info, draws):
    tm = rows[-1]
    return dict(first_call=rows[0], **{k: spread([r[k] for r in rows[1:]]) for k in STAGES}, info=int(info), n_levels=st["n_levels"],
                n_empty=st["n_empty"], k_max=st["k_max"], n_capped=st["n_capped"], n_site_neighbours=int(tm["n_site_neighbours"]),
                n_solved=int(tm["n_solved"]), draws_finite=bool(np.all(np.isfinite(draws))), ensemble_sd_mean=float(draws.std(axis=0).mean()))


def main_case(max_dist=400.0):
    from sif_xco2_cokriging_amd import synth, vecchia
    pb = synth.conus_problem(20000)
    m = len(pb["pcoords"])
    ranks = {o: vecchia.ordering_ranks([pb["pcoords"]], o, 0) for o in ("random", "hilbert")}
    h = handle(pb)
    h.set_local_neighbours(*CAPS)
    hj = handle(pb)
    t0 = time.perf_counter()
    hj.assemble_joint()
    assert hj.factor() == 0
    joint_factor_ms = 1e3 * (time.perf_counter() - t0)
    cells = [("random", 100), ("random", 1000), ("hilbert", 100)]
    acc = {c: [] for c in cells}
    last = {}
    point_ms, joint_ms = [], {100: [], 1000: []}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        pred, err, pinfo = h.predict_local(0, pb["pcoords"], max_dist=max_dist)
        if rep:
            point_ms.append(1e3 * (time.perf_counter() - t0))
        for o, nd in cells:
            last[o, nd] = simulate(h, pb, ranks[o], max_dist, nd, acc[o, nd])
        for nd in joint_ms:
            t0 = time.perf_counter()
            jd = hj.conditional_draws(0, pb["pcoords"], nd, seed=1)
            assert jd[4] == 0
            if rep:
                joint_ms[nd].append(1e3 * (time.perf_counter() - t0))
    out = dict(n_obs=40000, m=m, max_dist_km=max_dist, caps=list(CAPS), local_point_call_ms=spread(point_ms),
               local_point_call=dict(k_max=pinfo["k_max"], n_empty=pinfo["n_empty"]), joint_factor_ms=joint_factor_ms,
               joint_conditional_draws_ms={str(nd): spread(v) for nd, v in joint_ms.items()},
               joint_ensemble_sd_mean=float(jd[0].std(axis=0).mean()),
               cells=[dict(ordering=o, n_draws=nd, **summary(acc[o, nd], last[o, nd][2], last[o, nd][1], last[o, nd][0])) for o, nd in cells])
    h.close()
    hj.close()
    return out


def scale_case(n_per_process=250000, max_dist=60.0, n_draws=100):
    from sif_xco2_cokriging_amd import synth, vecchia
    t0 = time.perf_counter()
    pb = synth.conus_problem(n_per_process)
    h = handle(pb)
    h.set_local_neighbours(*CAPS)
    ranks = vecchia.ordering_ranks([pb["pcoords"]], "random", 0)
    setup_s = time.perf_counter() - t0
    rows, point_ms = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        h.predict_local(0, pb["pcoords"], max_dist=max_dist)
        if rep:
            point_ms.append(1e3 * (time.perf_counter() - t0))
        draws, info, st = simulate(h, pb, ranks, max_dist, n_draws, rows)
    h.close()
    return dict(n_per_process=n_per_process, m=len(pb["pcoords"]), max_dist_km=max_dist, caps=list(CAPS), ordering="random",
                n_draws=n_draws, setup_s=setup_s, local_point_call_ms=spread(point_ms), **summary(rows, st, info, draws))


if __name__ == "__main__":
    args = sys.argv[1:]
    path = args[args.index("--out") + 1] if "--out" in args else None
    out = {"repetitions": REPS}

    def save(key, value):
        out[key] = value
        print(json.dumps({key: value}), flush=True)
        if path:
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    if "main" in args or not [a for a in args if a in ("main", "scale")]:
        save("conus_20000", main_case())
    if "scale" in args:
        save("conus_250000", scale_case())
