"""Conditional simulation (ck_conditional_draws) against the point call on the resident factor at N = 40 000 (the 8 833-point
0.5-degree grid), with 1, 100 and 1 000 draws (and 1 024, the draw product's full tiles) from the device's Philox stream.
Interleaved repetitions after a warm-up of every shape; the per-stage split from ck_timings [30 ..]; the draw product's
flop (m^2 n_draws: the lower tiles of X = E L_S^T) over its own kernel time against the 78.6 TF FP64 MFMA peak.

    python scripts/bench_conditional.py [--reps 3] [--out profiles/<round>_conditional.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402

MFMA_PEAK_TF = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process (N = 2 n)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", default="1,100,1000,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pb = synth.conus_problem(a.n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.assemble_joint()
    pc = pb["pcoords"]
    m = len(pc)
    info, pred, err = h.factor_predict(0, pc)
    assert info == 0
    n_pad = h.num_panels()[2]
    cases = {"point": lambda: h.predict(0, pc)}
    for nd in [int(x) for x in a.draws.split(",")]:
        cases[f"draws_{nd}"] = (lambda nd=nd: h.conditional_draws(0, pc, nd, seed=1))
    for f in cases.values():   # warm-up of every shape
        f()
    wall = {k: [] for k in cases}
    stages = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():
            t0 = time.perf_counter()
            r = f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if k != "point":
                assert r[4] == 0
                stages[k].append(h.draws_timings())
    out = {"n_obs": 2 * a.n, "n_padded": n_pad, "m": m, "reps": a.reps, "mfma_peak_tf": MFMA_PEAK_TF, "cases": {}}
    for k in cases:
        c = {"wall_ms_median": float(np.median(wall[k])), "wall_ms_min": float(np.min(wall[k])),
             "wall_ms": [round(x, 3) for x in wall[k]]}
        if k != "point":
            t = stages[k]
            c.update({s: float(np.median([x[s] for x in t])) for s in t[0]})
            nd = int(k.split("_")[1])
            c["n_draws"] = nd
            c["product_flop"] = float(m) * m * nd
            c["product_tflops"] = c["product_flop"] / (c["product_ms"] / 1e3) / 1e12
            c["product_frac_of_mfma_peak"] = c["product_tflops"] / MFMA_PEAK_TF
            c["wall_over_point_wall"] = c["wall_ms_median"] / float(np.median(wall["point"]))
        out["cases"][k] = c
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    h.close()


if __name__ == "__main__":
    main()
