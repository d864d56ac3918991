"""Block cokriging (ck_predict_blocks) against the point sweep on the resident factor at N = 40 000 (the 8 833-point
0.5-degree grid): blocks of 1-degree cells (r = 2 257), 5-degree cells, 30-degree latitude bands (the larger holds 6 897
sites), one whole-domain mean, and 1-degree cells with the r x r covariance.
Interleaved repetitions after a warm-up of every shape; the per-stage split from ck_timings [16 ..]; the fold kernel's
bytes (member rows read + block rows written) over its time against the 8 TB/s HBM peak.

    python scripts/bench_blocks.py [--reps 5] [--out profiles/<round>_blocks.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402

HBM_PEAK_TBS = 8.0


def cells(pc, deg):
    key = np.floor(pc[:, 0] / deg).astype(np.int64) * 100000 + np.floor(pc[:, 1] / deg).astype(np.int64)
    uniq, lab = np.unique(key, return_inverse=True)
    return lab.astype(np.int32), len(uniq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process (N = 2 n)")
    ap.add_argument("--reps", type=int, default=5)
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
    lab1, r1 = cells(pc, 1.0)
    lab5, r5 = cells(pc, 5.0)
    w1 = 1.0 / np.bincount(lab1)[lab1]
    w5 = 1.0 / np.bincount(lab5)[lab5]
    lab30 = (np.floor(pc[:, 0] / 30.0).astype(np.int64) - int(np.floor(pc[:, 0].min() / 30.0))).astype(np.int32)
    r30 = int(lab30.max()) + 1
    w30 = 1.0 / np.bincount(lab30)[lab30]
    lab_all = np.zeros(m, dtype=np.int32)
    w_all = np.full(m, 1.0 / m)
    cases = {
        "point": lambda: h.predict(0, pc),
        "blocks_1deg": lambda: h.predict_blocks(0, pc, lab1, w1, r1),
        "blocks_5deg": lambda: h.predict_blocks(0, pc, lab5, w5, r5),
        "blocks_30deg_bands": lambda: h.predict_blocks(0, pc, lab30, w30, r30),
        "blocks_whole_domain": lambda: h.predict_blocks(0, pc, lab_all, w_all, 1),
        "blocks_1deg_cov": lambda: h.predict_blocks(0, pc, lab1, w1, r1, want_cov=True),
    }
    rows = {"point": m, "blocks_1deg": r1, "blocks_5deg": r5, "blocks_30deg_bands": r30, "blocks_whole_domain": 1,
            "blocks_1deg_cov": r1}
    sizes = {"blocks_1deg": lab1, "blocks_5deg": lab5, "blocks_30deg_bands": lab30, "blocks_whole_domain": lab_all,
             "blocks_1deg_cov": lab1}
    for f in cases.values():   # warm-up of every shape
        f()
    wall = {k: [] for k in cases}
    stages = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            stages[k].append(h.timings())
    out = {"n_obs": 2 * a.n, "n_padded": n_pad, "m": m, "reps": a.reps, "cases": {}}
    for k in cases:
        t = stages[k]
        med = lambda key: float(np.median([x[key] for x in t]))  # noqa: E731
        c = {"rows": rows[k], "wall_ms_median": float(np.median(wall[k])), "wall_ms_min": float(np.min(wall[k])),
             "wall_ms": [round(x, 3) for x in wall[k]]}
        if k == "point":
            c.update(assemble_ms=med("assemble_aux_ms"), solve_ms=med("solve_ms"), reduce_ms=med("reduce_ms"))
        else:
            c.update({s: med("blocks_" + s) for s in ("assemble_ms", "fold_ms", "prior_ms", "solve_ms", "reduce_ms",
                                                      "total_ms", "chunks")})
            fold_bytes = (m + rows[k] + 1) * n_pad * 8   # member rows read, block rows (+ data row) written
            n_b = np.bincount(sizes[k])
            c["largest_block"] = int(n_b.max())
            c["prior_pairs_diagonal"] = int(np.sum(n_b.astype(np.int64) ** 2))
            c["fold_bytes"] = fold_bytes
            c["fold_tb_per_s"] = fold_bytes / (c["fold_ms"] / 1e3) / 1e12
            c["fold_frac_of_hbm_peak"] = c["fold_tb_per_s"] / HBM_PEAK_TBS
        out["cases"][k] = c
    p = out["cases"]["point"]
    for k in ("blocks_1deg", "blocks_5deg", "blocks_30deg_bands", "blocks_whole_domain", "blocks_1deg_cov"):
        out["cases"][k]["solve_over_point_solve"] = out["cases"][k]["solve_ms"] / p["solve_ms"]
        out["cases"][k]["wall_over_point_wall"] = out["cases"][k]["wall_ms_median"] / p["wall_ms_median"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    h.close()


if __name__ == "__main__":
    main()
