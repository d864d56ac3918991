"""Leave-group-out cross-validation from ONE factorisation (ck_cv_folds) at the headline size, next to ck_loocv on the same
handle: per-stage times from ck_timings for four fold layouts of process 0.

    python scripts/bench_cv_folds.py [n_per_process = 20000] [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sif_xco2_cokriging_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
pb = synth.conus_problem(n)
pv = pb["params"]
h = native.Handle(0)
h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
h.set_metric(0)
for k in range(2):
    h.set_data(k, pb["coords"][k], pb["values"][k])
h.assemble_joint()
assert h.factor() == 0
c0, c1 = pb["coords"]
rng = np.random.default_rng(0)
kfold = np.empty(n, dtype=np.int32)
kfold[rng.permutation(n)] = np.arange(n) * 10 // n
# spatial blocks: a 20 x 20 grid over the sites' bounding box, empty cells dropped
gx = np.minimum((20 * (c0[:, 0] - c0[:, 0].min()) / np.ptp(c0[:, 0])).astype(int), 19)
gy = np.minimum((20 * (c0[:, 1] - c0[:, 1].min()) / np.ptp(c0[:, 1])).astype(int), 19)
blocks = np.unique(gx * 20 + gy, return_inverse=True)[1].astype(np.int32)
# the co-located partners of process 1 leave with their process-0 datum's fold
where = {tuple(c): a for a, c in enumerate(c0)}
partner = np.array([where.get(tuple(c), -1) for c in c1])
also = np.where(partner >= 0, kfold[np.maximum(partner, 0)], -1).astype(np.int32)
layouts = [("kfold10", kfold, None), ("blocks400", blocks, None), ("singletons", np.arange(n, dtype=np.int32), None),
           ("kfold10_with_partner", kfold, also)]
rows = []
for rep in range(2):
    t0 = time.perf_counter()
    lp, le = h.loocv(0, n)
    rows.append({"layout": "ck_loocv", "rep": rep, "n_obs": n, "seconds": time.perf_counter() - t0, "sweep_ms": h.timings()["solve_ms"]})
    print(json.dumps(rows[-1]), flush=True)
    for name, fi, fo in layouts:
        t0 = time.perf_counter()
        info, pred, err = h.cv_folds(0, fi, fo)
        dt = time.perf_counter() - t0
        t = h.cv_folds_timings()
        sizes = np.bincount(fi, minlength=int(fi.max()) + 1) + (0 if fo is None else np.bincount(fo[fo >= 0], minlength=int(fi.max()) + 1))
        row = {"layout": name, "rep": rep, "n_obs": n, "n_folds": int(fi.max()) + 1, "largest_fold": int(sizes.max()), "info": info,
               "seconds": dt, **t, "solve_share": t["solve_ms"] / t["total_ms"],
               "rmse": float(np.sqrt(np.mean((pred - pb["values"][0]) ** 2))), "checksum": float(pred.sum())}
        if name == "singletons":
            row["max_abs_diff_to_loocv"] = float(np.max(np.abs(pred - lp)))
        rows.append(row)
        print(json.dumps(row), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
