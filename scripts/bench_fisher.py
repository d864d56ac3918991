"""The Fisher information of the likelihood fit (ck_loglik_fisher) on the CONUS lattice at N = 10 000 and 40 000, bivariate,
all eleven parameters live: wall clock of assemble + call, ck_loglik's stages inside it (ck_timings [24 ..]: factorisation,
unit-row sweep, Sigma^-1) and the call's own (ck_timings [64 ..]: derivative assembly, products, contraction), the flop the
products executed and their rate against the 78.6 TFLOP/s FP64 matrix peak.  Beside it, in the same process, the
differenced-gradient route to the same end: 2 x n_live evaluations of assemble + ck_loglik(want_grad = 1), timed as one loop
(the parameters stay where they are: the cost of an evaluation does not depend on them).
Interleaved repetitions after a warm-up of each form.

    python scripts/bench_fisher.py [--reps 3] [--out profiles/r05_fisher.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402

PEAK_TF = 78.6
N_LIVE = 11


def loaded(n):
    pb = synth.conus_problem(n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(pb["metric"])
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000", help="sites per process (N = 2 n)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        h = loaded(n)
        N = 2 * n
        fisher_runs, diff_wall = [], []
        diag = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            h.assemble_joint()
            info, I = h.fisher()
            wall = (time.perf_counter() - t0) * 1e3
            assert info == 0 and np.all(np.isfinite(I)) and np.array_equal(I, I.T)
            t = h.fisher_timings()
            t.update({"lik_" + k: v for k, v in h.loglik_timings().items() if k in ("factor_ms", "sweep_ms", "syrk_ms")})
            t["wall_ms"] = wall
            t0 = time.perf_counter()
            for _ in range(2 * N_LIVE):
                h.assemble_joint()
                info, out3, g = h.loglik(True)
                assert info == 0
            dw = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                diag = np.diag(I)[:N_LIVE].tolist()
                continue
            fisher_runs.append(t)
            diff_wall.append(dw)
        med = {k: float(np.median([r[k] for r in fisher_runs])) for k in fisher_runs[0]}
        row = {"n_per_process": n, "N": N, "n_live": N_LIVE, "information_diagonal": diag, "median_ms": med,
               "product_flop": med["flop"], "product_flop_over_N3": med["flop"] / float(N) ** 3,
               "product_tflops": med["flop"] / (med["product_ms"] * 1e-3) / 1e12,
               "product_mfma_fraction": med["flop"] / (med["product_ms"] * 1e-3) / 1e12 / PEAK_TF,
               "differenced_gradient_evaluations": 2 * N_LIVE,
               "differenced_gradient_wall_ms": float(np.median(diff_wall)),
               "speedup_over_differenced_gradient": float(np.median(diff_wall)) / med["wall_ms"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        h.close()
    out = {"benchmark": "ck_loglik_fisher", "peak_tflops": PEAK_TF, "reps": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
