"""The Gaussian log-likelihood (ck_loglik) on the CONUS lattice at N = 10 000 and 40 000: l alone and l + gradient, broken
down by ck_timings [24 ..] (assembly, factorisation, unit-row sweep, G = alpha alpha^T - Sigma^-1, contraction, host wall
clock), with the MFMA fraction of the sweep and of the SYRK against the 78.6 TFLOP/s FP64 matrix peak.
Flop counts: factor N^3 / 3; the unit-row sweep (rows of the LOOCV layout over all N data, on the growing live prefix)
N^3 / 3; the SYRK over the lower tiles with the structurally zero panels skipped N^3 / 3.
Interleaved repetitions after a warm-up of each form.

    python scripts/bench_likelihood.py [--reps 3] [--out profiles/r05_likelihood.json]
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
        runs = {"loglik": [], "loglik_grad": []}
        vals = {}
        for rep in range(a.reps + 1):
            for form, grad in (("loglik", False), ("loglik_grad", True)):
                t0 = time.perf_counter()
                h.assemble_joint()
                info, out3, g = h.loglik(grad)
                wall = (time.perf_counter() - t0) * 1e3
                assert info == 0 and np.isfinite(out3[0])
                if rep == 0:
                    vals[form] = {"l": out3[0], "logdet": out3[1], "quad": out3[2],
                                  "grad": None if g is None else g.tolist()}
                    continue
                t = h.loglik_timings()
                t["wall_ms"] = wall
                runs[form].append(t)
        med = {form: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for form, rs in runs.items()}
        gt = med["loglik_grad"]
        flop3 = N ** 3 / 3.0
        row = {"n_per_process": n, "N": N, "values": vals, "median_ms": med,
               "sweep_tflops": flop3 / (gt["sweep_ms"] * 1e-3) / 1e12,
               "sweep_mfma_fraction": flop3 / (gt["sweep_ms"] * 1e-3) / 1e12 / PEAK_TF,
               "syrk_tflops": flop3 / (gt["syrk_ms"] * 1e-3) / 1e12,
               "syrk_mfma_fraction": flop3 / (gt["syrk_ms"] * 1e-3) / 1e12 / PEAK_TF,
               "factor_mfma_fraction": flop3 / (gt["factor_ms"] * 1e-3) / 1e12 / PEAK_TF if gt["factor_ms"] > 0 else None}
        print(json.dumps({k: v for k, v in row.items() if k != "values"}), flush=True)
        rows.append(row)
        h.close()
    out = {"benchmark": "ck_loglik", "peak_tflops": PEAK_TF, "reps": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
