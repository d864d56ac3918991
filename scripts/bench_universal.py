"""Universal cokriging and REML against simple cokriging and ML on one resident factor at N = 40 000 (the 8 833-point
0.5-degree grid): ck_predict against ck_predict_universal, and ck_loglik against ck_loglik_reml (value, and value with the
gradient), for no trend, "constant" (p = 2) and "linear" (p = 6).  Interleaved repetitions after a warm-up of every case;
the universal call's per-stage split from ck_timings [40 ..].

    python scripts/bench_universal.py [--reps 3] [--no-grad] [--out profiles/<round>_universal.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402
from sif_xco2_cokriging_amd.trend import TrendDesign  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process (N = 2 n)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-grad", action="store_true", help="skip the likelihood gradients")
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
    info, _, _ = h.factor_predict(0, pc)
    assert info == 0
    designs = {"none": None}
    for t in ("constant", "linear"):
        designs[t] = TrendDesign(t, [np.asarray(c)[:, :2] for c in pb["coords"]])

    def use(t):
        d = designs[t]
        for k in range(2):
            h.set_trend(k, None if d is None else d.data(k, np.asarray(pb["coords"][k])[:, :2]))
        return None if d is None else d(0, pc)

    def lik(fn, grad):
        h.assemble_joint()   # ck_loglik factors its Sigma itself: the likelihood of a fit step
        r = fn(grad)
        assert r[0] == 0
        return r

    cases = {"predict": lambda: (use("none"), h.predict(0, pc))}
    for t in ("constant", "linear"):
        cases[f"universal_{t}"] = (lambda t=t: h.predict_universal(0, pc, use(t)))
    for g in ([False] if a.no_grad else [False, True]):
        sfx = "_grad" if g else ""
        cases[f"loglik{sfx}"] = (lambda g=g: (use("none"), lik(h.loglik, g)))
        for t in ("constant", "linear"):
            cases[f"reml_{t}{sfx}"] = (lambda t=t, g=g: (use(t), lik(h.loglik_reml, g)))
    # the likelihood cases leave Sigma refactored: the prediction cases come first in every repetition, on the factor of
    # the last likelihood call (the same Sigma)
    for f in cases.values():
        f()
    wall = {k: [] for k in cases}
    stages = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if k.startswith("universal"):
                stages[k].append(h.universal_timings())
            elif k.startswith(("loglik", "reml")):
                stages[k].append(h.loglik_timings())
    out = {"n_obs": 2 * a.n, "n_padded": h.num_panels()[2], "m": m, "reps": a.reps,
           "p": {"constant": 2, "linear": 6}, "cases": {}}
    for k in cases:
        c = {"wall_ms_median": float(np.median(wall[k])), "wall_ms_min": float(np.min(wall[k])),
             "wall_ms": [round(x, 3) for x in wall[k]]}
        if stages[k]:
            c.update({s: float(np.median([x[s] for x in stages[k]])) for s in stages[k][0]})
        base = "predict" if k.startswith("universal") else ("loglik_grad" if k.endswith("_grad") else "loglik")
        if k != base:
            c["wall_over_" + base] = c["wall_ms_median"] / float(np.median(wall[base]))
        out["cases"][k] = c
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    h.close()


if __name__ == "__main__":
    main()
