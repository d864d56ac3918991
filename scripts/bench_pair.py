"""Joint prediction of both processes (ck_predict_pair, ck_conditional_draws_pair) against the single-process calls it
replaces, on the resident factor at N = 40 000 with the 8 833-point 0.5-degree grid as the sites of BOTH processes: the pair
call against ck_predict(0) + ck_predict(1), and 100 / 1 000 joint draws against the two single-process draw calls.  One
process, variants interleaved, medians after a warm-up of every shape; the per-stage split from ck_timings ([2 .. 4] of the
point calls, [134 ..] of the pair call, [30 ..] / [124 ..] of the draws).

    python scripts/bench_pair.py [--reps 3] [--out profiles/<round>_pair.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sif_xco2_cokriging_amd import native, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000, help="sites per process (N = 2 n)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", default="100,1000")
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
    co = np.column_stack([np.arange(m)] * 2)
    point_keys = ["assemble_aux_ms", "solve_ms", "reduce_ms"]

    def two_points():
        st = {}
        for i in range(2):
            h.predict(i, pc)
            t = h.timings()
            for s in point_keys:
                st[s] = st.get(s, 0.0) + t[s]
        return st

    def pair():
        h.predict_pair(pc, pc, co)
        t = h.pair_timings()
        return {s: t[s] for s in ("pair_assemble_ms", "pair_sweep_ms", "pair_reduce_ms", "pair_total_ms")}

    def two_draws(nd):
        st = {}
        for i in range(2):
            assert h.conditional_draws(i, pc, nd, seed=1)[4] == 0
            for s, v in h.draws_timings().items():
                st[s] = st.get(s, 0.0) + v
        return st

    def pair_draws(nd):
        assert h.conditional_draws_pair(pc, pc, nd, seed=1)[4] == 0
        return h.pair_timings()

    cases = {"two_point_calls": two_points, "pair_call": pair}
    for nd in [int(x) for x in a.draws.split(",")]:
        cases[f"two_draw_calls_{nd}"] = (lambda nd=nd: two_draws(nd))
        cases[f"pair_draws_{nd}"] = (lambda nd=nd: pair_draws(nd))
    for f in cases.values():   # warm-up of every shape
        f()
    wall = {k: [] for k in cases}
    stages = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():
            t0 = time.perf_counter()
            st = f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            stages[k].append(st)
    out = {"n_obs": 2 * a.n, "n_padded": h.num_panels()[2], "m0": m, "m1": m, "reps": a.reps, "cases": {}}
    for k in cases:
        c = {"wall_ms_median": float(np.median(wall[k])), "wall_ms_min": float(np.min(wall[k])),
             "wall_ms": [round(x, 3) for x in wall[k]]}
        c.update({s: float(np.median([x[s] for x in stages[k]])) for s in stages[k][0]})
        out["cases"][k] = c
    cs = out["cases"]
    out["pair_over_two_point_calls"] = cs["pair_call"]["wall_ms_median"] / cs["two_point_calls"]["wall_ms_median"]
    for nd in [int(x) for x in a.draws.split(",")]:
        out[f"pair_draws_over_two_draw_calls_{nd}"] = cs[f"pair_draws_{nd}"]["wall_ms_median"] / cs[f"two_draw_calls_{nd}"]["wall_ms_median"]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    h.close()


if __name__ == "__main__":
    main()
