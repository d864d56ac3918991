"""GPU measurements of the Vecchia likelihood with a GLS trend (ck_loglik_vecchia_trend / _trend_grad; DESIGN 5d-5,
profiles/r12_vecchia_trend.json).

    python scripts/bench_vecchia_trend.py [calls] [fit] [--out file.json]

calls   conus_problem with set A, caps (16,16), random ordering, at N = 40 000 (800 km) and N = 2 x 250 000 (60 km): the value
        call and the gradient call with p = 2 ("constant") and p = 6 ("linear") against ck_loglik_vecchia and
        ck_loglik_vecchia_grad on the same data, ranks and caps (a handle without the trend).  Host wall clock of the call and
        the stages of ck_timings [96 ..] / [80 ..] / [72 ..].
fit     N = 40 000, sigma_11, len_scale_11 and nugget_11 free from a displaced start, a constant mean per process in the data:
        evaluations, native calls and wall clock of fit_likelihood with Vecchia(trend="constant") under gradient="numeric" and
        under gradient="analytic"
One warm-up, then interleaved repetitions in one process, medians, the slab reserved (as bench_vecchia.py)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

from bench_vecchia import handle, spread  # noqa: E402

REPS = 3
CAPS = (16, 16)


def calls(n_per_process, max_dist):
    from sif_xco2_cokriging_amd import synth, vecchia
    from sif_xco2_cokriging_amd.trend import TrendDesign
    pb = synth.conus_problem(n_per_process)
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 0)
    hs = {}
    for tag in ("none", "constant", "linear"):
        hs[tag] = handle(pb)
        hs[tag].local_reserve(0)
        hs[tag].set_local_neighbours(*CAPS)
        if tag != "none":
            design = TrendDesign(tag, pb["coords"])
            for k in range(2):
                hs[tag].set_trend(k, design.data(k, pb["coords"][k]))
    cells = ["value", "grad", "value_p2", "grad_p2", "value_p6", "grad_p6"]
    acc = {c: [] for c in cells}
    last = {}
    for rep in range(REPS + 1):          # rep 0: the warm-up of every shape
        for c in cells:
            h = hs["none" if "_" not in c else "constant" if c.endswith("p2") else "linear"]
            t0 = time.perf_counter()
            if c == "value":
                out, info, st = h.loglik_vecchia(ranks, max_dist)
            elif c == "grad":
                out, _, info, st = h.loglik_vecchia_grad(ranks, max_dist)
            elif c.startswith("value"):
                out, _, _, info, st = h.loglik_vecchia_trend(ranks, max_dist)
            else:
                out, _, _, _, info, st = h.loglik_vecchia_trend_grad(ranks, max_dist)
            wall = 1e3 * (time.perf_counter() - t0)
            stages = (h.vecchia_trend_timings() if "_" in c else h.vecchia_grad_timings() if c == "grad" else h.vecchia_timings())
            if rep:
                acc[c].append(dict(stages, wall_ms=wall))
            last[c] = dict(l=float(out[0]), info=int(info), k_max=st["k_max"], n_empty=st["n_empty"], n_capped=st["n_capped"])
    for h in hs.values():
        h.close()
    out = dict(n_per_process=n_per_process, max_dist_km=max_dist, caps=list(CAPS), ordering="random", repetitions=REPS)
    for c in cells:
        keys = [k for k in acc[c][0] if k.endswith("_ms")]
        out[c] = dict(last[c], **{k: spread([r[k] for r in acc[c]]) for k in keys})
    wall = {c: out[c]["wall_ms"]["median"] for c in cells}
    out["value_p2_over_value"] = wall["value_p2"] / wall["value"]
    out["value_p6_over_value"] = wall["value_p6"] / wall["value"]
    out["grad_p2_over_grad"] = wall["grad_p2"] / wall["grad"]
    out["grad_p6_over_grad"] = wall["grad_p6"] / wall["grad"]
    # the solve kernels alone: k_vecchia_trend (2 + p riding rows) against k_local_solve (2)
    out["solve_p2_over_solve"] = out["value_p2"]["solve_ms"]["median"] / out["value"]["solve_ms"]["median"]
    out["solve_p6_over_solve"] = out["value_p6"]["solve_ms"]["median"] / out["value"]["solve_ms"]["median"]
    return out


def fit(n_per_process=20000, max_dist=800.0):
    from sif_xco2_cokriging_amd import fields, model, native, synth, vecchia
    pb = synth.conus_problem(n_per_process)
    # conus_problem's values are cosine fields; a fit needs data of the model: z = L eps from the library's own factor, plus a
    # constant per process
    pv = pb["params"]
    hs = native.Handle(0)
    hs.set_option("site_order", 0)
    hs.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    hs.set_metric(pb["metric"])
    for k in range(2):
        hs.set_data(k, pb["coords"][k], np.zeros(n_per_process))
    hs.assemble_joint()
    assert hs.factor() == 0
    z = hs.sample(np.random.default_rng(7).standard_normal(2 * n_per_process))
    hs.close()
    means = (1.5, -0.75)
    mf = fields.MultiField([fields.Field(pb["coords"][k], z[k * n_per_process:(k + 1) * n_per_process] + means[k]) for k in range(2)])
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    start = list(pb["params"])
    start[0], start[5], start[8] = 1.3 * start[0], 1.3 * start[5], 2.0 * start[8]
    counts = {"n": 0}
    value_call, grad_call = native.Handle.loglik_vecchia_trend, native.Handle.loglik_vecchia_trend_grad

    def counted(fn):
        def f(self, *a, **k):
            counts["n"] += 1
            return fn(self, *a, **k)
        return f

    native.Handle.loglik_vecchia_trend, native.Handle.loglik_vecchia_trend_grad = counted(value_call), counted(grad_call)
    rows = []
    try:
        for how in ("numeric", "analytic"):
            mod = model.MultivariateMatern(2)
            mod.params.set_values(start)
            names = list(mod.params.get_names())
            counts["n"] = 0
            t0 = time.perf_counter()
            mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free],
                               vecchia=vecchia.Vecchia(max_dist, max_neighbours=CAPS, ordering="random", seed=0, gradient=how,
                                                       trend="constant"))
            secs = time.perf_counter() - t0
            r = mod.fit_result
            x = mod.params.get_values().astype(float)
            rows.append(dict(gradient=how, l=r.loglik, x=x[[0, 5, 8]].tolist(), beta=r.beta.tolist(),
                             beta_se=np.sqrt(np.diag(r.beta_cov)).tolist(), n_eval=r.n_eval, native_calls=counts["n"],
                             n_iter=r.n_iter, success=r.success, message=r.message, seconds=secs))
    finally:
        native.Handle.loglik_vecchia_trend, native.Handle.loglik_vecchia_trend_grad = value_call, grad_call
    return dict(N=2 * n_per_process, max_dist_km=max_dist, caps=list(CAPS), free=free, start=[start[0], start[5], start[8]],
                means=list(means), rows=rows, analytic_over_numeric_seconds=rows[1]["seconds"] / rows[0]["seconds"])


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

    if "calls" in args:
        save("calls", [calls(20000, 800.0)])
        save("calls", out["calls"] + [calls(250000, 60.0)])
    if "fit" in args:
        save("fit", fit())
