"""GPU measurements of the analytic gradient of the Vecchia likelihood (ck_loglik_vecchia_grad; DESIGN 5d-3,
profiles/r08_vecchia_grad.json).

    python scripts/bench_vecchia_grad.py [calls] [fit] [parent <library of the parent commit>] [--out file.json]

calls   conus_problem with set A, caps (16,16), random ordering, at N = 40 000 (800 km) and N = 2 x 250 000 (60 km): the gradient
        call with every slot live, the gradient call with the three nu held, the value call of this library and -- with
        `parent` -- the value call of the parent commit's library on a handle of its own.  Host wall clock of the call and the
        stages of ck_timings [80 ..] / [72 ..].
fit     N = 40 000, sigma_11, len_scale_11 and nugget_11 free from a displaced start: evaluations, native calls and wall clock
        of fit_likelihood with Vecchia(gradient="numeric") and with gradient="analytic"
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


def calls(n_per_process, max_dist, parent_lib=None):
    from sif_xco2_cokriging_amd import native, synth, vecchia
    import bench_local_nmax
    pb = synth.conus_problem(n_per_process)
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 0)
    libs = {"this": native.lib()}
    if parent_lib:
        libs["parent"] = bench_local_nmax.bind(parent_lib)
    hs = {}
    for tag in libs:
        native._lib = libs[tag]          # every native call goes through native.lib()
        hs[tag] = handle(pb)
        hs[tag].local_reserve(0)
        hs[tag].set_local_neighbours(*CAPS)
    nu_held = np.ones(13, dtype=bool)
    nu_held[2:5] = False
    cells = ["grad_all", "grad_nu_held", "value"] + (["value_parent"] if parent_lib else [])
    acc = {c: [] for c in cells}
    last = {}
    for rep in range(REPS + 1):          # rep 0: the warm-up of every shape
        for c in cells:
            tag = "parent" if c == "value_parent" else "this"
            native._lib = libs[tag]
            h = hs[tag]
            t0 = time.perf_counter()
            if c.startswith("grad"):
                out3, grad, info, st = h.loglik_vecchia_grad(ranks, max_dist, free=None if c == "grad_all" else nu_held)
            else:
                out3, info, st = h.loglik_vecchia(ranks, max_dist)
                grad = None
            wall = 1e3 * (time.perf_counter() - t0)
            stages = h.vecchia_grad_timings() if c.startswith("grad") else h.vecchia_timings()
            if rep:
                acc[c].append(dict(stages, wall_ms=wall))
            last[c] = dict(l=float(out3[0]), info=int(info), k_max=st["k_max"], n_empty=st["n_empty"], n_capped=st["n_capped"],
                           gradient=None if grad is None else grad.tolist())
    for tag in libs:
        native._lib = libs[tag]
        hs[tag].close()
    native._lib = libs["this"]
    out = dict(n_per_process=n_per_process, max_dist_km=max_dist, caps=list(CAPS), ordering="random", repetitions=REPS)
    for c in cells:
        keys = [k for k in acc[c][0] if k.endswith("_ms")]
        out[c] = dict(last[c], **{k: spread([r[k] for r in acc[c]]) for k in keys})
        if c.startswith("grad"):
            out[c].update(n_data=int(acc[c][0]["n_data"]), n_pairs=int(acc[c][0]["n_pairs"]))
    g, v = out["grad_all"]["wall_ms"]["median"], out["value"]["wall_ms"]["median"]
    out["grad_over_value"] = g / v
    out["grad_nu_held_over_value"] = out["grad_nu_held"]["wall_ms"]["median"] / v
    out["value_bits_equal_gradient_call"] = out["grad_all"]["l"] == out["value"]["l"]
    if parent_lib:
        vp = out["value_parent"]["wall_ms"]["median"]
        out["value_over_parent_value"] = v / vp
        out["value_bits_equal_parent"] = out["value"]["l"] == out["value_parent"]["l"]
        out["grad_over_six_parent_values"] = g / (6.0 * vp)   # a three-parameter numeric gradient costs six value calls
    return out


def fit(n_per_process=20000, max_dist=800.0):
    from sif_xco2_cokriging_amd import fields, model, native, synth, vecchia
    pb = synth.conus_problem(n_per_process)
    # conus_problem's values are cosine fields; a fit needs data of the model: z = L eps from the library's own factor
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
    mf = fields.MultiField([fields.Field(pb["coords"][k], z[k * n_per_process:(k + 1) * n_per_process]) for k in range(2)])
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    start = list(pb["params"])
    start[0], start[5], start[8] = 1.3 * start[0], 1.3 * start[5], 2.0 * start[8]
    counts = {"n": 0}
    value_call, grad_call = native.Handle.loglik_vecchia, native.Handle.loglik_vecchia_grad

    def counted(fn):
        def f(self, *a, **k):
            counts["n"] += 1
            return fn(self, *a, **k)
        return f

    native.Handle.loglik_vecchia, native.Handle.loglik_vecchia_grad = counted(value_call), counted(grad_call)
    rows = []
    try:
        for how in ("numeric", "analytic"):
            mod = model.MultivariateMatern(2)
            mod.params.set_values(start)
            names = list(mod.params.get_names())
            counts["n"] = 0
            t0 = time.perf_counter()
            mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free],
                               vecchia=vecchia.Vecchia(max_dist, max_neighbours=CAPS, ordering="random", seed=0, gradient=how))
            secs = time.perf_counter() - t0
            r = mod.fit_result
            x = mod.params.get_values().astype(float)
            rows.append(dict(gradient=how, l=r.loglik, x=x[[0, 5, 8]].tolist(), n_eval=r.n_eval, native_calls=counts["n"],
                             n_iter=r.n_iter, success=r.success, message=r.message, seconds=secs))
    finally:
        native.Handle.loglik_vecchia, native.Handle.loglik_vecchia_grad = value_call, grad_call
    return dict(N=2 * n_per_process, max_dist_km=max_dist, caps=list(CAPS), free=free, start=[start[0], start[5], start[8]],
                rows=rows)


if __name__ == "__main__":
    args = sys.argv[1:]
    path = args[args.index("--out") + 1] if "--out" in args else None
    parent = args[args.index("parent") + 1] if "parent" in args else None
    out = {"repetitions": REPS}

    def save(key, value):
        out[key] = value
        print(json.dumps({key: value}), flush=True)
        if path:
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    if "calls" in args:
        save("calls", [calls(20000, 800.0, parent)])
        save("calls", out["calls"] + [calls(250000, 60.0, parent)])
    if "fit" in args:
        save("fit", fit())
