"""GPU measurements of the Vecchia likelihood (ck_loglik_vecchia; DESIGN 5d-3, profiles/r07_vecchia.json).

    python scripts/bench_vecchia.py [quality] [scale] [fd] [fit] [parent <library of the parent commit>] [--out file.json]

quality  l_Vecchia - l_exact and the time per evaluation against ck_loglik: conus_problem at N = 10 000 and 40 000, caps
         (8,8) / (16,16) / (32,32), random and Hilbert ordering
scale    time per evaluation at N = 2 x 250 000 and 2 x 500 000 with caps (16,16), per stage (ck_timings [72 ..])
fd       N = 400, full conditioning: the central-difference gradient against ck_loglik's analytic one, steps 1e-3 .. 1e-6
fit      the fit of tests/test_gpu_vecchia.py under several steps and stopping rules
parent   bench_local_nmax.gate: the uncapped 400 km local call of this library against the parent commit's, alternated
One warm-up, then interleaved repetitions in one process, the slab reserved (as bench_local_nmax.py)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

REPS = 3
CAPS = [(8, 8), (16, 16), (32, 32)]


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


def quality(n_total, max_dist):
    from sif_xco2_cokriging_amd import synth, vecchia
    pb = synth.conus_problem(n_total // 2)
    hd = handle(pb)
    hd.assemble_joint()
    exact_ms = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        hd.assemble_joint()   # an evaluation at new parameters assembles, factors and reduces
        info, exact, _ = hd.loglik(False)
        if rep:
            exact_ms.append(1e3 * (time.perf_counter() - t0))
    assert info == 0
    hd.close()
    h = handle(pb)
    h.local_reserve(0)
    ranks = {o: vecchia.ordering_ranks(pb["coords"], o, 0) for o in ("random", "hilbert")}
    cells = [(o, c) for o in ranks for c in CAPS]
    acc = {c: [] for c in cells}
    out = {}
    for rep in range(REPS + 1):
        for o, caps in cells:
            h.set_local_neighbours(*caps)
            out3, info, st = h.loglik_vecchia(ranks[o], max_dist)
            tv, t = h.vecchia_timings(), h.timings()
            if rep:
                acc[o, caps].append(tv["total_ms"])
            out[o, caps] = dict(ordering=o, caps=list(caps), l=float(out3[0]), l_minus_exact=float(out3[0] - exact[0]),
                                logdet_minus_exact=float(out3[1] - exact[1]), quad_minus_exact=float(out3[2] - exact[2]),
                                info=int(info), k_max=st["k_max"], n_empty=st["n_empty"], n_capped=st["n_capped"],
                                n_rescan=int(t["local_n_rescan"]), select_ms=tv["select_ms"], solve_ms=tv["solve_ms"],
                                terms_ms=tv["terms_ms"])
    h.close()
    return dict(N=n_total, max_dist_km=max_dist, l_exact=float(exact[0]), ck_loglik_ms=spread(exact_ms),
                cells=[dict(out[c], total_ms=spread(acc[c])) for c in cells])


def scale(n_per_process, max_dist, caps=(16, 16)):
    from sif_xco2_cokriging_amd import synth, vecchia
    t0 = time.perf_counter()
    pb = synth.conus_problem(n_per_process)
    h = handle(pb)
    h.local_reserve(0)
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 0)
    setup_s = time.perf_counter() - t0
    h.set_local_neighbours(*caps)
    rows = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        out3, info, st = h.loglik_vecchia(ranks, max_dist)
        wall = 1e3 * (time.perf_counter() - t0)
        tv, t = h.vecchia_timings(), h.timings()
        rows.append(dict(tv, wall_ms=wall))
    h.close()
    keys = ["select_ms", "solve_ms", "terms_ms", "total_ms", "wall_ms"]
    return dict(n_per_process=n_per_process, max_dist_km=max_dist, caps=list(caps), ordering="random", setup_s=setup_s,
                first_call=rows[0], **{k: spread([r[k] for r in rows[1:]]) for k in keys}, l=float(out3[0]), info=int(info),
                k_max=st["k_max"], n_empty=st["n_empty"], n_capped=st["n_capped"], n_rescan=int(t["local_n_rescan"]),
                cand_max=int(t["local_cand_max"]), n_lds=int(tv["n_lds"]), n_tiled=int(tv["n_tiled"]))


def fit_problem():
    from oracle import cokrige_oracle as orc
    from sif_xco2_cokriging_amd import fields
    truth = [1.0, 0.8, 1.5, 1.5, 1.5, 450.0, 450.0, 450.0, 0.05, 0.03, 0.5]
    rng = np.random.default_rng(31)
    pts = np.column_stack([rng.uniform(25, 50, 300), rng.uniform(-120, -70, 300)])
    coords = [pts[:200].copy(), pts[100:300].copy()]
    S = orc.joint_cov(orc.Params.from_flat(truth), coords, 0)
    z = np.linalg.cholesky(S) @ rng.standard_normal(400)
    mf = fields.MultiField([fields.Field(coords[k], [z[:200], z[200:]][k]) for k in range(2)])
    start = list(truth)
    start[0], start[5], start[8] = 1.3, 600.0, 0.1
    return truth, start, mf


def fd_table():
    """N = 400, full conditioning, at the fit test's starting point: the gradient in the [0, 1] coordinates by central
    differences of the Vecchia value against ck_loglik's analytic gradient times the bound widths"""
    from sif_xco2_cokriging_amd import model, vecchia
    truth, start, mf = fit_problem()
    mod = model.MultivariateMatern(2)
    mod.params.set_values(start)
    bounds = np.array([tuple(b) for b in mod.params.get_bounds()], dtype=float)
    lo, width = bounds[:, 0], bounds[:, 1] - bounds[:, 0]
    ll, g = mod.log_likelihood(mf, gradient=True)
    gu = np.asarray(g, dtype=float) * width
    v = vecchia.Vecchia(1e5, ordering="random", seed=2)
    rk = v.ranks([np.asarray(f.coords_main)[:, :2] for f in mf.fields])
    u0 = (np.array(start) - lo) / width

    def value(u):
        mod.params.set_values(lo + width * u)
        return mod.log_likelihood(mf, vecchia=v, _ranks=rk)

    rows = []
    for step in (1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 1e-6):
        fd = np.zeros(11)
        for j in range(11):
            up, dn = u0.copy(), u0.copy()
            up[j] += step
            dn[j] -= step
            fd[j] = (value(up) - value(dn)) / (2 * step)
        err = np.abs(fd - gu)
        rows.append(dict(step=step, max_abs_err=float(err.max()), max_rel_err=float(np.max(err / np.maximum(np.abs(gu), 1e-300))),
                         err_over_gnorm=float(err.max() / np.abs(gu).max()), worst=int(np.argmax(err))))
    mod.params.set_values(start)
    return dict(N=400, l=float(ll), l_vecchia_minus_exact=float(value(u0) - ll), analytic_gradient_u=gu.tolist(), rows=rows)


def fit_trials():
    from sif_xco2_cokriging_amd import model, vecchia
    truth, start, mf = fit_problem()
    free = ["sigma_11", "len_scale_11", "nugget_11"]
    out = []

    def run(label, v, fd_step=None, opts=None):
        import warnings
        mod = model.MultivariateMatern(2)
        mod.params.set_values(start)
        names = list(mod.params.get_names())
        if opts:
            model.VECCHIA_FIT_OPTIONS.update(opts)
        t0 = time.perf_counter()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            kw = {} if fd_step is None else {"fd_step": fd_step}
            mod.fit_likelihood(mf, guess=mod.params, fixed=[n for n in names if n not in free], vecchia=v, **kw)
        secs = time.perf_counter() - t0
        x = mod.params.get_values().astype(float)
        exact = model.MultivariateMatern(2)
        exact.params.set_values(x)
        r = mod.fit_result
        return dict(label=label, fd_step=fd_step, options=dict(model.VECCHIA_FIT_OPTIONS) if v is not None else None,
                    x=x[[0, 5, 8]].tolist(), exact_l=float(exact.log_likelihood(mf)), n_eval=r.n_eval, n_iter=r.n_iter,
                    success=r.success, message=r.message, warned=len(w) > 0, seconds=secs)

    out.append(run("dense", None))
    for fd_step in (1e-3, 1e-4, 1e-5):
        for opts in ({"ftol": 1e-13, "gtol": 1e-9}, {"ftol": 1e-11, "gtol": 1e-6}, {"ftol": 1e-10, "gtol": 1e-5}):
            out.append(run("vecchia", vecchia.Vecchia(1e5, ordering="random", seed=2), fd_step, opts))
            out[-1]["l_minus_dense_optimum"] = out[-1]["exact_l"] - out[0]["exact_l"]
    return out


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

    if "fd" in args:
        save("fd_step_table", fd_table())
    if "fit" in args:
        save("fit_trials", fit_trials())
    if "parent" in args:
        import bench_local_nmax
        save("uncapped_400km_against_parent", bench_local_nmax.gate(20000, args[args.index("parent") + 1]))
    if "quality" in args:
        save("quality", [quality(10000, 1500.0), quality(40000, 800.0)])
    if "scale" in args:
        save("scale", [scale(250000, 60.0), scale(500000, 45.0)])
