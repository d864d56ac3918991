"""GPU measurements of the expected information of the Vecchia likelihood (ck_loglik_vecchia_fisher; DESIGN 5d-4,
profiles/r05_vecchia_info.json).

    python scripts/bench_vecchia_info.py [--out file.json]

bench_vecchia_grad.py's sizes and caps: conus_problem with set A, caps (16,16), random ordering, at N = 40 000 (800 km) and
N = 2 x 250 000 (60 km), all eleven parameters live.  Three things interleaved in one process on one handle:
  info     the information call (host wall clock and the stages of ck_timings [88 ..])
  grad     the gradient call
  fd       what the information cost before: central differencing of the analytic gradient over the same eleven slots, 22
           gradient calls at displaced parameters.  Reported twice: the gradient calls alone (`grad_calls_ms`, the number the
           condition uses) and with the ck_set_model before each of them (`wall_ms`, what a caller pays).
The problem's values are cosine fields, not draws from the model: the differenced (observed) diagonal recorded beside the
expected one is no check of it.  One warm-up, then repetitions, medians, the slab reserved (as bench_vecchia.py).  The condition of the feature: info is faster
than fd's gradient calls alone; `info_over_fd` is the ratio."""
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
FD_REL = 1e-4   # the relative displacement of a differenced parameter


def set_params(h, pv):
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])


def calls(n_per_process, max_dist):
    from sif_xco2_cokriging_amd import synth, vecchia
    pb = synth.conus_problem(n_per_process)
    ranks = vecchia.ordering_ranks(pb["coords"], "random", 0)
    h = handle(pb)
    h.local_reserve(0)
    h.set_local_neighbours(*CAPS)
    pv = np.asarray(pb["params"], dtype=float)
    acc = {c: [] for c in ("info", "grad", "fd")}
    last = {}
    for rep in range(REPS + 1):          # rep 0: the warm-up of every shape
        t0 = time.perf_counter()
        I, info, st = h.loglik_vecchia_fisher(ranks, max_dist)
        wall = 1e3 * (time.perf_counter() - t0)
        if rep:
            acc["info"].append(dict(h.vecchia_fisher_timings(), wall_ms=wall))
        last["info"] = dict(info=int(info), k_max=st["k_max"], n_empty=st["n_empty"], n_capped=st["n_capped"],
                            fisher_diag=np.diag(I)[:11].tolist())
        t0 = time.perf_counter()
        out3, grad, ginfo, _ = h.loglik_vecchia_grad(ranks, max_dist)
        wall = 1e3 * (time.perf_counter() - t0)
        if rep:
            acc["grad"].append(dict(h.vecchia_grad_timings(), wall_ms=wall))
        last["grad"] = dict(l=float(out3[0]), info=int(ginfo))
        # the observed information by central differences of the analytic gradient: column j = -(g(+e_j) - g(-e_j)) / (2 e_j)
        H = np.zeros((11, 11))
        inner = 0.0
        t0 = time.perf_counter()
        for j in range(11):
            e = FD_REL * max(abs(pv[j]), 1e-3)
            g = []
            for sgn in (1.0, -1.0):
                y = pv.copy()
                y[j] += sgn * e
                set_params(h, y)
                t1 = time.perf_counter()
                g.append(h.loglik_vecchia_grad(ranks, max_dist)[1][:11])
                inner += 1e3 * (time.perf_counter() - t1)
            H[:, j] = -(g[0] - g[1]) / (2.0 * e)
        wall = 1e3 * (time.perf_counter() - t0)
        set_params(h, pv)
        if rep:
            acc["fd"].append(dict(wall_ms=wall, grad_calls_ms=inner))
        last["fd"] = dict(n_gradient_calls=22, observed_diag=np.diag(H).tolist())
    h.close()
    out = dict(n_per_process=n_per_process, max_dist_km=max_dist, caps=list(CAPS), ordering="random", repetitions=REPS, live_slots=11)
    for c in acc:
        keys = [k for k in acc[c][0] if k.endswith("_ms")]
        out[c] = dict(last[c], **{k: spread([r[k] for r in acc[c]]) for k in keys})
    out["info"].update(n_data=int(acc["info"][0]["n_data"]), n_entries=int(acc["info"][0]["n_entries"]))
    i, g = out["info"]["wall_ms"]["median"], out["grad"]["wall_ms"]["median"]
    out["info_over_grad"] = i / g
    out["info_over_fd"] = i / out["fd"]["grad_calls_ms"]["median"]
    out["info_over_fd_with_set_model"] = i / out["fd"]["wall_ms"]["median"]
    out["info_faster_than_fd"] = bool(i < out["fd"]["grad_calls_ms"]["median"])
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

    save("calls", [calls(20000, 800.0)])
    save("calls", out["calls"] + [calls(250000, 60.0)])
