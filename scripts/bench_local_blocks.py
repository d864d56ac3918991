"""GPU benchmark of block cokriging in the moving neighbourhood (ck_predict_local_blocks): bench_local.py's inputs (config-3
sites, 2 x 20 000 observations, 400 km) without a cap and with caps (16, 16).  The members are the 8 833 sites of the 0.5-degree
grid, the blocks the 1-degree cells over the grid's extent that hold a member, every cell the plain mean of its members, the
search centre the default of Predictor.predict_blocks.  Beside it ck_predict_local on the same member sites: the only thing a
user could run before, and it does not yield the block error.  Per stage (ck_timings [104 ..]): the counting / select pass,
the LDS class, the tiled class, the sigma_BB pass, host wall clock, and the member-neighbour covariance evaluations.  One
warm-up per shape, five interleaved repetitions, the spread reported.

    python scripts/bench_local_blocks.py [sites per process, default 20000] [--out profiles/r13_local_blocks.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

MAX_DIST = 400.0
CAPS = [None, (16, 16)]
REPS = 5


def spread(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def cells_of(pc):
    """1-degree cells of the member grid: compact labels, plain-mean weights, centres = normalised mean unit vector"""
    key = np.floor(pc[:, 0]).astype(np.int64) * 1000 + np.floor(pc[:, 1]).astype(np.int64)
    _, lab = np.unique(key, return_inverse=True)
    r = int(lab.max()) + 1
    n_b = np.bincount(lab, minlength=r)
    la, lo = np.radians(pc[:, 0]), np.radians(pc[:, 1])
    u = np.column_stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    mu = np.column_stack([np.bincount(lab, weights=u[:, c], minlength=r) for c in range(3)])
    mu /= np.linalg.norm(mu, axis=1)[:, None]
    centres = np.column_stack([np.degrees(np.arcsin(mu[:, 2])), np.degrees(np.arctan2(mu[:, 1], mu[:, 0]))])
    return lab.astype(np.int32), 1.0 / n_b[lab], centres, n_b


def main():
    args = [a for a in sys.argv[1:]]
    out_path = None
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    n = int(args[0]) if args else 20000
    from sif_xco2_cokriging_amd import native, synth
    pb = synth.conus_problem(n)
    pv = pb["params"]
    h = native.Handle(0)
    h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
    h.set_metric(0)
    for k in range(2):
        h.set_data(k, pb["coords"][k], pb["values"][k])
    h.local_reserve(0)   # the scratch slab once: no timed call grows it
    pc = np.ascontiguousarray(pb["pcoords"], dtype=np.float64)
    lab, w, centres, n_b = cells_of(pc)
    r = len(centres)
    acc = {c: dict(blocks={}, blocks_wall=[], points_dev=[], points_wall=[]) for c in CAPS}
    res = {}
    for caps in CAPS:      # warm-up of every shape
        h.set_local_neighbours(*(caps or (0, 0)))
        h.predict_local_blocks(0, centres, pc, lab, w, max_dist=MAX_DIST)
        h.predict_local(0, pc, MAX_DIST)
    for _ in range(REPS):  # interleaved
        for caps in CAPS:
            h.set_local_neighbours(*(caps or (0, 0)))
            t0 = time.perf_counter()
            bp, be, binfo = h.predict_local_blocks(0, centres, pc, lab, w, max_dist=MAX_DIST)
            acc[caps]["blocks_wall"].append((time.perf_counter() - t0) * 1e3)
            for key, v in h.local_blocks_timings().items():
                acc[caps]["blocks"].setdefault(key, []).append(v)
            t0 = time.perf_counter()
            pp, pe, pinfo = h.predict_local(0, pc, MAX_DIST)
            acc[caps]["points_wall"].append((time.perf_counter() - t0) * 1e3)
            acc[caps]["points_dev"].append(h.timings()["local_ms"])
            res[caps] = (bp, be, binfo, pp, pe, pinfo)
    rows = []
    for caps in CAPS:
        bp, be, binfo, pp, pe, pinfo = res[caps]
        a = acc[caps]
        st = {k: spread(v) for k, v in a["blocks"].items()}
        evals = st.pop("cbar_evals")["median"]
        dev = st["count_ms"]["median"] + st["lds_ms"]["median"] + st["tiled_ms"]["median"] + st["prior_ms"]["median"]
        # the naive cell value a user could form before: the mean of the members' point predictions (its error is not available)
        mean_pts = np.bincount(lab, weights=w * np.nan_to_num(pp), minlength=r)
        rows.append(dict(
            caps=list(caps) if caps else None, max_dist_km=MAX_DIST, observations=2 * n, blocks=r, members=len(pc),
            members_per_block=dict(min=int(n_b.min()), max=int(n_b.max())),
            blocks_stage_ms=st, blocks_device_ms=dev, blocks_wall_ms=spread(a["blocks_wall"]), cbar_evals=evals,
            blocks_info={k: int(v) for k, v in binfo.items()},
            points_device_ms=spread(a["points_dev"]), points_wall_ms=spread(a["points_wall"]),
            points_info={k: int(v) for k, v in pinfo.items()},
            systems_factored=dict(blocks=r, points=len(pc)),
            blocks_over_points_device=dev / float(np.median(a["points_dev"])),
            max_abs_block_minus_mean_of_points=float(np.nanmax(np.abs(bp - mean_pts))),
            mean_block_err=float(np.nanmean(be)), mean_point_err=float(np.nanmean(pe)),
            checksum=float(np.nansum(bp))))
        print(json.dumps(rows[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(script="scripts/bench_local_blocks.py", reps=REPS, rows=rows), f, indent=1)
    h.close()


if __name__ == "__main__":
    main()
