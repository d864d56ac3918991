"""Do the local entry points give the bits of another build of the library?  The check a refactor of ck_local.hip or of the local
stages of ck_api.hip records in profiles/: build the other commit as a second library (CK_BUILD_OUT=<path> python
sif-xco2-cokriging_amd/build_native.py in its checkout), then

    python scripts/check_local_bits.py --other-lib <path> [--out profiles/<name>.json]

Both libraries run the same calls on fixed inputs, each in a fresh child process (CK_LIB_PATH for the other one; a library that
lacks newer entry points binds only what it exports), and the outputs are compared with numpy.array_equal:
ck_predict_local (both processes, cv on and off, 150 / 400 / 900 km, caps (0, 0) with local_tile_min default / 0 / 10^6 and caps
(16, 16)), ck_simulate_local (draws from the device stream and from given noise, means, variances, counts, the weights of
ck_debug_simulate_local_weights, both processes) and ck_predict_local_blocks, on conus_problem(1500, seed=9), 200 sites.
--out: the result is merged into that JSON file as its section "parent_bits".  Exit status 1 when an array differs."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def outputs(path):
    """child mode: the calls on the library native.py loads, their outputs into path (npz)"""
    import ctypes

    from sif_xco2_cokriging_amd import native, synth
    old = ctypes.CDLL(native.LIB_PATH)   # the library may be an older commit's: bind only what it exports
    for name in [k for k in native._PROTOS if not hasattr(old, k)]:
        del native._PROTOS[name]
    out = {}
    pb = synth.conus_problem(1500, seed=9)
    pv = pb["params"]
    pc = pb["pcoords"][::41][:200]
    for caps, tile_min in [((0, 0), None), ((0, 0), 0), ((16, 16), None), ((0, 0), 10 ** 6)]:
        h = native.Handle(0)
        if tile_min is not None:
            h.set_option("local_tile_min", tile_min)
        h.set_model(2, pv[0:2], pv[2:5], pv[5:8], pv[8:10], pv[10])
        h.set_metric(0)
        for k in range(2):
            h.set_data(k, pb["coords"][k], pb["values"][k])
        h.set_local_neighbours(*caps)
        for i in range(2):
            for md in (150.0, 400.0, 900.0):
                for cv in (False, True):
                    p, e, _ = h.predict_local(i, pc, max_dist=md, cv=cv)
                    out[f"predict_local_{caps}_{tile_min}_{i}_{md}_{cv}_pred"] = p
                    out[f"predict_local_{caps}_{tile_min}_{i}_{md}_{cv}_err"] = e
        if caps != (0, 0):
            rng = np.random.default_rng(3)
            for i in range(2):
                ranks = rng.permutation(len(pc)).astype(np.int64)
                d, _, st = h.simulate_local(i, pc, ranks, 400.0, 9, seed=5)
                out[f"simulate_local_{i}_draws"], out[f"simulate_local_{i}_mean"] = d, st["mean"]
                out[f"simulate_local_{i}_var"], out[f"simulate_local_{i}_count"] = st["var"], st["count"]
                eps = rng.standard_normal((4, len(pc)))
                out[f"simulate_local_{i}_draws_given_noise"] = h.simulate_local(i, pc, ranks, 400.0, 4, noise=eps)[0]
                idx, w = h.simulate_local_weights(i, pc, ranks, 400.0)
                out[f"simulate_local_weights_{i}_idx"], out[f"simulate_local_weights_{i}_w"] = idx, w
            lab = (np.arange(len(pc)) // 4).astype(np.int32)
            cc = np.array([pc[lab == b].mean(axis=0) for b in range(lab.max() + 1)])
            p, e, _ = h.predict_local_blocks(0, cc, pc, lab, np.full(len(pc), 0.25), max_dist=900.0)
            out["predict_local_blocks_pred"], out["predict_local_blocks_err"] = p, e
        h.close()
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(child mode) write the outputs of the loaded library to this npz file")
    a = ap.parse_args()
    if a.child:
        return outputs(a.child)
    if not a.other_lib:
        ap.error("--other-lib is required")
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for tag, lib in (("this", None), ("other", os.path.abspath(a.other_lib))):
            env = dict(os.environ)
            env.pop("CK_LIB_PATH", None)
            if lib:
                env["CK_LIB_PATH"] = lib
            files.append(os.path.join(tmp, tag + ".npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[-1]], env=env, check=True, timeout=600)
        x, y = np.load(files[0]), np.load(files[1])
        assert sorted(x.files) == sorted(y.files)
        bad = [k for k in sorted(x.files) if not np.array_equal(x[k], y[k], equal_nan=True)]
        res = dict(source="scripts/check_local_bits.py --other-lib <the parent commit's library, built with CK_BUILD_OUT>: the calls "
                          "its docstring lists, this commit's library against the other one, numpy.array_equal",
                   arrays=len(x.files), values=int(sum(x[k].size for k in x.files)), differing=bad)
    print(json.dumps(res))
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["parent_bits"] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
