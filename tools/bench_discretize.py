"""Timing of the CCTA vessel discretisation (not part of bench.py): the nearest-anchor pass of discretize_vessel on a
synthetic aorta (every surface vertex against slice anchors every --step mm), its kernel time from the engine's HIP
events, the wall time of discretize_vessel and of discretize_vessel_tree on the labelled synthetic take-off mesh, and the
numpy checker on the same discretize_vessel input (a host restatement, not the reference).  Prints one JSON line.

    python tools/bench_discretize.py [--theta 256] [--rings 400] [--length 150] [--step 0.2] [--reps 5] [--skip-host]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multimoda_rs_amd as mm  # noqa: E402
from multimoda_rs_amd import _native as N  # noqa: E402
from multimoda_rs_amd.centerline import Centerline  # noqa: E402


def _cl(xyz):
    xyz = np.asarray(xyz, dtype=np.float64)
    t = np.gradient(xyz, axis=0)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return Centerline.from_arrays(xyz, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=256)
    ap.add_argument("--rings", type=int, default=400)
    ap.add_argument("--length", type=float, default=150.0)
    ap.add_argument("--step", type=float, default=0.2)
    ap.add_argument("--n-points", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    v, f, ca, cr, cl, _ = mm.synth.synthetic_takeoff_mesh(n_theta=a.theta, n_z=a.rings, length=a.length, n_around=32)
    cla, clr, cll = _cl(ca), _cl(cr), _cl(cl)
    n_anchors = int(N.lib().mm_slice_anchor_count(N._ptr(cla.points), len(cla), 0, a.step))
    evals = float(v.shape[0]) * n_anchors
    with mm.Engine(0) as eng:
        run = lambda: mm.discretize_vessel(cla, v, 0, a.step, a.n_points, engine=eng)
        contours = run()                                                        # warm-up
        eng.profile(True)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run()
        wall_vessel = (time.perf_counter() - t0) / a.reps
        n, ms, pe, cand = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        N.check(N.lib().mm_engine_profile_read(eng.handle, C.byref(n), C.byref(ms), C.byref(pe), C.byref(cand)),
                "profile_read")
        eng.profile(False)
        kernel_ms = ms.value / max(int(n.value), 1)
        assert abs(pe.value / max(int(n.value), 1) - evals) < 0.5, (pe.value, n.value, evals)
        res = mm.label_geometry((v, f), cla, clr, cll, acute_takeoff_rca=True, engine=eng)
        rd = dict(res, rca_points_main=res["rca_points"], lca_points_main=res["lca_points"])
        mm.discretize_vessel_tree(cla, clr, cll, rd, step_size=a.step, n_points=a.n_points, engine=eng)   # warm-up
        t0 = time.perf_counter()
        for _ in range(a.reps):
            tree = mm.discretize_vessel_tree(cla, clr, cll, rd, step_size=a.step, n_points=a.n_points, engine=eng)
        wall_tree = (time.perf_counter() - t0) / a.reps
    out = {"tool": "bench_discretize", "vertices": int(v.shape[0]), "anchors": n_anchors, "step_mm": a.step,
           "n_points": a.n_points, "distance_evals": evals, "kernel_ms": round(kernel_ms, 4),
           "evals_per_s": evals / (kernel_ms * 1e-3), "discretize_vessel_ms": round(wall_vessel * 1e3, 3),
           "contours": len(contours), "discretize_vessel_tree_ms": round(wall_tree * 1e3, 3),
           "tree_contours": [len(tree.discretized_aorta), len(tree.discretized_rca_main), len(tree.discretized_lca_main)]}
    if not a.skip_host:
        from mm_checkers import discretize as DZ
        t0 = time.perf_counter()
        want = DZ.discretize_vessel(cla.xyz(), np.stack([cla.points[k] for k in ("tx", "ty", "tz")], 1),
                                    cla.points["branch_id"], v, 0, a.step, a.n_points)
        out["host_restatement_not_the_reference_s"] = round(time.perf_counter() - t0, 3)
        out["host_restatement_agrees"] = bool(len(want) == len(contours) and all(
            w[0] == c.id and np.array_equal(w[2], c.points) for w, c in zip(want, contours)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
