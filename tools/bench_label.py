"""Timing of the CCTA mesh labelling (not part of bench.py): the ray-triangle pass of the occlusion removal at a
realistic size (every face of a synthetic aorta-plus-coronary mesh against the rays of a 60 mm take-off), its kernel
time from the engine's HIP events, the label_geometry wall time, and the numpy checker on the same occlusion input
(a host restatement, not the reference).  Prints one JSON line.

    python tools/bench_label.py [--theta 256] [--rings 200] [--reps 5] [--skip-host]
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
    return Centerline.from_arrays(xyz, np.zeros_like(xyz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=256)
    ap.add_argument("--rings", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    v, f, ca, cr, cl, _ = mm.synth.synthetic_takeoff_mesh(n_theta=a.theta, n_z=a.rings, n_around=32)
    tris = v[f].reshape(-1, 9)
    cla, clr, cll = _cl(ca), _cl(cr), _cl(cl)
    n_rays = len(ca) * len(range(0, min(int(np.ceil(60.0 / ((cla.mean_spacing() + clr.mean_spacing()) / 2.0))),
                                        len(cr)), int(np.ceil(1.0 / ((cla.mean_spacing() + clr.mean_spacing()) / 2.0)))))
    tests = float(n_rays) * tris.shape[0]
    with mm.Engine(0) as eng:
        run = lambda: mm.ccta.occluded_point_flags(clr, cla, 60.0, v, tris, 1.0, engine=eng)
        rm, ex = run()                                                          # warm-up
        eng.profile(True)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run()
        wall_occl = (time.perf_counter() - t0) / a.reps
        n, ms, pe, cand = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        N.check(N.lib().mm_engine_profile_read(eng.handle, C.byref(n), C.byref(ms), C.byref(pe), C.byref(cand)),
                "profile_read")
        eng.profile(False)
        kernel_ms = ms.value / max(int(n.value), 1)
        assert abs(pe.value / max(int(n.value), 1) - tests) < 0.5, (pe.value, n.value, tests)
        mm.label_geometry((v, f), cla, clr, cll, acute_takeoff_rca=True, engine=eng)     # warm-up
        t0 = time.perf_counter()
        for _ in range(a.reps):
            res = mm.label_geometry((v, f), cla, clr, cll, acute_takeoff_rca=True, engine=eng)
        wall_label = (time.perf_counter() - t0) / a.reps
    out = {"tool": "bench_label", "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "rays": int(n_rays),
           "ray_triangle_tests": tests, "kernel_ms": round(kernel_ms, 4),
           "tests_per_s": tests / (kernel_ms * 1e-3), "occlusion_call_ms": round(wall_occl * 1e3, 3),
           "faces_excluded": int(ex.sum()), "points_removed": int(rm.sum()),
           "label_geometry_ms": round(wall_label * 1e3, 3),
           "label_counts": {k: int(res[k].shape[0]) for k in res if k != "mesh"}}
    if not a.skip_host:
        from mm_checkers import label_coronary as LC
        t0 = time.perf_counter()
        want_rm, want_ex = LC.occluded(cr, ca, 60.0, v, tris, 1.0)
        out["host_restatement_not_the_reference_s"] = round(time.perf_counter() - t0, 3)
        out["host_restatement_agrees"] = bool(np.array_equal(want_rm, rm.astype(bool)) and
                                              want_ex == set(np.nonzero(ex)[0].tolist()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
