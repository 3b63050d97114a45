"""Timing of the CCTA mesh morphing (not part of bench.py): every aortic vertex of a synthetic aorta moved about its
nearest point of an aortic centerline resampled every --spacing mm (the reference's workflow resamples to the IVUS frame
spacing before it scales), its kernel time from the engine's HIP events, the wall time of
scale_region_centerline_morphing, of mm.scale on the labelled take-off mesh with synthetic frames that carry walls, and
of the host mm_diameter_morphing (adjust_diameter_centerline_morphing_simple) on the same input.  Prints one JSON line.

    python tools/bench_morph.py [--theta 256] [--rings 400] [--length 150] [--spacing 0.15] [--reps 5] [--skip-host]
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
from multimoda_rs_amd.centerline import CL_DTYPE, Centerline  # noqa: E402


def _cl(xyz):
    xyz = np.asarray(xyz, dtype=np.float64)
    a = np.zeros(xyz.shape[0], dtype=CL_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return Centerline(a)


def _frames_with_walls(engine):
    """A placed-size intravascular geometry with walls (built as tests/test_gpu_workflow.py builds it, unaligned)."""
    from test_golden_and_api import _array_input
    dia = _array_input(mm, n_frames=16, n_points=120, thickness=0.9, seed=3)
    sys_ = _array_input(mm, n_frames=14, n_points=120, thickness=1.1, seed=4)
    sys_.diastole = False
    pair, _ = mm.from_array_singlepair(dia, sys_, step_rotation_deg=1.0, range_rotation_deg=20.0, engine=engine)
    return pair.geom_a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=256)
    ap.add_argument("--rings", type=int, default=400)
    ap.add_argument("--length", type=float, default=150.0)
    ap.add_argument("--spacing", type=float, default=0.15)
    ap.add_argument("--adj", type=float, default=0.4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    v, f, ca, cr, cl, n_aorta_faces = mm.synth.synthetic_takeoff_mesh(n_theta=a.theta, n_z=a.rings, length=a.length,
                                                                      n_around=32)
    n_aorta = int(f[:n_aorta_faces].max()) + 1                  # the aortic vertices come first
    z = np.arange(0.0, a.length + 1e-9, a.spacing)
    cla = _cl(np.stack([np.zeros_like(z), np.zeros_like(z), z], 1))
    clr, cll = _cl(cr), _cl(cl)
    region = v[:n_aorta]
    evals = float(n_aorta) * len(cla)
    with mm.Engine(0) as eng:
        run = lambda: mm.scale_region_centerline_morphing((v, f), region, cla, a.adj, engine=eng)
        moved = run()                                           # warm-up
        eng.profile(True)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run()
        wall_region = (time.perf_counter() - t0) / a.reps
        n, ms, pe, cand = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        N.check(N.lib().mm_engine_profile_read(eng.handle, C.byref(n), C.byref(ms), C.byref(pe), C.byref(cand)),
                "profile_read")
        eng.profile(False)
        kernel_ms = ms.value / max(int(n.value), 1)
        assert abs(pe.value / max(int(n.value), 1) - evals) < 0.5, (pe.value, n.value, evals)
        res = mm.label_geometry((v, f), cla, clr, cll, acute_takeoff_rca=True, engine=eng)
        mm.label_anomalous_region(clr, cr[20:52:2], res, engine=eng)
        frames = _frames_with_walls(eng)
        mm.scale(dict(res), clr, cla, frames, engine=eng)      # warm-up
        t0 = time.perf_counter()
        for _ in range(a.reps):
            mm.scale(dict(res), clr, cla, frames, engine=eng)
        wall_scale = (time.perf_counter() - t0) / a.reps
    out = {"tool": "bench_morph", "vertices": int(v.shape[0]), "region_vertices": n_aorta, "centerline_points": len(cla),
           "spacing_mm": a.spacing, "distance_evals": evals, "kernel_ms": round(kernel_ms, 4),
           "evals_per_s": evals / (kernel_ms * 1e-3), "scale_region_centerline_morphing_ms": round(wall_region * 1e3, 3),
           "scale_ms": round(wall_scale * 1e3, 3),
           "scale_regions": [len(res["distal_points"]), len(res["aorta_points"]) + len(res["rca_removed_points"]),
                             len(res["proximal_points"])]}
    if not a.skip_host:
        t0 = time.perf_counter()
        host = mm.adjust_diameter_centerline_morphing_simple(cla, region, a.adj)
        out["host_diameter_morphing_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["host_agrees"] = bool(np.array_equal(host, moved[0][:n_aorta]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
