"""Timing of the lumen morphometry (not part of bench.py): the contour-measures kernel on the four pullbacks of
mm.synthetic_case(--frames) (4 x frames x points lumen contours, one launch) from the engine's HIP events, with and
without the 2-D closest-opposite pass; the wall time of GeometryPair.get_summary on two of them (table not printed);
DiscretizedVesselTree.get_summary on a discretised synthetic tree; and, for context, the host time of the numpy
checker's farthest pair (tests/mm_checkers/morphometry.py) per contour.  Prints one JSON line.

    python tools/bench_morphometry.py [--frames 512] [--points 501] [--reps 5] [--host-contours 8]
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
from multimoda_rs_amd import morphometry as M  # noqa: E402


def _profiled(eng, run, reps):
    """(kernel ms per launch, wall ms per call) over `reps` calls after one warm-up"""
    run()
    eng.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    wall = (time.perf_counter() - t0) / reps
    n, ms, pe, cand = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    N.check(N.lib().mm_engine_profile_read(eng.handle, C.byref(n), C.byref(ms), C.byref(pe), C.byref(cand)),
            "profile_read")
    eng.profile(False)
    return ms.value / max(int(n.value), 1), wall * 1e3


def _tree(eng):
    from test_gpu_discretize import _tree_cl, curved_tube
    from multimoda_rs_amd.centerline import Centerline
    xyz, tan, bid, pts = curved_tube(41, n_cl=200, n_ring=64, branches=3)
    ao = _tree_cl(curved_tube(42, n_cl=300)[0])
    cor = Centerline.from_arrays(xyz, tan, branch_id=bid)
    ao_pts = curved_tube(42, n_cl=300, n_ring=96, radius=6.0)[3][0]
    return mm.ccta.discretize_vessel_tree_raw(ao, cor, cor, ao_pts, pts[0], pts[0], [pts[1], pts[2]], [pts[2]],
                                              step_size=0.5, n_points=200, engine=eng)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--points", type=int, default=501)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-contours", type=int, default=8)
    a = ap.parse_args()
    geoms = mm.synthetic_case(a.frames, a.points)
    off = np.concatenate([[0], np.cumsum([np.diff(g.lumen_off) for g in geoms])]).astype(np.int64)
    xyz = np.concatenate([g.lumen for g in geoms])
    out = {"tool": "bench_morphometry", "contours": int(off.shape[0] - 1), "points": a.points,
           "pairs": float(np.sum(np.diff(off) * (np.diff(off) - 1) // 2))}
    with mm.Engine(0) as eng:
        out["kernel_ms"], out["measures_ms"] = (round(v, 4) for v in _profiled(
            eng, lambda: M.measure_csr(off, xyz, engine=eng), a.reps))
        out["kernel_2d_ms"], out["measures_2d_ms"] = (round(v, 4) for v in _profiled(
            eng, lambda: M.measure_csr(off, xyz, closest_2d=True, engine=eng), a.reps))
        pair = mm.GeometryPair(geoms[0], geoms[1])
        out["pair_kernel_ms"], out["pair_get_summary_ms"] = (round(v, 4) for v in _profiled(
            eng, lambda: pair.get_summary(print_table=False, engine=eng), a.reps))
        tree = _tree(eng)
        out["tree_slices"] = sum(len(v) for v in [tree.discretized_aorta, tree.discretized_rca_main,
                                                  tree.discretized_lca_main, *tree.rca_branches, *tree.lca_branches])
        out["tree_kernel_ms"], out["tree_get_summary_ms"] = (round(v, 4) for v in _profiled(
            eng, lambda: tree.get_summary(engine=eng), a.reps))
        got = M.measure_csr(off[:a.host_contours + 1], xyz[:off[a.host_contours]], engine=eng)
    from mm_checkers import morphometry as MC
    t0 = time.perf_counter()
    host = [MC.farthest_points_np(xyz[off[k]:off[k + 1]]) for k in range(a.host_contours)]
    out["host_numpy_farthest_ms_per_contour"] = round((time.perf_counter() - t0) * 1e3 / a.host_contours, 3)
    out["host_agrees"] = all(h == ((int(got.major_pair[k, 0]), int(got.major_pair[k, 1])), float(got.major[k]))
                             for k, h in enumerate(host))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
