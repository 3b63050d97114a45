"""Timing of the CCTA mesh assembly (not part of bench.py): assemble_mesh of [take-off mesh of about 10^6 faces with a
section of the coronary cut out, the two strips, the IV tube] and fix_mesh_winding of the assembled faces with half of
them reversed, as whole-call wall times of the device path (csrc/mm_weld_kernels.hip) beside the plain numpy / Python
checker (tests/mm_checkers/stitch_mesh.py) on the same input.  The two agree bit for bit (checked here once).  Prints
one JSON line.

    python tools/bench_stitch.py [--theta 1024] [--rings 500] [--reps 5] [--skip-checker]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multimoda_rs_amd as mm  # noqa: E402
from mm_checkers import stitch_mesh as K  # noqa: E402


def _best(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3, float(np.median(times)) * 1e3, out


def parts_of(theta, rings, eng):
    v, f, _, cr, _, _ = mm.synth.synthetic_takeoff_mesh(n_theta=theta, n_z=rings)
    n_around, lo, hi = 16, 24, 48
    na = v.shape[0] - 2 * len(cr) * n_around
    ring = lambda k: v[na + k * n_around: na + (k + 1) * n_around]                   # noqa: E731
    res = {"mesh": (v, f), "section_points": np.concatenate([ring(k) for k in range(lo, hi + 1)])}
    cut = mm.remove_labeled_points_from_mesh(res, "section_points", target_boundaries=2, engine=eng)
    frames = [ring(k).mean(axis=0) + 0.8 * (ring(k) - ring(k).mean(axis=0)) for k in range(lo, hi + 1)]
    geom = mm.FlatGeometry.from_frames(frames)
    rings_ = [cut["boundary_points_1"], cut["boundary_points_2"]]
    parts, _, _ = K.stitch_parts(frames, geom.centroids, geom.centroids[0], rings_, cut["mesh"])
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=1024)
    ap.add_argument("--rings", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    a = ap.parse_args()
    out = {"bench": "stitch"}
    with mm.Engine() as eng:
        parts = parts_of(a.theta, a.rings, eng)
        assemble = lambda: mm.assemble_mesh(parts, engine=eng)                        # noqa: E731
        assemble()
        out["assemble_ms_min"], out["assemble_ms_median"], (gv, gf, rep) = _best(assemble, a.reps)
        mixed = gf.copy()
        flip = np.random.default_rng(0).random(len(gf)) < 0.5
        mixed[flip] = mixed[flip][:, ::-1]
        wind = lambda: mm.ccta._fix_winding(mixed, eng)                               # noqa: E731
        out["winding_ms_min"], out["winding_ms_median"], (gw, info) = _best(wind, a.reps)
        out.update(vertices_in=int(sum(len(p[0]) for p in parts)), faces_in=int(sum(len(p[1]) for p in parts)),
                   vertices=int(len(gv)), faces=int(len(gf)), winding_rounds=int(info["winding_rounds"]),
                   open_edges=int(rep["n_open_edges"]), welded=int(rep["n_welded_vertices"]))
    if not a.skip_checker:
        t0 = time.perf_counter()
        wv, wf, wrep = K.assemble(parts)
        out["checker_assemble_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ww = K.fix_winding(mixed)[0]
        out["checker_winding_ms"] = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(gv.view(np.uint64), wv.view(np.uint64)) and np.array_equal(gf, wf)
        same &= np.array_equal(gw, ww) and np.float64(rep["volume"]).view(np.uint64) == np.float64(wrep["volume"]).view(np.uint64)
        out["identical_to_checker"] = bool(same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
