"""Timing of the rim conditioning (not part of bench.py): condition_boundary_rings on the take-off mesh of about 10^6
faces with a section of the coronary cut out, and its three mesh-wide stages on their own (locate_points,
enforce_layer_gap_from_plane, split_rim_edges), as whole-call wall times of the device path (csrc/mm_rim.cpp,
csrc/mm_rim_kernels.hip) beside the plain numpy / Python checker (tests/mm_checkers/rim_condition.py) on the same
input on the same machine.  Faces, indices and layers are compared exactly, coordinates at 1e-9 mm.  Prints one JSON
line.

    python tools/bench_rim.py [--theta 1024] [--rings 500] [--reps 5] [--skip-checker]
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
from mm_checkers import rim_condition as K  # noqa: E402
from mm_checkers import stitch_mesh as SK  # noqa: E402


def _best(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3, float(np.median(times)) * 1e3, out


def case_of(theta, rings, eng):
    v, f, _, cr, _, _ = mm.synth.synthetic_takeoff_mesh(n_theta=theta, n_z=rings)
    n_around, lo, hi = 16, 24, 48
    na = v.shape[0] - 2 * len(cr) * n_around
    ring = lambda k: v[na + k * n_around: na + (k + 1) * n_around]                   # noqa: E731
    res = {"mesh": (v, f), "section_points": np.concatenate([ring(k) for k in range(lo, hi + 1)]), "aorta_points": v[:na:97]}
    cut = mm.remove_labeled_points_from_mesh(res, "section_points", target_boundaries=2, engine=eng)
    frames = []
    for k in range(lo, hi + 1):
        c = ring(k).mean(axis=0)
        fine = np.empty((2 * n_around, 3))
        fine[0::2] = ring(k)
        fine[1::2] = 0.5 * (ring(k) + np.roll(ring(k), -1, axis=0))
        frames.append(c + 0.8 * (fine - c))
    return cut, mm.FlatGeometry.from_frames(frames), frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=1024)
    ap.add_argument("--rings", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    a = ap.parse_args()
    out = {"bench": "rim"}
    c = mm.ccta
    with mm.Engine() as eng:
        cut, geom, frames = case_of(a.theta, a.rings, eng)
        v, f = cut["mesh"]
        rings = [cut["boundary_points_1"], cut["boundary_points_2"]]
        i, j, _ = SK.assign_rings_to_ends(rings, geom.centroids[0], geom.centroids[-1])
        whole = lambda: mm.condition_boundary_rings(cut["mesh"], cut, geom, engine=eng)          # noqa: E731
        whole()
        out["condition_ms_min"], out["condition_ms_median"], got = _best(whole, a.reps)
        rep = got["rim_report"]
        ring_idx = c.locate_points(v, rings[i], eng)
        counts = c.densify_plan(rings[i], 32)[0]
        o, n = c.fit_ring_plane(frames[0])
        locate = lambda: c.locate_points(v, rings[i], eng)                                        # noqa: E731
        push = lambda: c.enforce_layer_gap_from_plane((v, f), ring_idx, o, n, engine=eng, return_info=True)   # noqa: E731
        split = lambda: c.split_rim_edges(v, f, ring_idx, counts, eng)                             # noqa: E731
        out["locate_ms_min"], out["locate_ms_median"], g_idx = _best(locate, a.reps)
        out["layer_push_ms_min"], out["layer_push_ms_median"], g_push = _best(push, a.reps)
        out["split_ms_min"], out["split_ms_median"], g_split = _best(split, a.reps)
        out.update(vertices=int(len(v)), faces=int(len(f)), vertices_out=int(rep["n_vertices"]), faces_out=int(rep["n_faces"]),
                   n_launches=int(rep["n_launches"]), bytes_uploaded=int(rep["bytes_uploaded"]),
                   bytes_downloaded=int(rep["bytes_downloaded"]), ring_points=[int(len(rings[i])), int(len(rings[j]))],
                   target_n=int(rep["target_n"]), clamped=int(rep["clamped"]))
    if not a.skip_checker:
        first = SK.downsample(frames[0], 100)
        t0 = time.perf_counter()
        wp, wd, (wv, wf), wrep = K.prepare_prox_dist_boundary_pts(
            (v, f), rings[i], rings[j], geom.centroids[0], proximal_iv_frame_pts=first, clamp_overshoot=0.5,
            target_n=rep["target_n"], prox_outward=geom.centroids[0] - geom.centroids[-1], aorta_pts=cut["aorta_points"])
        out["checker_condition_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        w_idx = K.locate_points(v, rings[i])
        out["checker_locate_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        (pv, _), w_layer, _, _ = K.enforce_layer_gap_from_plane((v, f), ring_idx, o, n)
        out["checker_layer_push_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        (sv, sf), s_dense, _ = K.split_rim_edges((v, f), ring_idx, counts)
        out["checker_split_ms"] = (time.perf_counter() - t0) * 1e3
        bits = lambda x, y: x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))   # noqa: E731
        gv, gf = got["mesh"]
        same = np.array_equal(gf, wf) and gv.shape == wv.shape and float(np.abs(gv - wv).max()) < 1e-9
        same &= float(np.abs(got["boundary_points_1"] - wp).max()) < 1e-9 and float(np.abs(got["boundary_points_2"] - wd).max()) < 1e-9
        same &= np.array_equal(g_idx, w_idx) and np.array_equal(g_push[1], w_layer) and bits(g_push[0][0], pv)
        same &= bits(g_split[0], sv) and np.array_equal(g_split[1], sf) and g_split[2].tolist() == s_dense
        out["agrees_with_checker"] = bool(same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
