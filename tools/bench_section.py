"""Timing of the mesh cross-sections (not part of bench.py): mm.mesh_cross_sections on the million-face thin tube of
tools/bench_geodesic.py with 2 000 stations along its axis.  Reported apart: the whole call (wall clock), the device
time of the cut (the engine's events around the clear and the cut kernel), the host plan (the test hook
mm_section_plan, one call, no device) and the host chain and measure (the test hook mm_section_chain on the call's
own segments); then the same on the noisy capped tube of tools/bench_mesh_refine.py (`--dense`, 100 000 faces), where
every plane crosses some 800 faces and the segments are many.  As context, a vectorised numpy restatement of rules 1
to 4 on 16 threads over `--numpy-planes` of the planes, with no cull (it is a yardstick for the work, not a competitor:
it tests every face against every plane).
Then what the vertex-cloud slices of mm.discretize_vessel cost: on the noisy capped tube of tools/bench_mesh_refine.py
(radius 1, 100 sides: its polygon's area is 3.1395) the area of the middle station under discretize_vessel and under
vessel_profile, before and after isotropic_remesh.  No time is promised and there is no baseline: the call is new.
Prints one JSON line and writes it to profiles/bench_section.json.

    python tools/bench_section.py [--rings 125001] [--stations 2000] [--reps 5] [--numpy-planes 32] [--dense 400x125]
                                    [--compare 100x50]
"""
import argparse
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multimoda_rs_amd as mm  # noqa: E402
from bench_geodesic import thin_tube  # noqa: E402
from bench_mesh_refine import _best, capped_tube  # noqa: E402

S = mm.section
N = mm._native


def numpy_cut(v, f, o, n):
    """rules 1 to 4 for one plane, vectorised, every face: the (m, 2, 3) points of the crossed faces"""
    h = (n[0] * (v[:, 0] - o[0]) + n[1] * (v[:, 1] - o[1])) + n[2] * (v[:, 2] - o[2])
    s = h >= 0.0
    fs = s[f]
    hit = np.nonzero((fs[:, 0] != fs[:, 1]) | (fs[:, 1] != fs[:, 2]))[0]
    t, fs = f[hit], fs[hit]
    k = np.where(fs[:, 0] == fs[:, 1], 2, np.where(fs[:, 0] == fs[:, 2], 1, 0))           # the corner alone on its side
    rows = np.arange(len(t))
    a = t[rows, k]
    pts = np.empty((len(t), 2, 3))
    for j in (1, 2):
        b = t[rows, (k + j) % 3]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        tt = h[lo] / (h[lo] - h[hi])
        pts[:, j - 1] = v[lo] + tt[:, None] * (v[hi] - v[lo])
    return hit, pts


def _plan_once(v, f, o, n):
    """one mm_section_plan call: what the host does in front of the upload"""
    order, info = np.zeros(max(len(f), 1), dtype=np.int32), np.zeros(8, dtype=np.int64)
    N.check(N.lib().mm_section_plan(N._ptr(v), len(v), N._ptr(f), len(f), N._ptr(o), N._ptr(n), len(o), N._ptr(order),
                                    N._ptr(info), None, None, 0, None, 0), "section_plan")
    return info


def timed_parts(v, f, o, n, eng, reps, numpy_planes):
    run = lambda: mm.mesh_cross_sections((v, f), o, n, engine=eng)          # noqa: E731
    run()
    t_min, t_median, got = _best(run, reps)
    eng.profile(True)
    run()
    ms, _evals = eng.profile_launches()
    eng.profile(False)
    p_min, p_median, info = _best(lambda: _plan_once(v, f, o, n), reps)
    seg = S.section_cut_host((v, f), o, n)
    c_min, c_median, chained = _best(lambda: S.section_chain(seg, o, n), reps)
    assert chained.points.tobytes() == got.points.tobytes()
    sub = np.linspace(0, len(o) - 1, min(numpy_planes, len(o))).astype(int)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        n_hit = sum(len(hit) for hit, _pts in pool.map(lambda p: numpy_cut(v, f, o[p], n[p]), sub))
    np_ms = (time.perf_counter() - t0) * 1e3
    h = hashlib.sha256()
    for a in (got.contour_off, got.points, got.contour_area, got.selected):
        h.update(np.ascontiguousarray(a).tobytes())
    return {"vertices": int(len(v)), "faces": int(len(f)), "planes": int(len(o)), "ms_min": t_min, "ms_median": t_median,
            "device_cut_ms": float(ms.sum()), "plan_ms_min": p_min, "plan_ms_median": p_median, "chain_ms_min": c_min,
            "chain_ms_median": c_median, "workgroups": int(info[4]), "numpy_planes": int(len(sub)),
            "numpy_ms": np_ms, "numpy_ms_per_plane": np_ms / max(len(sub), 1), "numpy_segments": int(n_hit), **got.report,
            "sha256": h.hexdigest()}


def slices_against_sections(size, stretch, eng):
    """the middle station of a capped tube of radius 1 under discretize_vessel and under vessel_profile"""
    n_around, n_rings = (int(x) for x in size.split("x"))
    v, f, step = capped_tube(n_around, n_rings, stretch)
    z1 = (n_rings - 1) * step * stretch
    zs = np.arange(0.25, z1 - 0.25, 0.5)
    xyz = np.stack([0 * zs, 0 * zs, zs], 1)
    cl = mm.Centerline.from_arrays(xyz, np.tile([0.0, 0.0, 1.0], (len(zs), 1)), radius=1.0, branch_id=0)
    out = {"mesh": size, "stretch": stretch, "polygon_area": 0.5 * n_around * np.sin(2.0 * np.pi / n_around), "stations": int(len(zs))}
    rv, rf = mm.isotropic_remesh((v, f), engine=eng)[0]
    for label, (mv, mf) in (("as_it_comes", (v, f)), ("remeshed", (np.asarray(rv), np.asarray(rf)))):
        prof = mm.vessel_profile((mv, mf), cl, engine=eng)
        slices = mm.discretize_vessel(cl, mv, 0, 0.5, 200, engine=eng)
        areas = mm.contour_measures(slices, closest_2d=False, engine=eng).area
        mid = len(zs) // 2
        out[label] = {"faces": int(len(mf)), "section_area_mid": float(prof.table[mid, 2]),
                      "section_area_min_max": [float(np.nanmin(prof.table[:, 2])), float(np.nanmax(prof.table[:, 2]))],
                      "slices": int(len(slices)), "slice_area_mid": float(areas[len(areas) // 2]),
                      "slice_area_min_max": [float(np.min(areas)), float(np.max(areas))], "n_missing": prof.report["n_missing"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=125001)
    ap.add_argument("--stations", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-planes", type=int, default=32)
    ap.add_argument("--compare", default="100x50")
    ap.add_argument("--dense", default="400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_section.json"))
    a = ap.parse_args()
    out = {"bench": "mesh_cross_sections", "time": "wall clock, ms; device_cut_ms from the engine's events"}
    with mm.Engine() as eng:
        v, f = thin_tube(a.rings)
        v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
        z1 = 0.25 * (a.rings - 1)
        zs = (np.arange(a.stations) + 0.37) * (z1 / a.stations)
        o = np.stack([0 * zs, 0 * zs, zs], 1)
        n = np.tile([0.05, -0.03, 1.0], (a.stations, 1))
        out["tube"] = timed_parts(v, f, o, n, eng, a.reps, a.numpy_planes)
        if a.dense:                                                       # many segments a plane: where the host's share grows
            n_around, n_rings = (int(x) for x in a.dense.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            z1 = (n_rings - 1) * step * a.stretch
            zs = (np.arange(a.stations) + 0.37) * (z1 / a.stations)
            o = np.stack([0 * zs, 0 * zs, zs], 1)
            out["dense"] = {"mesh": a.dense, **timed_parts(v, f, o, np.ascontiguousarray(n[:len(o)]), eng, a.reps, a.numpy_planes)}
        if a.compare:
            out["slices_against_sections"] = slices_against_sections(a.compare, a.stretch, eng)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
