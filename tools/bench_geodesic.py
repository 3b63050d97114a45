"""Timing of the centerline-from-mesh calls (not part of bench.py): mm.mesh_geodesic_distance, mm.mesh_skeleton and
mm.centerline_from_mesh on the thin tubes of tests/test_gpu_stitch.py (4 vertices a ring, rings 0.25 apart) at three
sizes up to the million-face one, seeded at the first ring.  A tube of n rings is a path n - 1 hops long, the worst shape
for a relaxation: the point of the numbers is `rounds`, which has to follow the number of 256-vertex blocks the path
crosses (nv / 256), not its hops.  Whole-call wall times (the argument checks, the one upload, the launches with the
marks read back once a batch, the one download), best and median of `--reps` after one warm-up call, with the rounds, the
batches, the launches and a sha256 of the field; beside each, scipy's Dijkstra on the same host as context, where scipy is
installed, and whether it returns the same bits.  Nothing on the commit before does this work, so no time is compared
and none is promised.  Prints one JSON line and writes it to profiles/bench_geodesic.json.

    python tools/bench_geodesic.py [--rings 1251,12501,125001] [--reps 5] [--skip-scipy]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multimoda_rs_amd as mm  # noqa: E402
from bench_mesh_refine import _best  # noqa: E402


def thin_tube(n_rings, n_around=4, radius=1.0):
    c = np.stack([np.zeros(n_rings), np.zeros(n_rings), 0.25 * np.arange(n_rings, dtype=float)], 1)
    return mm.synth._tube(c, np.tile([1.0, 0, 0], (n_rings, 1)), np.tile([0, 1.0, 0], (n_rings, 1)), radius, n_around)


def scipy_dijkstra(v, f, seeds):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.stack([e.min(axis=1), e.max(axis=1)], 1), axis=0)
    d = v[e[:, 1]] - v[e[:, 0]]
    w = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    g = csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                   shape=(len(v), len(v)))
    t0 = time.perf_counter()
    dist = dijkstra(g, directed=True, indices=np.asarray(seeds), min_only=True)
    return (time.perf_counter() - t0) * 1e3, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", default="1251,12501,125001")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_geodesic.json"))
    a = ap.parse_args()
    out = {"bench": "centerline_from_mesh", "time": "whole call, wall clock, ms", "cases": []}
    with mm.Engine() as eng:
        for n_rings in (int(x) for x in a.rings.split(",")):
            v, f = thin_tube(n_rings)
            v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
            seeds = np.arange(4, dtype=np.int64)
            field = lambda: mm.mesh_geodesic_distance((v, f), seeds, engine=eng)          # noqa: E731
            field()
            t_min, t_median, (dist, pred, rep) = _best(field, a.reps)
            s_min, s_median, graph = _best(lambda: mm.mesh_skeleton((v, f), seeds, engine=eng), a.reps)
            c_min, c_median, (cl, crep) = _best(lambda: mm.centerline_from_mesh((v, f), seeds, engine=eng), a.reps)
            case = {"n_rings": n_rings, "vertices": int(len(v)), "faces": int(len(f)), "hops": n_rings - 1,
                    "blocks_of_256": (len(v) + 255) // 256, "rounds": rep["rounds"], "n_batches": rep["n_batches"],
                    "n_launches": rep["n_launches"], "field_ms_min": t_min, "field_ms_median": t_median,
                    "skeleton_ms_min": s_min, "skeleton_ms_median": s_median, "skeleton_launches": graph.report["n_launches"],
                    "nodes": int(len(graph.nodes)), "node_edges": int(len(graph.edges)), "band_mm": graph.report["band_mm"],
                    "centerline_ms_min": c_min, "centerline_ms_median": c_median, "centerline_points": len(cl),
                    "branches": crep["n_branches"], "max_dist": rep["max_dist"],
                    "sha256": hashlib.sha256(dist.tobytes() + pred.tobytes()).hexdigest()}
            if not a.skip_scipy:
                try:
                    case["scipy_dijkstra_ms"], want = scipy_dijkstra(v, f, seeds)
                    case["equals_scipy"] = bool(np.array_equal(want.view(np.uint64), dist.view(np.uint64)))
                except ImportError:
                    case["scipy_dijkstra_ms"] = None
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
