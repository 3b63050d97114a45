"""Timing of the CCTA branch labelling (not part of bench.py): label_branches in one launch (csrc/mm_branch_kernels.hip)
beside the route it replaces -- one find_centerline_bounded_points_simple call per branch (B + 1 uploads and launches)
and the split of the point list on the host -- on the same inputs, as whole-call wall times (every call ends in a device
synchronise).  N mesh points in a shell around a tree of B branches with about M centerline points in all.  Both routes
are warmed up at every shape, then timed alternately; the two agree list by list (checked here once per shape).  Prints
one JSON line.

    python tools/bench_branch_label.py [--n 20000 200000] [--m 2000] [--branches 2 6] [--reps 15] [--only new|old]

--only runs one route alone (no comparison, no timing of the other): for a kernel-trace run of one of them.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimoda_rs_amd as mm  # noqa: E402
from multimoda_rs_amd.centerline import Centerline  # noqa: E402


def tree(m, n_branches, seed):
    """A main vessel along x and n_branches - 1 side branches leaving it, about m points in all, 0.3 mm apart."""
    r = np.random.default_rng(seed)
    per = max(m // n_branches, 8)
    parts, ids = [], []
    main = np.stack([0.3 * np.arange(per), 3.0 * np.sin(0.01 * np.arange(per)), np.zeros(per)], 1)
    parts.append(main), ids.append(np.zeros(per, dtype=np.uint32))
    for b in range(1, n_branches):
        k = int(r.integers(per // 8, per - per // 8))
        d = r.normal(size=3)
        d[0] = 0.3 * d[0]
        d /= np.linalg.norm(d)
        parts.append(main[k] + 0.3 * np.arange(1, per + 1)[:, None] * d)
        ids.append(np.full(per, b, dtype=np.uint32))
    xyz = np.concatenate(parts)
    return Centerline.from_arrays(xyz, np.zeros_like(xyz), branch_id=np.concatenate(ids))


def shell(cl, n, seed):
    """n points 1 .. 4 mm from random centerline points: most within the 3 mm radius of some branch, some of none."""
    r = np.random.default_rng(seed)
    c = cl.xyz()[r.integers(0, len(cl), n)]
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(c + r.uniform(1.0, 4.0, (n, 1)) * d)


def old_route(cl, pts, radius, eng):
    """labeling.py:453-487 on find_centerline_bounded_points_simple: B + 1 device searches, host set logic between them"""
    find = mm.find_centerline_bounded_points_simple
    found = find(cl.get_branch(0), pts, radius, engine=eng)
    row = np.dtype((np.void, 24))                                           # `p in main_set` as one sorted numpy lookup on whole rows
    in_main = np.isin(pts.view(row).ravel(), found.view(row).ravel())       # (about half the time of a Python set of tuples)
    out = {"p_main": pts[in_main], "p_side": pts[~in_main]}
    for k in range(1, len(cl.branch_start_indices)):
        out[f"p_side_{k}"] = find(cl.get_branch(k), out["p_side"], radius, engine=eng)
    return out


def new_route(cl, pts, radius, eng):
    with contextlib.redirect_stdout(io.StringIO()):                         # label_branches prints the reference's log lines
        return mm.label_branches(cl, {"p": pts}, results_key="p", bounding_sphere_radius_mm=radius, engine=eng)


def stats(t):
    t = np.sort(np.array(t)) * 1e3
    return {"min_ms": float(t[0]), "median_ms": float(np.median(t)), "p90_ms": float(t[int(0.9 * (len(t) - 1))]),
            "max_ms": float(t[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--branches", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--only", choices=["new", "old"], default=None)
    a = ap.parse_args()
    out = {"bench": "branch_label", "m": a.m, "reps": a.reps, "radius": a.radius, "cases": []}
    routes = {"new": new_route, "old": old_route}
    with mm.Engine() as eng:
        for nb in a.branches:
            cl = tree(a.m, nb, 7 + nb)
            for n in a.n:
                pts = shell(cl, n, n + nb)
                case = {"n": n, "branches": nb, "centerline_points": len(cl)}
                run = [k for k in routes if a.only in (None, k)]
                res = {}
                for _ in range(a.warmup):
                    for k in run:
                        res[k] = routes[k](cl, pts, a.radius, eng)
                if a.only is None:
                    for key, v in res["old"].items():
                        if not np.array_equal(res["new"][key].view(np.uint64), v.view(np.uint64)):
                            raise SystemExit(f"the two routes differ in {key} at n = {n}, branches = {nb}")
                    case["lists_equal"] = True
                    case["main"], case["side"] = int(len(res["old"]["p_main"])), int(len(res["old"]["p_side"]))
                times = {k: [] for k in run}
                for _ in range(a.reps):                                     # alternating: both see the same noise
                    for k in run:
                        t0 = time.perf_counter()
                        routes[k](cl, pts, a.radius, eng)
                        times[k].append(time.perf_counter() - t0)
                for k in run:
                    case[k] = stats(times[k])
                if a.only is None:
                    case["old_over_new_median"] = case["old"]["median_ms"] / case["new"]["median_ms"]
                out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
