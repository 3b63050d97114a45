"""Timing of the winding number (not part of bench.py): mm.mesh_winding_number on two shapes -- a large one (a
million-face open tube against 256 k queries; the cost is queries x faces, nothing is pruned) and a clinical one (a
coronary's 20 000 vertices against a 200 000-face aortic wall) -- beside mm.point_mesh_distance on the same inputs for
scale.  Whole-call wall times (argument checks, the removal of degenerate faces, staging, upload, both launches, download,
w and err on the host), with the report, the classification counts and a sha256 over the
device's (turns, p, rho, touch).  No time is promised and there is no baseline: the call is new.  Prints one JSON line
and writes it to profiles/bench_winding.json.

    python tools/bench_winding.py [--shapes 1000000x262144,200000x20000] [--reps 3]
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

import multimoda_rs_amd as mm  # noqa: E402


def open_tube(n_faces, radius=10.0, length=80.0):
    """an open tube of about n_faces faces (square-ish quads), outward"""
    n_around = max(3, int(round(np.sqrt(n_faces / 2 * (2 * np.pi * radius) / length))))
    n_along = max(1, int(round(n_faces / 2 / n_around)))
    j = np.arange(n_around)
    ring = np.stack([radius * np.cos(2 * np.pi * j / n_around), radius * np.sin(2 * np.pi * j / n_around)], axis=1)
    z = length * (np.arange(n_along + 1) / n_along - 0.5)
    v = np.concatenate([np.repeat(ring[None], n_along + 1, axis=0), np.repeat(z[:, None, None], n_around, axis=1)], axis=2)
    i0 = (np.arange(n_along)[:, None] * n_around + j[None, :]).reshape(-1)
    i1 = (np.arange(n_along)[:, None] * n_around + ((j + 1) % n_around)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i0, i1, i1 + n_around], axis=1), np.stack([i0, i1 + n_around, i0 + n_around], axis=1)])
    return np.ascontiguousarray(v.reshape(-1, 3)), np.ascontiguousarray(f.astype(np.int64))


def _best(run, reps):
    times, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = run()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), float(np.median(times)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x262144,200000x20000", help="faces x queries, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_winding.json"))
    a = ap.parse_args()
    out = {"bench": "mesh_winding_number", "cases": []}
    rng = np.random.default_rng(0)
    with mm.Engine() as eng:
        for shape in a.shapes.split(","):
            n_faces, nq = (int(x) for x in shape.split("x"))
            v, f = open_tube(n_faces)
            q = rng.uniform(-1.0, 1.0, size=(nq, 3)) * np.array([15.0, 15.0, 50.0])
            run = lambda: mm.mesh_winding_number(q, (v, f), engine=eng)                              # noqa: E731
            run()
            t_min, t_median, r = _best(run, a.reps)
            print(f"{len(f)} faces x {nq} queries: winding number {t_min:.2f} ms", file=sys.stderr, flush=True)
            dist = lambda: mm.point_mesh_distance(q, (v, f), engine=eng)                            # noqa: E731
            dist()
            d_min, d_median, _ = _best(dist, a.reps)
            h = hashlib.sha256()
            for arr in (r.turns, r.p, r.rho, r.touch):
                h.update(np.ascontiguousarray(arr).tobytes())
            pairs = float(nq) * r.report["n_staged_faces"]
            out["cases"].append({"faces": int(len(f)), "queries": nq, "ms_min": t_min, "ms_median": t_median,
                                 "pairs_per_s_at_min": pairs / (t_min * 1e-3),
                                 "point_mesh_distance_ms_min": d_min, "point_mesh_distance_ms_median": d_median,
                                 "inside": int((r.inside == 1).sum()), "outside": int((r.inside == 0).sum()),
                                 "undecided": int((r.inside == -1).sum()), "largest_finite_err": float(r.err[np.isfinite(r.err)].max()),
                                 **r.report, "sha256": h.hexdigest()})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
