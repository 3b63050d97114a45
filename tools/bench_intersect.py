"""Timing of the mesh intersection check (not part of bench.py): mm.mesh_self_intersections on the noisy capped tube of
tools/bench_mesh_refine.py (the sizes tools/bench_surface.py uses), as it comes and after refine_mesh.  Whole-call wall
times (argument checks, canonical ids, slab order, items, the upload, both launches, the downloads, the sort), and the
host plan alone through the test hook mm_isect_plan (one call, no device): `device_ms` is the difference, so it holds
the staging copy, the transfers and the sort as well as the kernels.  With the report of every case and a sha256 over
flags, pairs and states.  No time is promised and there is no baseline: the call is new, and the checker
(tests/mm_checkers/mesh_intersections.py) is Python, a yardstick for bits and not for speed.  Prints one JSON line and
writes it to profiles/bench_intersect.json.

    python tools/bench_intersect.py [--sizes 100x50,200x100,400x125] [--stretch 4] [--reps 5]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multimoda_rs_amd as mm  # noqa: E402
from bench_mesh_refine import _best, capped_tube  # noqa: E402

N = mm._native


def _plan_once(v, f):
    """one mm_isect_plan call: what the host does in front of the upload"""
    order, info = np.zeros(max(len(f), 1), dtype=np.int32), np.zeros(5, dtype=np.int64)
    N.check(N.lib().mm_isect_plan(N._ptr(v), len(v), N._ptr(f), len(f), None, 0, None, 0, N._ptr(order), None, N._ptr(info),
                                  None, None, 0), "isect_plan")
    return info


def _case(label, v, f, eng, reps):
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    run = lambda: mm.mesh_self_intersections((v, f), engine=eng)          # noqa: E731
    run()
    t_min, t_median, got = _best(run, reps)
    p_min, p_median, _ = _best(lambda: _plan_once(v, f), reps)
    h = hashlib.sha256()
    for a in (got.face_state, got.pairs, got.pair_state):
        h.update(np.ascontiguousarray(a).tobytes())
    return {"mesh": label, "vertices": int(len(v)), "faces": int(len(f)), "ms_min": t_min, "ms_median": t_median,
            "plan_ms_min": p_min, "plan_ms_median": p_median, "device_ms_min": t_min - p_min, **got.report,
            "sha256": h.hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_intersect.json"))
    a = ap.parse_args()
    out = {"bench": "mesh_self_intersections", "stretch": a.stretch, "cases": []}
    with mm.Engine() as eng:
        for size in a.sizes.split(","):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            out["cases"].append(_case(size, v, f, eng, a.reps))
            fv, ff = mm.refine_mesh((v, f), step, engine=eng)[0]
            out["cases"].append(_case(size + " refined", fv, ff, eng, a.reps))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
