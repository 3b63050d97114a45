"""Timing of the mesh relaxation (not part of bench.py): mm.relax_mesh on the refined noisy capped tubes of
tools/bench_surface.py, relaxed on themselves.  Whole-call wall times (the host's free-vertex and plan work, the one
upload, every launch of step 0 and the iterations, the one download), with the items run and skipped and the bytes each
way.  Beside it the cost of the same projections through the public calls of the commit before: iterations + 1 calls
of mm.point_mesh_distance on the same queries (the free vertices; their positions do not change between these calls,
so this is a lower estimate: it leaves out the host's averaging and guard in between).  No time is promised.  Prints one
JSON line and writes it to profiles/bench_relax.json.

    python tools/bench_relax.py [--sizes 100x50,200x100,400x125] [--stretch 4] [--iterations 5] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--lamb", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_relax.json"))
    a = ap.parse_args()
    out = {"bench": "relax_mesh", "stretch": a.stretch, "iterations": a.iterations, "lamb": a.lamb, "cases": []}
    with mm.Engine() as eng:
        for size in a.sizes.split(","):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            fine = mm.refine_mesh((v, f), step, engine=eng)[0]
            run = lambda: mm.relax_mesh(fine, iterations=a.iterations, lamb=a.lamb, engine=eng)     # noqa: E731
            run()
            t_min, t_median, (new, face, rep) = _best(run, a.reps)
            queries = np.ascontiguousarray(fine[0][face >= 0])

            def composed():
                for _ in range(a.iterations + 1):
                    r = mm.point_mesh_distance(queries, fine, engine=eng)
                return r

            composed()
            c_min, c_median, r = _best(composed, a.reps)
            digest = hashlib.sha256(np.ascontiguousarray(new[0]).tobytes() + face.tobytes()).hexdigest()
            out["cases"].append({"n_around": n_around, "n_rings": n_rings, "vertices": int(len(fine[0])),
                                 "faces": int(len(fine[1])), "ms_min": t_min, "ms_median": t_median,
                                 "composed_calls": a.iterations + 1, "composed_ms_min": c_min,
                                 "composed_ms_median": c_median, "composed_bytes_uploaded": (a.iterations + 1) * r.report["bytes_uploaded"],
                                 "composed_bytes_downloaded": (a.iterations + 1) * r.report["bytes_downloaded"],
                                 **{k: rep[k] for k in mm.ccta.RELAX_REPORT_KEYS}, "sha256": digest})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
