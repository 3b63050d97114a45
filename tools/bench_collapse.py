"""Timing of the mesh edge collapse and of the composite remesh (not part of bench.py): mm.collapse_edges and
mm.isotropic_remesh on the refined noisy capped tubes of tools/bench_surface.py, at a target of 1.5 times the length the
tubes were refined at, so that there is something to collapse.  Whole-call wall times (the argument checks, the one
upload, every pass with its 128 bytes of counters read back, the compaction, the one download; for the remesh the four
calls of every iteration, each from its own upload), with the passes, the collapses, the launches and the bytes each way,
and the Hausdorff distance (mm.surface_distance) between the input and the result, which is what MeshLab's checksurfdist
would bound; the plain Python checker (tests/mm_checkers/collapse_edges.py) on the smallest size only.  Nothing on the
commit before does this work, so no time is compared and none is promised.  Prints one JSON line and writes it to
profiles/bench_collapse.json.

    python tools/bench_collapse.py [--sizes 100x50,200x100,400x125] [--stretch 4] [--reps 5] [--iterations 3] [--skip-checker]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multimoda_rs_amd as mm  # noqa: E402
from bench_flip import min_angles  # noqa: E402
from bench_mesh_refine import _best, capped_tube  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_collapse.json"))
    a = ap.parse_args()
    out = {"bench": "collapse_edges", "stretch": a.stretch, "target_over_step": 1.5, "crease_deg": 30.0, "quality_keep": 0.5,
           "remesh_iterations": a.iterations, "cases": []}
    with mm.Engine() as eng:
        for i, size in enumerate(a.sizes.split(",")):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            fine = mm.refine_mesh((v, f), step, engine=eng)[0]
            target = 1.5 * step
            run = lambda: mm.collapse_edges(fine, target, engine=eng)                       # noqa: E731
            run()
            t_min, t_median, (new, origin, tgt, rep) = _best(run, a.reps)
            case = {"n_around": n_around, "n_rings": n_rings, "vertices": int(len(fine[0])), "faces": int(len(fine[1])),
                    "target": target, "ms_min": t_min, "ms_median": t_median,
                    **{k: rep[k] for k in mm.ccta.COLLAPSE_REPORT_KEYS}, "collapses_per_pass": rep["collapses_per_pass"],
                    "hausdorff": mm.surface_distance(fine, new, engine=eng).hausdorff,
                    "min_angle_worst_mean": {"refined": min_angles(fine), "collapsed": min_angles(new)},
                    "sha256": hashlib.sha256(new[0].tobytes() + new[1].tobytes() + tgt.tobytes()).hexdigest()}
            if i == 0 and not a.skip_checker:
                from mm_checkers import collapse_edges as CE
                t0 = time.perf_counter()
                want = CE.collapse(fine[0], fine[1], target)
                case["checker_ms"] = (time.perf_counter() - t0) * 1e3
                case["equals_checker"] = bool(np.array_equal(want[1], new[1]) and np.array_equal(want[3], tgt) and
                                              want[0].tobytes() == new[0].tobytes())
            remesh = lambda: mm.isotropic_remesh(fine, target, iterations=a.iterations, engine=eng)   # noqa: E731
            remesh()
            r_min, r_median, (iso, irep) = _best(remesh, a.reps)
            case["remesh"] = {"ms_min": r_min, "ms_median": r_median, "vertices": int(len(iso[0])), "faces": int(len(iso[1])),
                              "share_in_range_before": irep["share_in_range_before"],
                              "share_in_range_after": irep["share_in_range_after"],
                              "collapses": [it["collapse"]["n_collapses"] for it in irep["iterations"]],
                              "collapse_passes": [it["collapse"]["passes_run"] for it in irep["iterations"]],
                              "flips": [it["flip"]["n_flips"] for it in irep["iterations"]],
                              "launches": [sum(it[k]["n_launches"] for k in ("refine", "collapse", "flip", "relax"))
                                           for it in irep["iterations"]],
                              "hausdorff": mm.surface_distance(fine, iso, engine=eng).hausdorff,
                              "min_angle_worst_mean": min_angles(iso)}
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
