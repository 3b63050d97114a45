"""Timing of the mesh edge flips (not part of bench.py): mm.flip_edges on the refined noisy capped tubes of
tools/bench_surface.py.  Whole-call wall times (the argument checks, the one upload, every pass with its 128 bytes of
counters read back, the one download), with the passes, the flips, the launches and the bytes each way; the plain Python
checker (tests/mm_checkers/flip_edges.py) on the smallest size only.  Then the quality the flips buy on the smallest
size: the worst and the mean minimum angle of the refined mesh, after the relaxation alone, after flips and relaxation,
and after a second round of both.  Nothing on the commit before does this work, so no time is compared and none is
promised.  Prints one JSON line and writes it to profiles/bench_flip.json.

    python tools/bench_flip.py [--sizes 100x50,200x100,400x125] [--stretch 4] [--reps 5] [--skip-checker]
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
from bench_mesh_refine import _best, capped_tube  # noqa: E402


def min_angles(mesh):
    """(worst, mean) over the faces of their smallest angle, degrees."""
    v, f = np.asarray(mesh[0]), np.asarray(mesh[1])
    a = v[f]
    out = []
    for k in range(3):
        u, w = a[:, (k + 1) % 3] - a[:, k], a[:, (k + 2) % 3] - a[:, k]
        cos = (u * w).sum(axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(w, axis=1))
        out.append(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))))
    m = np.min(out, axis=0)
    return [round(float(m.min()), 3), round(float(m.mean()), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_flip.json"))
    a = ap.parse_args()
    out = {"bench": "flip_edges", "stretch": a.stretch, "crease_deg": 30.0, "quality_keep": 0.5, "cases": []}
    with mm.Engine() as eng:
        for i, size in enumerate(a.sizes.split(",")):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            fine = mm.refine_mesh((v, f), step, engine=eng)[0]
            run = lambda: mm.flip_edges(fine, engine=eng)                                  # noqa: E731
            run()
            t_min, t_median, (new, rep) = _best(run, a.reps)
            case = {"n_around": n_around, "n_rings": n_rings, "vertices": int(len(fine[0])), "faces": int(len(fine[1])),
                    "ms_min": t_min, "ms_median": t_median, **{k: rep[k] for k in mm.ccta.FLIP_REPORT_KEYS},
                    "flips_per_pass": rep["flips_per_pass"], "sha256": hashlib.sha256(new[1].tobytes()).hexdigest()}
            if i == 0:
                if not a.skip_checker:
                    from mm_checkers import flip_edges as FE
                    t0 = time.perf_counter()
                    want = FE.flip(fine[0], fine[1])[0]
                    case["checker_ms"] = (time.perf_counter() - t0) * 1e3
                    case["equals_checker"] = bool(np.array_equal(want, new[1]))
                relaxed = mm.relax_mesh(fine, engine=eng)[0]
                both = mm.relax_mesh(new, engine=eng)[0]
                second = mm.relax_mesh(mm.flip_edges(both, engine=eng)[0], engine=eng)[0]
                case["min_angle_worst_mean"] = {"refined": min_angles(fine), "flips_only": min_angles(new),
                                                "relax_only": min_angles(relaxed), "flip_relax": min_angles(both),
                                                "two_rounds": min_angles(second)}
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
