"""Timing of the CCTA mesh refinement (not part of bench.py; tools/bench_refine.py is the alignment refinement, another
thing): mm.refine_mesh on a synthetic capped tube with a little noise, whose rings are `stretch` times as far apart as
their points, so that a target at the ring's own edge length splits the long edges only.  Whole-call wall times of the
device path (csrc/mm_refine_kernels.hip: upload, every pass, the two volumes, download, the widening to int64) at a few
sizes, with the passes, splits, launches and bytes of the report, and the same for mm.mesh_edge_lengths.  On the smallest
size the result is compared bit for bit with the Python checker (tests/mm_checkers/refine_mesh.py, plain Python: its time
is printed but is no baseline).  Prints one JSON line and writes it to profiles/bench_mesh_refine.json.

    python tools/bench_mesh_refine.py [--sizes 100x50,400x125,1000x250] [--stretch 4] [--reps 5] [--skip-checker]
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
from mm_checkers import refine_mesh as R  # noqa: E402


def capped_tube(n_around, n_rings, stretch, seed=0):
    step = 2.0 * np.pi / n_around
    z = np.arange(n_rings, dtype=float) * step * stretch
    v, f = mm.synth._tube(np.stack([np.zeros(n_rings), np.zeros(n_rings), z], 1), np.tile([1.0, 0, 0], (n_rings, 1)),
                          np.tile([0, 1.0, 0], (n_rings, 1)), 1.0, n_around)
    nv = v.shape[0]
    v = np.concatenate([v, [[0, 0, z[0]], [0, 0, z[-1]]]])
    k = np.arange(n_around)
    top = (n_rings - 1) * n_around
    caps = np.concatenate([np.stack([np.full(n_around, nv), (k + 1) % n_around, k], 1),
                           np.stack([np.full(n_around, nv + 1), top + k, top + (k + 1) % n_around], 1)])
    v = v + 0.02 * step * np.random.default_rng(seed).standard_normal(v.shape)
    return np.ascontiguousarray(v), np.ascontiguousarray(np.concatenate([f, caps]).astype(np.int64)), step


def _best(fn, reps):
    times, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), float(np.median(times)), res


def _bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,400x125,1000x250")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mesh_refine.json"))
    a = ap.parse_args()
    out = {"bench": "mesh_refine", "ratio": 4.0 / 3.0, "stretch": a.stretch, "cases": []}
    with mm.Engine() as eng:
        for i, size in enumerate(a.sizes.split(",")):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            case = {"n_around": n_around, "n_rings": n_rings, "vertices": int(len(v)), "faces": int(len(f)), "target": step}
            run = lambda: mm.refine_mesh((v, f), step, engine=eng)                                    # noqa: E731
            run()
            t = _best(run, a.reps)
            case["refine_ms_min"], case["refine_ms_median"] = t[0], t[1]
            mesh, parents, rep = t[2]
            case["report"] = {k: (x if isinstance(x, list) else (int(x) if isinstance(x, (int, np.integer)) else float(x)))
                              for k, x in rep.items()}
            e = _best(lambda: mm.mesh_edge_lengths((v, f), engine=eng), a.reps)
            case["edge_lengths_ms_min"], case["edge_lengths_ms_median"] = e[0], e[1]
            t0 = time.perf_counter()
            case["auto_target"] = mm.edge_length_target((v, f), engine=eng)
            case["auto_target_ms"] = (time.perf_counter() - t0) * 1e3
            if i == 0 and not a.skip_checker:
                t0 = time.perf_counter()
                wv, wf, wp, _ = R.refine(v, f, step)
                case["checker_ms"] = (time.perf_counter() - t0) * 1e3
                case["identical_to_checker"] = bool(_bits(mesh[0], wv) and np.array_equal(mesh[1], wf)
                                                    and np.array_equal(parents, wp))
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
