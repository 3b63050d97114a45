"""Timing of the mesh repair (not part of bench.py): mm.repair_mesh on the noisy capped tubes of tools/bench_mesh_refine.py
with a fixed share of planted defects -- one wall face in `--every` gets a small fin on its first edge (an edge with three
owners), a small tetrahedron that touches its second corner (a bow-tie vertex) and a bit-equal copy of its third corner
that the face then names (a duplicated vertex).  Whole-call wall times (the argument checks, the one upload, the
launches with one word read back a pointer-jumping round, the counters, the one download), with the launches, the
rounds, the bytes each way and a sha256 of the outputs; the plain Python checker (tests/mm_checkers/repair_mesh.py) on the
smallest size only.  Nothing on the commit before does this work, so no time is compared and none is promised.  Prints
one JSON line and writes it to profiles/bench_repair.json.

    python tools/bench_repair.py [--sizes 100x50,200x100,400x125,800x250] [--every 200] [--reps 5] [--skip-checker]
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


def plant(v, f, every, step):
    """(vertices, faces, number of defect sites): the defects of the module docstring at every `every`-th wall face."""
    v, f = [p for p in v.tolist()], f.tolist()
    sites = range(every // 2, len(f) - 2 * every, every)                  # wall faces only: the caps are the last
    for i in sites:
        a, b, c = f[i]
        pa, pb, pc = np.array(v[a]), np.array(v[b]), np.array(v[c])
        n = len(v)
        v.append((0.5 * (pa + pb) * [1.0 + 0.1 * step, 1.0 + 0.1 * step, 1.0]).tolist())        # the fin's apex
        f.append([a, b, n])
        out = pb * [1.0, 1.0, 0.0]
        out = out / np.linalg.norm(out)
        e = 0.1 * step
        v.extend([(pb + e * out + [0, 0, e]).tolist(), (pb + e * out - [0, 0, e]).tolist(),
                  (pb + 2.0 * e * out + [e * out[1], -e * out[0], 0]).tolist()])
        f.extend([[b, n + 1, n + 2], [b, n + 3, n + 1], [b, n + 2, n + 3], [n + 1, n + 3, n + 2]])
        v.append(pc.tolist())                                              # the copy of c
        f[i] = [a, b, n + 4]
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64), len(sites)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125,800x250")
    ap.add_argument("--every", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_repair.json"))
    a = ap.parse_args()
    out = {"bench": "repair_mesh", "defect_sites_one_in": a.every, "time": "whole call, wall clock, ms", "cases": []}
    with mm.Engine() as eng:
        for i, size in enumerate(a.sizes.split(",")):
            n_around, n_rings = (int(x) for x in size.split("x"))
            tv, tf, step = capped_tube(n_around, n_rings, 1.0)
            v, f, n_sites = plant(tv, tf, a.every, step)
            run = lambda: mm.repair_mesh((v, f), engine=eng)                                 # noqa: E731
            run()
            t_min, t_median, (new, origin, tgt, rep) = _best(run, a.reps)
            t_count = _best(lambda: mm.mesh_manifold_report((v, f), eng), a.reps)[0]
            case = {"n_around": n_around, "n_rings": n_rings, "vertices": int(len(v)), "faces": int(len(f)),
                    "defect_sites": n_sites, "ms_min": t_min, "ms_median": t_median, "manifold_report_ms_min": t_count,
                    **{k: rep[k] for k in mm.ccta.REPAIR_REPORT_KEYS}, "watertight": bool(rep["watertight"]),
                    "sha256": hashlib.sha256(new[0].tobytes() + new[1].tobytes() + origin.tobytes() + tgt.tobytes()).hexdigest()}
            if i == 0 and not a.skip_checker:
                from mm_checkers import repair_mesh as RM
                t0 = time.perf_counter()
                want = RM.repair(v, f)
                case["checker_ms"] = (time.perf_counter() - t0) * 1e3
                case["equals_checker"] = bool(want[0].tobytes() == new[0].tobytes() and np.array_equal(want[1], new[1]) and
                                              np.array_equal(want[2], origin) and np.array_equal(want[3], tgt))
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
