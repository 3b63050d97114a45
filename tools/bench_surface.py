"""Timing of the surface distance (not part of bench.py): mm.surface_distance on the noisy capped tube of
tools/bench_mesh_refine.py against its refined and Taubin-smoothed self, at a few sizes.  Whole-call wall times (the
lattice samples in numpy, the host staging and work items, both uploads, every launch of both directions, both
downloads, the means), with the distances and, per direction, the items of pass A and pass B, the items pass B skipped,
the launches and the bytes each way, and a sha256 over every figure of the report but the skipped items.  No time is
promised and there is no baseline: the call is new, and the checker (tests/mm_checkers/surface_distance.py) is numpy, a
yardstick for bits and not for speed.  Prints one JSON line and writes it to profiles/bench_surface.json.

    python tools/bench_surface.py [--sizes 100x50,200x100,400x125] [--stretch 4] [--samples 1] [--reps 5]
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
from bench_mesh_refine import _best, capped_tube  # noqa: E402


def _direction(d):
    return {"n": d.n, "max": d.max, "mean": d.mean, "rms": d.rms, **d.report}


def _digest(rep):
    """sha256 over every figure of both directions, floats by their bits"""
    h = hashlib.sha256()
    for d in (rep.a_to_b, rep.b_to_a):
        h.update(np.array([d.max, d.mean, d.rms, *d.closest], dtype=np.float64).tobytes())
        counts = {k: n for k, n in d.report.items() if k != "items_skipped"}   # what pass B skips depends on its schedule
        h.update(json.dumps([d.argmax, d.sample_face, d.face, d.n, counts], sort_keys=True).encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x50,200x100,400x125")
    ap.add_argument("--stretch", type=float, default=4.0)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_surface.json"))
    a = ap.parse_args()
    out = {"bench": "surface_distance", "stretch": a.stretch, "samples": a.samples, "cases": []}
    with mm.Engine() as eng:
        for size in a.sizes.split(","):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f, step = capped_tube(n_around, n_rings, a.stretch)
            fine = mm.refine_mesh((v, f), step, engine=eng)[0]
            smooth = mm.smooth_mesh(fine, engine=eng)[0]
            run = lambda: mm.surface_distance((v, f), smooth, samples=a.samples, engine=eng)        # noqa: E731
            run()
            t_min, t_median, rep = _best(run, a.reps)
            t0 = time.perf_counter()
            mm.sample_mesh_surface((v, f), a.samples), mm.sample_mesh_surface(smooth, a.samples)
            sample_ms = (time.perf_counter() - t0) * 1e3
            out["cases"].append({"n_around": n_around, "n_rings": n_rings, "faces_a": int(len(f)), "faces_b": int(len(smooth[1])),
                                 "ms_min": t_min, "ms_median": t_median, "sampling_ms": sample_ms,
                                 "hausdorff": rep.hausdorff, "a_to_b": _direction(rep.a_to_b), "b_to_a": _direction(rep.b_to_a),
                                 "n_launches": rep.n_launches, "bytes_uploaded": rep.bytes_uploaded,
                                 "bytes_downloaded": rep.bytes_downloaded, "sha256": _digest(rep)})
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
