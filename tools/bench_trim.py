"""Timing of the CCTA mesh trimming (not part of bench.py): remove_labeled_points_from_mesh of a band of the aortic wall
and keep_labeled_points_from_mesh of the aorta minus that band, on a synthetic take-off mesh of about 10^6 faces, as
wall times of the device path (csrc/mm_trim_kernels.hip and the host rim logic) beside the plain numpy / Python checker
(tests/mm_checkers/trim_mesh.py) on the same input.  The two agree bit for bit (checked here once).  Prints one JSON
line.

    python tools/bench_trim.py [--theta 1024] [--rings 500] [--reps 5] [--skip-checker]
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
from mm_checkers import trim_mesh as TM  # noqa: E402


def _best(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3, float(np.median(times)) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=1024)
    ap.add_argument("--rings", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    a = ap.parse_args()
    v, f, *_ = mm.synth.synthetic_takeoff_mesh(n_theta=a.theta, n_z=a.rings)
    band = (v[:, 2] > 20.0) & (v[:, 2] < 26.0) & (v[:, 0] > 0.0)
    res = {"mesh": (v, f), "anomalous_points": v[band], "aorta_points": v[~band]}
    out = {"bench": "trim", "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "removed": int(band.sum())}
    with mm.Engine() as eng:
        remove = lambda: mm.remove_labeled_points_from_mesh(dict(res), "anomalous_points", engine=eng)   # noqa: E731
        keep = lambda: mm.keep_labeled_points_from_mesh(dict(res), "aorta_points", engine=eng)          # noqa: E731
        remove()
        out["remove_ms_min"], out["remove_ms_median"], got_r = _best(remove, a.reps)
        out["keep_ms_min"], out["keep_ms_median"], got_k = _best(keep, a.reps)
        out["rings_remove"] = [len(got_r[k]) for k in sorted(got_r) if k.startswith("boundary_points_")]
    if not a.skip_checker:
        t0 = time.perf_counter()
        want_r = TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points")
        out["checker_remove_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        want_k = TM.keep_labeled_points_from_mesh(dict(res), "aorta_points")
        out["checker_keep_ms"] = (time.perf_counter() - t0) * 1e3
        same = True
        for g, w in ((got_r, want_r), (got_k, want_k)):
            same &= np.array_equal(g["mesh"][0].view(np.uint64), w["mesh"][0].view(np.uint64))
            same &= np.array_equal(g["mesh"][1], w["mesh"][1])
            same &= all(np.array_equal(np.asarray(g[k]), np.asarray(w[k])) for k in w if k != "mesh")
        out["identical_to_checker"] = bool(same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
