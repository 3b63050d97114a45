"""Timing of the CCTA mesh closing (not part of bench.py): fill_holes on the aortic sub-mesh of the take-off mesh (about
10^6 faces; its two rims and two ostia are filled) and on the stitched mesh of tools/bench_stitch.py, and
smooth_mesh_labels(faces=...) for 1, 5 and 20 iterations on the take-off mesh with a few percent of banded labels
flipped at random, as whole-call wall times of the device path (csrc/mm_close_kernels.hip, csrc/mm_weld_kernels.hip)
beside the plain numpy / Python checker (tests/mm_checkers/close_mesh.py) on the same input.  The two agree bit for bit
(checked here once).  Prints one JSON line and writes it to profiles/bench_close.json.

    python tools/bench_close.py [--theta 1024] [--rings 500] [--reps 5] [--skip-checker] [--out profiles/bench_close.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import multimoda_rs_amd as mm  # noqa: E402
from mm_checkers import close_mesh as CM  # noqa: E402
from bench_stitch import _best, parts_of  # noqa: E402


def _same(got, want):
    return bool(np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1]) and
                np.float64(got[2]["volume"]).view(np.uint64) == np.float64(want[2]["volume"]).view(np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--theta", type=int, default=1024)
    ap.add_argument("--rings", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_close.json"))
    a = ap.parse_args()
    out = {"bench": "close"}
    v, f, _, cr, _, n_aorta_faces = mm.synth.synthetic_takeoff_mesh(n_theta=a.theta, n_z=a.rings)
    na = v.shape[0] - 2 * len(cr) * 16
    av, af = v[:na], f[:n_aorta_faces]
    af = af[(af < na).all(axis=1)]
    r = np.random.default_rng(0)
    n_labels = 5
    labels = (np.arange(len(v)) * n_labels // len(v)).astype(np.uint8)
    noise = r.random(len(v)) < 0.03
    labels[noise] = r.integers(0, n_labels, int(noise.sum()))
    with mm.Engine() as eng:
        sv, sf, _ = mm.assemble_mesh(parts_of(a.theta, a.rings, eng), engine=eng)
        cases = {"aorta": (av, af), "stitched": (sv, sf)}
        got = {}
        for name, (cv, cf) in cases.items():
            fill = lambda: mm.fill_holes(cv, cf, engine=eng)                          # noqa: E731
            fill()
            out[f"fill_{name}_ms_min"], out[f"fill_{name}_ms_median"], got[name] = _best(fill, a.reps)
            rep = got[name][2]
            out[f"fill_{name}"] = {"faces_in": int(len(cf)), "faces": int(rep["n_faces"]), "loops": int(rep["n_loops_filled"]),
                                   "fan_faces": int(rep["n_fan_faces"]), "winding_rounds": int(rep["winding_rounds"]),
                                   "irregular_components": int(rep["n_irregular_components"]),
                                   "open_edges": int(rep["n_open_edges"])}
        smoothed = {}
        for it in (1, 5, 20):
            smooth = lambda: mm.ccta.smooth_mesh_labels_info(labels, iterations=it, faces=f, engine=eng)   # noqa: E731
            smooth()
            out[f"smooth_{it}_ms_min"], out[f"smooth_{it}_ms_median"], smoothed[it] = _best(smooth, a.reps)
            out[f"smooth_{it}"] = smoothed[it][1]
        out.update(smooth_vertices=int(len(v)), smooth_faces=int(len(f)), labels_flipped=int(noise.sum()))
    if not a.skip_checker:
        same = True
        for name, (cv, cf) in cases.items():
            t0 = time.perf_counter()
            want = CM.fill_holes(cv, cf)
            out[f"checker_fill_{name}_ms"] = (time.perf_counter() - t0) * 1e3
            same &= _same(got[name], want)
        rows = CM.adjacency_of_faces(f, len(v))
        for it in (1, 5, 20):
            t0 = time.perf_counter()
            want, _ = CM.smooth_labels(labels, rows, it)
            out[f"checker_smooth_{it}_ms"] = (time.perf_counter() - t0) * 1e3
            same &= bool(np.array_equal(smoothed[it][0], want))
        out["identical_to_checker"] = bool(same)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
