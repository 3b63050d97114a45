"""Timing of mesh clipping (not part of bench.py): mm.clip_mesh on the million-face thin tube of tools/bench_section.py
with an inlet and an outlet LOOP cut, capped.  Reported: the whole call (wall clock; its section pass, the host's
reading of the loops and writing of the records, the copies and the kernels are NOT separated), the pointer-jumping
rounds and the report.  Beside it, as context and not as a bar, two existing calls on the same mesh: mm.mesh_cross_sections
for the same two planes, and the trim (mm_trim_mesh, remove mode) of the vertices beyond the two planes.  No time is
promised and there is no baseline: the call is new.  Prints one JSON line and writes it to profiles/bench_clip.json.

    python tools/bench_clip.py [--rings 125001] [--reps 5]
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
from bench_geodesic import thin_tube  # noqa: E402
from bench_mesh_refine import _best  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=125001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_clip.json"))
    a = ap.parse_args()
    v, f = thin_tube(a.rings)
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    z1 = 0.25 * (a.rings - 1)
    o = np.array([[0.0, 0.0, 0.1037 * z1], [0.0, 0.0, 0.9041 * z1]])
    n = np.tile([0.05, -0.03, 1.0], (2, 1))
    keep = ["above", "below"]
    out = {"bench": "clip_mesh", "time": "wall clock, ms, whole calls; sections, host records, copies and kernels not separated",
           "vertices": int(len(v)), "faces": int(len(f)), "cuts": 2, "cap": True}
    with mm.Engine() as eng:
        run = lambda: mm.clip_mesh((v, f), o, n, keep=keep, cap=True, engine=eng)          # noqa: E731
        run()
        out["clip_ms_min"], out["clip_ms_median"], got = _best(run, a.reps)
        sec = lambda: mm.mesh_cross_sections((v, f), o, n, engine=eng)                     # noqa: E731
        sec()
        out["sections_ms_min"], out["sections_ms_median"], _ = _best(sec, a.reps)
        region = ((v[:, 2] < o[0, 2]) | (v[:, 2] > o[1, 2])).astype(np.uint8)
        trim = lambda: mm.ccta._trim(v, f, region, 0, 2, eng)                              # noqa: E731
        trim()
        out["trim_ms_min"], out["trim_ms_median"], trimmed = _best(trim, a.reps)
        out["trim_vertices"], out["trim_faces"] = int(len(trimmed[0])), int(len(trimmed[1]))
    h = hashlib.sha256()
    for arr in (got.vertices, got.faces, got.face_origin, got.face_kind):
        h.update(np.ascontiguousarray(arr).tobytes())
    out.update({k: x for k, x in got.report.items()})
    out["cut_area"], out["sha256"] = got.cut_area.tolist(), h.hexdigest()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
