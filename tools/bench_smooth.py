"""Timing of the CCTA mesh finishing (not part of bench.py): mm.filter_taubin at 10 iterations on a synthetic capped tube
of about 2 * 10^5 and 10^6 vertices (the cap centres have rows as long as a ring: the longest-row cost is in the numbers),
as whole-call wall times of the device path (csrc/mm_smooth_kernels.hip) at 0, 1 and 10 steps -- so that the time of a
step ((t10 - t1) / 9) separates from what every call pays (upload, adjacency build, two volumes, displacement, download:
t1 minus one step) -- with the adjacency build timed on its own (mm.mesh_adjacency_csr, its download included) and the
bytes each way.  Beside it, on the same input: the numpy checker (tests/mm_checkers/smooth_mesh.py) and scipy.sparse CSR
`dot` with sorted indices (up to 16 threads for whatever of numpy / scipy uses them).  The three results are compared bit
for bit after the timing.  Prints one JSON line and writes it to profiles/bench_smooth.json.

    python tools/bench_smooth.py [--sizes 400x500,1000x1000] [--reps 5] [--skip-checker] [--out profiles/bench_smooth.json]
"""
import argparse
import json
import os
import sys
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, "16")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multimoda_rs_amd as mm  # noqa: E402
from mm_checkers import smooth_mesh as SMO  # noqa: E402


def capped_tube(n_around, n_rings, seed=0):
    z = np.arange(n_rings, dtype=float) * (2.0 * np.pi / n_around)
    v, f = mm.synth._tube(np.stack([np.zeros(n_rings), np.zeros(n_rings), z], 1), np.tile([1.0, 0, 0], (n_rings, 1)),
                          np.tile([0, 1.0, 0], (n_rings, 1)), 1.0, n_around)
    nv = v.shape[0]
    v = np.concatenate([v, [[0, 0, z[0]], [0, 0, z[-1]]]])
    k = np.arange(n_around)
    top = (n_rings - 1) * n_around
    caps = np.concatenate([np.stack([np.full(n_around, nv), (k + 1) % n_around, k], 1),
                           np.stack([np.full(n_around, nv + 1), top + k, top + (k + 1) % n_around], 1)])
    v = v + 0.02 * (2.0 * np.pi / n_around) * np.random.default_rng(seed).standard_normal(v.shape)
    return np.ascontiguousarray(v), np.ascontiguousarray(np.concatenate([f, caps]).astype(np.int64))


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
    ap.add_argument("--sizes", default="400x500,1000x1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-checker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_smooth.json"))
    a = ap.parse_args()
    out = {"bench": "smooth", "lamb": 0.5, "nu": 0.5, "iterations": 10, "cases": []}
    with mm.Engine() as eng:
        for size in a.sizes.split(","):
            n_around, n_rings = (int(x) for x in size.split("x"))
            v, f = capped_tube(n_around, n_rings)
            case = {"n_around": n_around, "n_rings": n_rings, "vertices": int(len(v)), "faces": int(len(f)),
                    "bytes_up": int(len(f) * 12 + len(v) * 24), "bytes_down": int(len(v) * 24 + 256)}
            run = lambda n: mm.smooth_mesh((v, f), SMO.taubin_factors(0.5, 0.5, n), engine=eng)       # noqa: E731
            run(10)
            t = {}
            for n in (0, 1, 10):
                t[n] = _best(lambda: run(n), a.reps)
                case[f"steps{n}_ms_min"], case[f"steps{n}_ms_median"] = t[n][0], t[n][1]
            got, rep = t[10][2]
            case["per_step_ms"] = (t[10][0] - t[1][0]) / 9.0
            case["per_call_ms"] = t[1][0] - case["per_step_ms"]
            csr = _best(lambda: mm.mesh_adjacency_csr(f, len(v), engine=eng), a.reps)
            case["csr_call_ms_min"], case["csr_call_ms_median"] = csr[0], csr[1]
            case["report"] = {k: (int(x) if isinstance(x, (int, np.integer)) else float(x)) for k, x in rep.items()}
            case["gather_bytes_per_step"] = int((csr[2][2]["entries"] * (24 + 4)) + len(v) * (24 + 24 + 8))
            if not a.skip_checker:
                import scipy.sparse as sp
                t0 = time.perf_counter()
                want, _ = SMO.smooth(v, f, SMO.taubin_factors(0.5, 0.5, 10))
                case["checker_ms"] = (time.perf_counter() - t0) * 1e3
                off, nb, _ = csr[2]
                t0 = time.perf_counter()
                deg = np.diff(off)
                L = sp.csr_matrix((np.repeat(1.0 / deg, deg), nb, off), shape=(len(v), len(v)))
                case["scipy_build_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                x = v.copy()
                for fac in SMO.taubin_factors(0.5, 0.5, 10):
                    x = x + fac * (L.dot(x) - x)
                case["scipy_steps_ms"] = (time.perf_counter() - t0) * 1e3
                case["identical_to_checker"] = _bits(got[0], want)
                case["identical_to_scipy"] = _bits(got[0], x)
            out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
