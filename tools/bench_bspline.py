#!/usr/bin/env python3
"""Time the closed B-spline fit: the batch call (one launch) for an aorta of 441 contours of 200 points (DESIGN 4.8's
workload) and for a whole tree (441 x 100 aorta, 2 x 120 x 100 mains, 4 x 40 x 100 side branches), the numpy-free
Python checker on a sample of the same input, and -- where scipy imports -- the reference's per-contour
splprep / splev loop.  Writes profiles/bench_bspline.json."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def contours(n, m, seed):
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi, m, endpoint=False)
    out = []
    for i in range(n):
        r = (2.0 + 10.0 * (seed == 0)) * (1 + 0.15 * np.cos(3 * th + i)) + 0.05 * rng.normal(size=m)
        out.append(np.stack([1.3 * r * np.cos(th), r * np.sin(th), 0.05 * rng.normal(size=m) + i], 1))
    return out


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception as e:
        return f"unknown ({type(e).__name__})"


def versions():
    v = {"numpy": np.__version__}
    try:
        import scipy
        v["scipy"] = scipy.__version__
    except Exception:
        v["scipy"] = None
    try:
        import torch
        v["torch"], v["hip"] = torch.__version__, torch.version.hip
    except Exception:
        v["torch"] = v["hip"] = None
    try:
        import multimoda_rs_amd as mm
        v["library"] = mm._native.lib().mm_version().decode()
    except Exception:
        v["library"] = None
    return v


def main():
    import multimoda_rs_amd as mm
    from mm_checkers import bspline as B
    try:
        from scipy.interpolate import splev, splprep
    except Exception:
        splprep = None
    aorta = contours(441, 200, 0)
    tree = contours(441, 100, 0) + contours(240, 100, 1) + contours(160, 100, 2)
    res = {"device": device_name(), "versions": versions(), "checker_note": "the checker column is timed on 8 contours "
           "spread over the input and scaled to the whole input", "cases": []}
    with mm.Engine(0) as eng:
        for name, cs in (("aorta_441x200", aorta), ("tree_841x100", tree)):
            for s in (0.0, 0.0025 * cs[0].shape[0], 100.0):
                mm.fit_bspline_contours(cs, s, 3, engine=eng)                      # warm-up
                med, best = median_ms(lambda: mm.fit_bspline_contours(cs, s, 3, engine=eng), 7)
                _, reports = mm.fit_bspline_contours(cs, s, 3, engine=eng)
                hist = {}
                for r in reports:
                    hist[r.status] = hist.get(r.status, 0) + 1
                case = {"input": name, "smoothing": s, "degree": 3, "contours": len(cs), "gpu_batch_ms_median": med,
                        "gpu_batch_ms_min": best, "statuses": hist}
                sample = cs[:: max(1, len(cs) // 8)][:8]
                t0 = time.perf_counter()
                for c in sample:
                    B.fit_closed(c, s, 3)
                case["checker_ms_per_contour"] = (time.perf_counter() - t0) * 1e3 / len(sample)
                case["checker_ms_whole_input_extrapolated"] = case["checker_ms_per_contour"] * len(cs)
                if splprep is not None:
                    def loop():
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            for c in cs:
                                tck, _ = splprep([c[:, 0], c[:, 1], c[:, 2]], s=s, k=3, per=True)
                                splev(np.linspace(0, 1, c.shape[0], endpoint=False), tck)
                    case["scipy_loop_ms_median"], case["scipy_loop_ms_min"] = median_ms(loop, 3)
                res["cases"].append(case)
                print(json.dumps(case))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_bspline.json"), "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
