"""Generate tests/golden/*.json: expected outputs of the CPU oracle (oracle/) on the data
fixtures of the reference's own tests (tests/golden/ivus_rest, ivus_stress, idealized_geometry).

The oracle's behaviour is pinned by the reference's known-answer tests (test_oracle_kat.py);
the reference itself cannot be built here, so these vectors are "oracle-generated, not
reference-verified".  The oracle's INPUT geometries come from tests/refbuild.py, an independent
restatement of the reference's CSV reader and geometry builder -- not from the product's
multimoda_rs_amd.io, so a builder bug cannot cancel out (tests/test_refbuild.py compares the two).
Floats are stored as hex strings (bit-exact).  Run:
    python tests/make_golden.py

`python tests/make_golden.py prune_plans` records tests/golden/prune_plans.json instead: a sha256 of every array the host
plans of the pruned searches return (mm.ccta.nn_plan, surface.tri_plan) -- permutations, items, bounds, info -- on the
inputs of tests/test_nn_plan_host.py and of the plan tests of tests/test_surface_host.py.  It pins order, ties and
every bit of every bound; record it at the commit whose plans are to be kept (tests/test_prune_plan_golden.py compares).
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = [
    # (name, folder, diastole, step, range, bruteforce, sample_size)
    ("ivus_rest_dia_brute_2deg", "ivus_rest", True, 2.0, 90.0, True, 500),
    ("ivus_rest_sys_hier_0p5deg", "ivus_rest", False, 0.5, 90.0, False, 500),
    ("ivus_stress_dia_hier_0p05deg", "ivus_stress", True, 0.05, 45.0, False, 200),
    ("idealized_dia_hier_0p01deg", "idealized_geometry", True, 0.01, 20.0, False, 200),
]


def hexf(x):
    return float(x).hex()


def main():
    from oracle import oracle as orc
    import refbuild                      # independent pure-Python restatement of the reference's reader + builder
    out = {}
    for name, folder, dia, step, rng, brute, ss in CASES:
        og = g = refbuild.oracle_geometry(orc, os.path.join(GOLD, folder), dia, folder)
        logs = orc.align_within_chain(og, step, rng, brute, ss, n_threads=8)
        out[name] = {
            "folder": folder, "diastole": dia, "step_deg": step, "range_deg": rng, "bruteforce": brute,
            "sample_size": ss, "n_frames": g.n_frames,
            "logs": [[int(l[0]), int(l[1])] + [hexf(v) for v in l[2:]] for l in logs],
            "lumen_sum_hex": [hexf(np.sum(og.lumen[:, 0])), hexf(np.sum(og.lumen[:, 1]))],
            "first_points_hex": [[hexf(v) for v in og.frame_lumen(i)[0]] for i in range(g.n_frames)],
        }
        print(name, g.n_frames, "frames; first rot_deg", logs[0][2])
    # between: rest diastole vs systole after their chains
    oa = refbuild.oracle_geometry(orc, os.path.join(GOLD, "ivus_rest"), True, "rest")
    ob = gb = refbuild.oracle_geometry(orc, os.path.join(GOLD, "ivus_rest"), False, "rest")
    orc.align_within_chain(oa, 1.0, 90.0, False, 500, n_threads=8)
    orc.align_within_chain(ob, 1.0, 90.0, False, 500, n_threads=8)
    best = orc.align_between(oa, ob, 90.0, 0.5, 500, n_threads=8)
    out["ivus_rest_between_chain_only"] = {"best_rotation_hex": hexf(best),
                                           "b_first_points_hex": [[hexf(v) for v in ob.frame_lumen(i)[0]]
                                                                  for i in range(gb.n_frames)]}
    with open(os.path.join(GOLD, "oracle_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", os.path.join(GOLD, "oracle_vectors.json"))


def _plan_digest(plan):
    """name -> sha256 of every array of a plan dict (lists of arrays by position), scalars as int64."""
    out = {}
    for key in sorted(plan):
        val = plan[key]
        for k, a in enumerate(val) if isinstance(val, list) else [(None, val)]:
            a = np.ascontiguousarray(a if isinstance(a, np.ndarray) else np.int64(a))
            head = f"{a.dtype.str}{a.shape}".encode()
            out[key if k is None else f"{key}[{k}]"] = hashlib.sha256(head + a.tobytes()).hexdigest()
    return out


def prune_plans():
    """case -> array -> sha256 for the nearest-neighbour and the point-to-triangle host plans."""
    import multimoda_rs_amd as mm
    from multimoda_rs_amd import surface
    from mm_checkers import refine_mesh as R
    from nn_worst_cases import cases, radial
    from test_refine_host import jitter, wound_tube
    from test_surface_host import long_tube
    from test_trim_host import octahedron

    out = {}
    for name, a, b, r2 in cases():
        out["nn/" + name] = _plan_digest(mm.ccta.nn_plan([a, b], [(0, 1), (1, 0), (0, 0)], r2))
    rng = np.random.default_rng(7)                     # the morphed sets of test_work_lists_of_morphed_sets
    for name, a, b, r2 in [c for c in cases() if c[0] in ("grid", "offset1e+06", "duplicates", "nonfinite", "block_max")]:
        unit, has = radial(rng, len(a))
        sets = [b] + [{"xyz": a, "unit": unit, "has": has, "adj": adj} for adj in (-2.0, -0.30000000000000004, 1.3, 2.0)]
        pairs = [p for i in range(1, len(sets)) for p in ((0, i), (i, 0))]
        out["nn_morphed/" + name] = _plan_digest(mm.ccta.nn_plan(sets, pairs, r2, [0] + [1] * (len(sets) - 1)))
    v, f = wound_tube(15, 17)
    v = jitter(v, 17)
    out["tri/two_chunks"] = _plan_digest(surface.tri_plan(mm.sample_mesh_surface((v + [0.1, 0.0, 0.2], f))[0], (v, f)))
    v, f, moved = long_tube()
    out["tri/long_tube"] = _plan_digest(surface.tri_plan(R.refine(moved, f, 0.6)[0], (v, f)))
    v, f = octahedron()
    out["tri/octahedron"] = _plan_digest(surface.tri_plan(np.zeros((3, 3)), (v, f)))
    out["tri/no_faces"] = _plan_digest(surface.tri_plan(np.zeros((3, 3)), (v, np.zeros((0, 3), dtype=np.int64))))
    out["tri/no_queries"] = _plan_digest(surface.tri_plan(np.zeros((0, 3)), (v, f)))
    return out


def main_prune_plans():
    path = os.path.join(GOLD, "prune_plans.json")
    with open(path, "w") as f:
        json.dump(prune_plans(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main_prune_plans() if sys.argv[1:] == ["prune_plans"] else main()
