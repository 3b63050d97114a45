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

`python tests/make_golden.py level_plans` rewrites tests/golden/level_plans.json from ITSELF: every case's stored inputs go
through mm_level_plan_probe (the search engine's level planner, no device) and the plan is written back in the file's
format.  The file was recorded from the engine's staging code before the planner was cut out of it, so a run that changes
a byte of it shows a planning decision that moved (tests/test_level_plan_golden.py compares case by case).
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


# ---- level plans: the words of mm_level_plan_probe (include/mm_hausdorff.h) and the file that pins them ----
LEVEL_HEADER = ["precision", "P", "W", "W_lb", "A", "T", "max_na", "max_nbp", "max_nt", "use_fast", "use_lb", "lb_stride",
                "lb_runs_cap", "lb_mx_tiles", "kept_nct", "kept_acap", "pair_evals", "lb_pair_evals", "lb_sparse_total",
                "slice_end", "want_costs", "bound_min_candidates", "bound_matrix", "bound_matrix_qt", "bound_matrix_nc",
                "screen_cull", "screen_split", "screen_group"]
LEVEL_LAYOUT = ["pairs", "work", "work_lb", "cos32", "sin32", "cos64", "sin64", "ang64", "sq32", "sq64", "flag", "items",
                "n_items", "lb32", "pick", "items_pick", "items_lb", "klist", "emit", "qlist", "best_cost", "best_idx",
                "n_rescored", "near_cnt", "near_idx", "lvl_in_bytes", "lvl_bytes", "off_best_cost", "res_bytes",
                "off_all_costs", "r_best_idx", "r_n_rescored", "r_near_cnt", "r_near_idx", "emit_rows", "emit_cols"]
LEVEL_GROUP = ["screen", "nct", "multi", "a_cap", "work_begin", "work_count", "candidates", "tiles_full"]
LEVEL_PAIR_WORDS = 22          # PairDesc's 20 fields, trivial, pair_slice_end; ref_main / tgt_main are words 12, 13
LEVEL_OPTS = LEVEL_HEADER[21:]
LEVEL_F64_INPUTS = ["set_rho", "cx", "cy", "tie_tol", "delta_extra"]       # stored as the hex of their little-endian bytes
LEVEL_I32_INPUTS = ["set_len", "set_main", "ref_set", "tgt_set", "flags", "list_of", "slice_begin", "slice_end"]


def _f64_hex(a):
    """f64 values as the hex of their little-endian bytes; a run of one value as {"fill": hex, "n": count}."""
    b = np.ascontiguousarray(a, dtype="<f8").tobytes()
    return {"fill": b[:8].hex(), "n": len(b) // 8} if len(b) > 8 and b == b[:8] * (len(b) // 8) else b.hex()


def _f64_unhex(h):
    if isinstance(h, dict):
        return np.frombuffer(bytes.fromhex(h["fill"]) * h["n"], dtype="<f8").copy()
    return np.frombuffer(bytes.fromhex(h), dtype="<f8").copy()


def _i32_pack(a):
    a = [int(v) for v in a]
    return {"fill": a[0], "n": len(a)} if len(a) > 1 and a == a[:1] * len(a) else a


def _i32_unpack(v):
    return np.full(v["n"], v["fill"], dtype=np.int32) if isinstance(v, dict) else np.ascontiguousarray(v, dtype=np.int32)


def _bits_f64(word):
    return float(np.array([word], dtype=np.int64).view(np.float64)[0])


def level_plan_arrays(words):
    """The seven arrays of mm_level_plan_probe's words (each preceded by its length), as int64 arrays."""
    words = np.asarray(words, dtype=np.int64)
    out, at = [], 0
    for _ in range(7):
        n = int(words[at])
        out.append(words[at + 1:at + 1 + n])
        at += 1 + n
    assert at == len(words), (at, len(words))
    return out


def level_plan_entry(inputs, words):
    """One case of level_plans.json: the inputs as stored, header / layout / groups readably, a sha256 for the rest, and
    what the hashed arrays show of the branches taken: the work items' pads, the pairs' ref_main / tgt_main, the trivial pairs."""
    header, layout, pairs, tables, work, work_lb, groups = level_plan_arrays(words)
    assert len(header) == len(LEVEL_HEADER) and len(layout) == len(LEVEL_LAYOUT) and len(groups) % len(LEVEL_GROUP) == 0
    assert len(pairs) == LEVEL_PAIR_WORDS * int(header[1])
    head = {k: int(v) for k, v in zip(LEVEL_HEADER, header)}
    for k in ("pair_evals", "lb_pair_evals"):
        head[k] = hexf(_bits_f64(head[k]))
    sha = {k: hashlib.sha256(np.ascontiguousarray(a, dtype="<i8").tobytes()).hexdigest()
           for k, a in (("pairs", pairs), ("tables", tables), ("work", work), ("work_lb", work_lb))}
    split = pairs.reshape(-1, LEVEL_PAIR_WORDS)[:, 12:14]
    return {"in": inputs, "header": head, "layout": {k: int(v) for k, v in zip(LEVEL_LAYOUT, layout)},
            "groups": [{k: int(v) for k, v in zip(LEVEL_GROUP, g)} for g in groups.reshape(-1, len(LEVEL_GROUP))],
            "pads": sorted({int(v) for v in work[3::4]}), "mains": sorted({int(v) for v in split.ravel()}),
            "trivial": int(pairs.reshape(-1, LEVEL_PAIR_WORDS)[:, 20].sum()), "sha256": sha}


def level_plan_probe(inputs, lists):
    """mm_level_plan_probe on one case's stored inputs; `lists`: the file's pool of candidate lists (name -> hex)."""
    import ctypes as C
    import multimoda_rs_amd as mm
    L = mm._native.lib()
    f64 = {k: _f64_unhex(inputs[k]) for k in LEVEL_F64_INPUTS}
    i32 = {k: _i32_unpack(inputs[k]) for k in LEVEL_I32_INPUTS}
    pool = [_f64_unhex(lists[name]) for name in inputs["lists"]]
    off = np.zeros(len(pool) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in pool])
    angles = np.concatenate(pool + [np.zeros(1)])

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def call(out, cap, n):
        rc = L.mm_level_plan_probe(
            len(i32["set_len"]), ptr(i32["set_len"]), ptr(f64["set_rho"]), ptr(i32["set_main"]), len(i32["ref_set"]),
            ptr(i32["ref_set"]), ptr(i32["tgt_set"]), ptr(f64["cx"]), ptr(f64["cy"]), ptr(i32["flags"]), ptr(i32["list_of"]),
            len(pool), ptr(off), ptr(angles), ptr(f64["tie_tol"]), ptr(f64["delta_extra"]), ptr(i32["slice_begin"]),
            ptr(i32["slice_end"]), inputs["precision"], inputs["angle_begin"], inputs["angle_end"], inputs["want_costs"],
            *[inputs["opts"][k] for k in LEVEL_OPTS], out, cap, C.byref(n))
        assert rc == 0, L.mm_last_error().decode()

    n = C.c_int64(0)
    call(None, 0, n)
    words = np.zeros(n.value, dtype=np.int64)
    call(ptr(words), len(words), n)
    assert n.value == len(words)
    return words


def dump_level_plans(doc, path):
    with open(path, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


def main_level_plans():
    path = os.path.join(GOLD, "level_plans.json")
    with open(path) as f:
        doc = json.load(f)
    for name, case in doc["cases"].items():
        doc["cases"][name] = level_plan_entry(case["in"], level_plan_probe(case["in"], doc["lists"]))
    dump_level_plans(doc, path)
    print("wrote", path)


if __name__ == "__main__":
    {"prune_plans": main_prune_plans, "level_plans": main_level_plans}.get(" ".join(sys.argv[1:]), main)()
