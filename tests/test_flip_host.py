"""Mesh edge flips without a GPU: the rule as tests/mm_checkers/flip_edges.py states it -- nv, nf and the untouched
faces stay, closed manifolds stay closed and manifold, every pass lowers the deviation by exactly the sum of its gains,
the flips of a pass share no vertex, the passes end -- the shapes that flip nothing, the serialisation at a cap centre,
each of the four guards, masks and bands, the quality in front of the relaxation, the public surface, and the kernels'
resources from the compiler's remarks.

Measured on the jittered wound_tube(15, 17) (seed 17) refined at 0.4 (1460 vertices, 2916 faces): 628 flips in 14 passes
(81, 89, 104, 97, 101, 74, 39, 25, 11, 4, 1, 1, 1, 0), the deviation 5656 -> 890; blocked over the passes: 0 existing,
334 normal, 1335 crease, 3197 quality.  Minimum angle, worst / mean: refined 6.30 / 33.64, relax only 14.19 / 35.91,
flip then relax 16.05 / 38.59, a second round 19.72 / 39.71 degrees."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from mm_checkers import flip_edges as FE
from mm_checkers import refine_mesh as R
from mm_checkers import relax_mesh as RX
from mm_checkers import smooth_mesh as SMO
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import jitter, wound_tube, open_tube, messy, directed_edges
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm

KERNELS = ("k_edge_insert_first", "k_flip_valence", "k_flip_deviation", "k_flip_candidates", "k_flip_apply")


def tube():
    return wound_tube(15, 17)


def jittered_tube():
    v, f = wound_tube(15, 17)
    return jitter(v, 17), f


@functools.lru_cache(maxsize=None)
def refined_tube():
    v, f = jittered_tube()
    return R.refine(v, f, 0.4)[:2]


@functools.lru_cache(maxsize=None)
def refined_open_tube():
    v, f = open_tube()
    return R.refine(jitter(v, 17), f, 0.4)[:2]


def existing_edge_shape(k=7):
    """A closed surface on which the flip of a - b would make the edge c - d a second time: a tetrahedron a, b, c, d --
    the faces (a, b, c) and (b, a, d), with c - d on the other two -- whose faces (a, c, d) and (b, d, c) are cut by a
    path of k vertices from c to d each: a fan at a (at b) above the path, a fan at a new vertex below it, which keeps
    c - d.  a and b get valence 3 + k, c and d 7: with k = 7 the gain of a - b is 2 (4 + 4 - 1 - 1) - 4 = 8."""
    a, b, c, d = 0, 1, 2, 3
    p, q, m, n = list(range(4, 4 + k)), list(range(4 + k, 4 + 2 * k)), 4 + 2 * k, 5 + 2 * k
    f = [(a, b, c), (b, a, d)]
    for apex, (u, w), path, low in ((a, (c, d), p, m), (b, (d, c), q, n)):
        ring = [u] + path + [w]
        f += [(apex, ring[i], ring[i + 1]) for i in range(k + 1)]                        # above the path
        f += [(low, ring[i + 1], ring[i]) for i in range(k + 1)] + [(low, u, w)]         # below it, down to u - w
    v = np.zeros((6 + 2 * k, 3))
    v[a], v[b], v[c], v[d] = [-1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0.5], [0, -1.0, 0.5]
    t = np.linspace(0.0, 1.0, k + 2)[1:-1]
    for side, path, low in ((-1.0, p, m), (1.0, q, n)):
        y = (1.0 - 2.0 * t) * (1.0 if side < 0 else -1.0)
        v[path] = np.stack([side * 0.8 * (1.0 - y * y) ** 0.5 * 0.9, y, 0.5 + 0.6 * (1.0 - y * y)], axis=1)
        v[low] = [side * 0.2, 0.0, 0.9]
    return v, np.array(f, dtype=np.int64)


SHAPES = {"octahedron": octahedron, "tetrahedron": tetrahedron, "tube": tube, "jittered_tube": jittered_tube,
          "refined_tube": refined_tube, "refined_open_tube": refined_open_tube, "messy": messy,
          "existing_edge": existing_edge_shape}
CLOSED = ("octahedron", "tetrahedron", "tube", "jittered_tube", "refined_tube", "existing_edge")


@functools.lru_cache(maxsize=None)
def flipped(name):
    v, f = SHAPES[name]()
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)
    return (v, f) + FE.flip(v, f, trace=True)


def min_angles(v, f):
    """(worst, mean) over the faces of their smallest angle, degrees."""
    a = v[f]
    out = []
    for k in range(3):
        u, w = a[:, (k + 1) % 3] - a[:, k], a[:, (k + 2) % 3] - a[:, k]
        cos = (u * w).sum(axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(w, axis=1))
        out.append(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))))
    m = np.min(out, axis=0)
    return float(m.min()), float(m.mean())


# ---- the rule, on the checker ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_checker_invariants(name):
    v, f, out, rep, passes = flipped(name)
    nv = len(v)
    assert out.shape == f.shape and rep["n_vertices"] == nv and rep["n_faces"] == len(f)
    assert rep["converged"] == 1 and rep["passes_run"] == len(passes) <= 50 and not passes[-1]["candidates"]
    cur = [tuple(t) for t in f.tolist()]
    dev = rep["deviation_before"]
    for k, p in enumerate(passes):
        assert p["info"]["deviation"] == dev
        touched, faces = set(), set()
        for e in p["flipped"]:
            quad = {e["lo"], e["hi"], e["c"], e["d"]}
            assert len(quad) == 4 and not quad & touched and not {e["fp"], e["fm"]} & faces and e["g"] > 0
            touched |= quad
            faces |= {e["fp"], e["fm"]}
        assert bool(p["flipped"]) == bool(p["candidates"])                # the largest priority always flips
        assert len({e["prio"] for e in p["candidates"]}) == len(p["candidates"]) and all(e["prio"] for e in p["candidates"])
        new = FE.rewrite(cur, p["flipped"])
        assert all(new[i] == cur[i] for i in range(len(cur)) if i not in faces)          # bit-identical and in place
        cur = new
        after = FE.valence(cur, nv)[2]["deviation"]
        assert after == dev - sum(e["g"] for e in p["flipped"]) and (after < dev or not p["flipped"])
        assert rep["flips_per_pass"][min(k, 15)] >= len(p["flipped"])
        dev = after
    assert np.array_equal(out, np.array(cur)) and rep["deviation_after"] == dev
    assert rep["n_flips"] == sum(len(p["flipped"]) for p in passes) == sum(rep["flips_per_pass"])
    # V - E + F, and the edge counts the flips cannot change
    b, a = FE.valence(f, nv)[2], FE.valence(out, nv)[2]
    for key in ("n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges"):
        assert a[key] == b[key] == rep[key], key
    if name in CLOSED:
        d = directed_edges(out)
        assert len(set(d)) == len(d) == 3 * len(f) and set(d) == {(y, x) for x, y in d}
        assert rep["n_open_edges"] == rep["n_nonmanifold_edges"] == rep["n_inconsistent_edges"] == 0
    want = FE.predict_report(nv, len(f), rep["passes_run"], 1)
    assert {k: rep[k] for k in want} == want
    assert rep["n_launches"] == 5 * rep["passes_run"] + 2 * SMO.volume_launches(len(f))
    print(name, rep["passes_run"], rep["flips_per_pass"], rep["deviation_before"], rep["deviation_after"],
          [rep[k] for k in FE.BLOCKS])


@pytest.mark.parametrize("name", ["tetrahedron", "octahedron", "tube"])
def test_regular_shapes_flip_nothing(name):
    v, f, out, rep, passes = flipped(name)
    assert rep["n_flips"] == 0 and rep["passes_run"] == 1 and np.array_equal(out, f)
    assert rep["deviation_before"] == rep["deviation_after"]


def test_the_refined_tube_flips_in_more_than_one_pass():
    v, f, out, rep, passes = flipped("refined_tube")
    assert (len(v), len(f)) == (1460, 2916) and rep["deviation_before"] == 5656
    assert rep["passes_run"] > 2 and rep["n_flips"] > 300 and sum(1 for n in rep["flips_per_pass"] if n) > 1
    assert rep["deviation_after"] < rep["deviation_before"] // 4
    assert abs(rep["volume_after"] - rep["volume_before"]) < 0.01 * abs(rep["volume_before"])


def test_the_cap_centre_serialises():
    v, f, out, rep, passes = flipped("jittered_tube")
    centre = len(v) - 2                                                   # the two cap centres are the last vertices
    deg = FE.valence(f, len(v))[0]
    assert deg[centre] == 15
    at = [k for k in passes[0]["candidates"] if centre in (k["lo"], k["hi"])]
    assert len(at) > 1 and sum(1 for k in passes[0]["flipped"] if centre in (k["lo"], k["hi"])) == 1
    assert rep["passes_run"] > 2


def test_every_guard_blocks_somewhere():
    v, f, out, rep, passes = flipped("refined_tube")
    first = passes[0]
    assert first["blocked_normal"] > 0 and first["blocked_crease"] > 0 and first["blocked_quality"] > 0
    assert first["blocked_existing"] == 0
    v, f, out, rep, passes = flipped("existing_edge")
    assert rep["blocked_existing"] > 0
    assert rep["n_open_edges"] == 0 and rep["n_inconsistent_edges"] == 0
    table = FE.edge_table([tuple(t) for t in f.tolist()])
    assert table[(0, 1)]["n"] == 2 and table[(2, 3)]["n"] == 2            # a - b could flip only onto c - d, which exists
    assert (0, 1) in FE.edge_table([tuple(t) for t in out.tolist()])


def test_open_rims_masks_and_bands():
    v, f, out, rep, passes = flipped("refined_open_tube")
    assert rep["n_open_edges"] > 0 and rep["n_flips"] > 0
    open_before = {k for k, e in FE.edge_table([tuple(t) for t in f.tolist()]).items() if e["n"] == 1}
    open_after = {k for k, e in FE.edge_table([tuple(t) for t in out.tolist()]).items() if e["n"] == 1}
    assert open_before == open_after
    v, f = refined_tube()
    mask = np.zeros(len(v), dtype=bool)
    mask[::3] = True
    out, rep, passes = FE.flip(v, f, mask=mask, trace=True)
    assert rep["n_masked_edges"] > 0 and rep["n_flips"] > 0 and rep["bytes_uploaded"] == 24 * len(v) + 12 * len(f) + len(v)
    for p in passes:
        assert not any(mask[k["lo"]] or mask[k["hi"]] for k in p["candidates"])
    # a band: everything farther than 3 edges from vertex 700 is masked, so only faces inside it change
    ring = SMO.rings(f, len(v), [700], 3)[0]
    out, rep = FE.flip(v, f, mask=ring < 0)
    changed = np.flatnonzero((out != f).any(axis=1))
    assert 0 < len(changed) and (ring[f[changed]] >= 0).any(axis=1).all() and (ring[out[changed]] >= 0).any(axis=1).all()
    assert not (ring[f] < 0).all(axis=1)[changed].any()


def test_passes_and_an_empty_mesh():
    v, f = refined_tube()
    full = flipped("refined_tube")[3]
    out0, rep0 = FE.flip(v, f, max_passes=0)
    assert np.array_equal(out0, f) and rep0["passes_run"] == 0 and rep0["converged"] == 0
    assert rep0["deviation_before"] == rep0["deviation_after"] == 5656 and rep0["n_edges"] == 4374
    assert rep0["n_launches"] == 3 + 2 * SMO.volume_launches(len(f))
    out1, rep1 = FE.flip(v, f, max_passes=1)
    assert rep1["passes_run"] == 1 and rep1["converged"] == 0 and rep1["n_flips"] == full["flips_per_pass"][0]
    assert rep1["n_launches"] == 5 + 3 + 2 * SMO.volume_launches(len(f)) and rep1["deviation_after"] < 5656
    out, rep = FE.flip(v, np.zeros((0, 3), dtype=np.int64))
    assert rep["n_launches"] == 0 and rep["bytes_uploaded"] == 0 and rep["deviation_after"] == 36 * len(v)


def test_flips_in_front_of_the_relaxation_raise_the_minimum_angles():
    v, f, out, rep, _ = flipped("refined_tube")
    plain = min_angles(RX.relax(v, f, iterations=5, lamb=0.5)[0], f)
    both = min_angles(RX.relax(v, out, iterations=5, lamb=0.5)[0], out)
    print(f"refined {min_angles(v, f)}, flips alone {min_angles(v, out)}, relax only {plain}, flip then relax {both}")
    assert both[0] > plain[0] and both[1] > plain[1]


# ---- public surface ------------------------------------------------------------------------------------------------------

def test_public_names_defaults_and_report_size():
    for name in ("mesh_valence", "flip_edges"):
        assert name in mm.__all__ and callable(getattr(mm, name))
    p = inspect.signature(mm.flip_edges).parameters
    assert list(p) == ["mesh", "crease_deg", "quality_keep", "passes", "pinned", "band", "engine"]
    assert p["crease_deg"].default == 30.0 and p["quality_keep"].default == 0.5 and p["passes"].default == 50
    assert p["pinned"].default is None and p["band"].default is None and p["engine"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert list(inspect.signature(mm.mesh_valence).parameters) == ["mesh", "engine"]
    for fn in (mm.stitch, mm.stitch_conditioned):
        assert inspect.signature(fn).parameters["flip"].default is False
    assert C.sizeof(mm._native.MMFlipReport) == 424                       # 51 integers, 2 doubles
    scalars = [n for n, t in mm._native.MMFlipReport._fields_ if n not in ("flips_per_pass", "candidates_per_pass")]
    assert scalars == list(mm.ccta.FLIP_REPORT_KEYS)
    header = open(os.path.join(ROOT, "include", "mm_ccta.h")).read()
    assert "mm_flip_report;" in header and "/* 424 bytes */" in header and "#define MM_FLIP_PASS_SLOTS 16" in header
    for sym in ("mm_mesh_valence", "mm_mesh_flip_edges"):
        assert f"int     {sym}(" in header and sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)
    assert FE.crease_cos(30.0) == np.cos(np.radians(30.0)) or abs(FE.crease_cos(30.0) - np.sqrt(0.75)) < 1e-15


def test_flip_edges_rejects_bad_arguments_before_the_device():
    mesh = octahedron()
    with pytest.raises(ValueError, match="out of range"):
        mm.flip_edges((mesh[0], [[0, 1, 6]]))
    with pytest.raises(ValueError, match="out of range"):
        mm.mesh_valence((mesh[0], [[0, 1, 6]]))
    with pytest.raises(ValueError, match="negative"):
        mm.flip_edges(mesh, passes=-1)
    for bad in (-1.0, 91.0, float("nan")):
        with pytest.raises(ValueError, match="crease_deg"):
            mm.flip_edges(mesh, crease_deg=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="quality_keep"):
            mm.flip_edges(mesh, quality_keep=bad)
    with pytest.raises(ValueError, match="one entry per vertex"):
        mm.flip_edges(mesh, pinned=np.zeros(5, dtype=bool))
    with pytest.raises(ValueError, match="non-finite"):
        mm.flip_edges((np.full((6, 3), np.nan), mesh[1]))


# ---- the kernels' resources -------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_flip_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_flip_kernels.hip" in b.SOURCES and "mm_flip.cpp" in b.SOURCES and "-ffp-contract=off" in b.FLAGS
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_flip_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                 # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        print(name, get("VGPRs"), get(r"Occupancy \[waves/SIMD\]"))
        seen.update(k for k in KERNELS if k in name)
    assert seen == set(KERNELS)
    assert not re.search(r"\bglobal_atomic_\w*_f(16|32|64)\b", text)
    assert not re.search(r"\batomic\w*_(f16|f32|f64)\b", text)
    assert "global_atomic_umax_x2" in text and "v_div_fixup_f64" in text                # 64-bit integer max, a true division
    assert not re.search(r"\basm\b", open(src).read())
