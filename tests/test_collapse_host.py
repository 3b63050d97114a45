"""Mesh edge collapse without a GPU: the rule as tests/mm_checkers/collapse_edges.py states it -- the closed stars of the
vertices a pass removes are disjoint, a pass with a candidate removes a vertex, survivors keep their bits and their order,
origin and target agree, V - E + F and the open, non-manifold and inconsistent counts stay, closed manifolds stay closed
and manifold, no pinned or border vertex vanishes, no edge grows past max(longest before, max_ratio L), what stays short
after a converged run is what the last pass counted as blocked -- the shapes that collapse nothing, each of the guards on
a shape built for it, masks and bands, the split and the collapse not undoing each other, the public surface, and the
kernels' resources from the compiler's remarks.

The tetrahedron stays whole by the valence guard; the octahedron passes (d) (every valence is 4) and stays whole by the
normal guard.

Measured on the checkers (the figures of DESIGN 4.24; L = the target, share = edges within [4/5 L, 4/3 L], angles = worst /
mean minimum angle in degrees; a remesh round = one split pass, the collapse, the flips, five relaxation iterations onto the
input).  The jittered wound_tube(15, 17) (seed 17) refined at 0.4 (1460 vertices, 2916 faces, 6.30 / 33.64, share 0.164), L =
0.6: collapse_edges alone 31 passes, 1040 collapses (68, 65, 63, 42, 47, 54, 53, 44, 48, 49, 43, 48, 46, 37, 40, 293 in the
last slot), short edges 3657 -> 287, blocked 0 fixed, 965 link, 0 valence, 9897 long, 4040 normal, 1750 quality: 420 vertices,
836 faces, 14.60 / 43.67, share 0.771; remesh 1 iteration 420 / 836, 25.92 / 51.27, 0.784; 3 iterations 386 / 768, 31.67 /
53.07, 0.853; 10 iterations 376 / 748, 26.01 / 53.83, 0.887.  A mesh of mixed resolution (the same tube, the rings below the
middle at half their spacing, refined at 0.5: 580 vertices, 1156 faces, 9.66 / 33.44, share 0.545), L = 0.4: collapse_edges
alone 7 passes, 105 collapses (31, 25, 22, 17, 9, 1, 0), short edges 334 -> 125, blocked 870 long, 7 normal: 475 / 946, 9.66 /
40.50, 0.600; remesh 1 iteration 761 / 1518, 20.59 / 48.06, 0.685; 3 iterations 680 / 1356, 30.22 / 51.84, 0.827; 10
iterations 664 / 1324, 32.77 / 52.91, 0.873."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from mm_checkers import collapse_edges as CE
from mm_checkers import flip_edges as FE
from mm_checkers import refine_mesh as R
from mm_checkers import smooth_mesh as SMO
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, messy, directed_edges
from test_flip_host import tube, refined_tube, refined_open_tube
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm

KERNELS = ("k_edge_insert_first", "k_col_valence", "k_col_candidates", "k_col_apply", "k_col_finish")
PATCH_FACES = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5), (0, 5, 1), (1, 5, 6), (1, 6, 7), (1, 7, 2)]


def patch(e=0.2, c=(0.0, 1.0), l1=(-1.0, 0.5), l2=(-1.0, -0.5), d=(0.0, -1.0), r2=(1.0, -0.5), r1=(1.0, 0.5)):
    """A flat disk around the short edge a - b (vertices 0 and 1 at (-e, 0) and (e, 0)): a fan at a over c, l1, l2, d and
    a fan at b over d, r2, r1, c.  The six outer vertices are border vertices; a and b are removable."""
    p = [(-e, 0.0), (e, 0.0), c, l1, l2, d, r2, r1]
    return np.array([(x, y, 0.0) for x, y in p]), np.array(PATCH_FACES, dtype=np.int64)


def link_shape():
    """The patch with a vertex t in the face (a, b, c): a and b share t beside c and d, so the link condition fails.  The
    edges at t are not short."""
    v, f = patch(c=(0.0, 1.7))
    v = np.concatenate([v, [[0.0, 0.85, 0.0]]])
    f = np.array([(0, 1, 8), (1, 2, 8), (2, 0, 8)] + PATCH_FACES[1:], dtype=np.int64)
    return v, f


def long_shape():
    """Either direction would make an edge to a far ring vertex, longer than 4/3."""
    return patch(l1=(-1.6, 0.5), l2=(-1.6, -0.5), r1=(1.6, 0.5), r2=(1.6, -0.5))


def fold_shape():
    """b lies beyond the ring edge l1 - l2 of a: a -> b folds the faces at it over.  b is pinned (PINNED_B)."""
    return patch(l1=(0.0, 0.5), l2=(0.0, -0.5))


def needle_shape():
    """A narrow face (a, l1, l2) with two short sides: a -> l1 (a -> l2) would stretch the fan at a into needles over the
    whole patch, below a quarter of the worst quality it has.  b is pinned (PINNED_B)."""
    return patch(e=0.35, l1=(-0.6, 0.1), l2=(-0.6, -0.1))


PINNED_B = np.arange(8) == 1
# name: (shape, target, mask)
SHAPES = {"tetrahedron": (tetrahedron, 100.0, None), "octahedron": (octahedron, 100.0, None), "tube": (tube, 1.0, None),
          "refined_tube": (refined_tube, 0.6, None), "refined_open_tube": (refined_open_tube, 0.6, None),
          "messy": (messy, 5.0, None), "patch": (patch, 1.0, None), "link": (link_shape, 1.0, None),
          "long": (long_shape, 1.0, None), "fold": (fold_shape, 1.0, PINNED_B), "needle": (needle_shape, 1.0, PINNED_B)}
CLOSED = ("tetrahedron", "octahedron", "tube", "refined_tube")
MANIFOLD = tuple(k for k in SHAPES if k != "messy")


@functools.lru_cache(maxsize=None)
def collapsed(name, max_passes=50):
    fn, target, mask = SHAPES[name]
    v, f = fn()
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)
    return (v, f) + CE.collapse(v, f, target, mask=mask, max_passes=max_passes, trace=True)


def longest_edge_sq(v, f):
    return max((x for x in R.edge_lengths(v, f)[1].tolist()), default=0.0)


def euler(v_count, f):
    info = FE.valence(f, v_count)[2]
    return v_count - info["n_edges"] + len(f), info


# ---- the rule, on the checker ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_checker_invariants(name):
    v, f, ov, of, origin, target, rep, passes = collapsed(name)
    nv, nf = len(v), len(f)
    L, mask = SHAPES[name][1], SHAPES[name][2]
    assert rep["n_vertices"] == nv and rep["n_faces"] == nf and rep["passes_run"] == len(passes) <= 50
    assert (rep["n_vertices_out"], rep["n_faces_out"]) == (len(ov), len(of)) == (nv - rep["n_collapses"], nf - 2 * rep["n_collapses"])
    border0 = FE.valence(f, nv)[1]
    to = list(range(nv))
    cur, alive = [tuple(t) for t in f.tolist()], [True] * nf
    for k, p in enumerate(passes):
        stars = [{e["r"]} | set(e["ring"]) for e in p["collapsed"]]
        assert sum(len(s) for s in stars) == len(set().union(*stars)) if stars else True       # pairwise disjoint
        assert bool(p["collapsed"]) == bool(p["candidates"])              # the largest priority always collapses
        assert len({e["prio"] for e in p["candidates"]}) == len(p["candidates"]) and all(e["prio"] for e in p["candidates"])
        assert len(p["short"]) == len(p["candidates"]) + sum(p[b] for b in CE.BLOCKS)
        for e in p["collapsed"]:
            assert not (mask is not None and mask[e["r"]]) and not border0[e["r"]] and to[e["r"]] == e["r"]
            to[e["r"]] = e["k"]
        new, alive2 = CE.rewrite(cur, alive, p["collapsed"])
        touched = {i for e in p["collapsed"] for i in e["faces"]}
        assert all(new[i] == cur[i] and alive2[i] == alive[i] for i in range(nf) if i not in touched)
        cur, alive = new, alive2
        assert rep["collapses_per_pass"][min(k, 15)] >= len(p["collapsed"])
    if rep["converged"]:
        assert not passes[-1]["candidates"]
        # what stays short is what the last pass counted as blocked
        last = passes[-1]
        assert rep["n_short_after"] == len(last["short"]) == sum(last[b] for b in CE.BLOCKS)
        thr = CE.thresholds(L)[0]
        e_out, l_out = R.edge_lengths(ov, of)
        short_out = {tuple(sorted(origin[list(e)].tolist())) for e, x in zip(e_out.tolist(), l_out.tolist()) if x < thr}
        assert short_out == set(last["short"])
    # survivors: their bits, their order; origin and target
    assert np.all(np.diff(origin) > 0) and same_bits(ov, v[origin]) and np.array_equal(target[origin], np.arange(len(ov)))
    root = np.arange(nv)
    for x in range(nv):
        while to[root[x]] != root[x]:
            root[x] = to[root[x]]
    assert np.array_equal(origin[target], root)
    live = np.array([t for t, a in zip(cur, alive) if a], dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(origin[of], live)                               # the faces in order, through the compaction
    gone = np.setdiff1d(np.arange(nv), origin)
    assert not border0[gone].any() and (mask is None or not np.asarray(mask)[gone].any())
    assert rep["n_collapses"] == len(gone) == sum(rep["collapses_per_pass"])
    if name in MANIFOLD:
        chi0, b = euler(nv, f)
        chi1, a = euler(len(ov), of)
        assert chi0 == chi1
        for key in ("n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges"):
            assert a[key] == b[key] == rep[key], key
        assert rep["n_edges"] == b["n_edges"]
    if name in CLOSED:
        d = directed_edges(of)
        assert len(set(d)) == len(d) == 3 * len(of) and set(d) == {(y, x) for x, y in d}
        assert len({tuple(sorted(t)) for t in of.tolist()}) == len(of)
    if len(of):
        assert longest_edge_sq(ov, of) <= max(longest_edge_sq(v, f), CE.thresholds(L)[1])
    want = CE.predict_report(nv, nf, len(ov), len(of), rep["passes_run"], rep["converged"], mask is not None)
    assert {k: rep[k] for k in want} == want
    print(name, rep["passes_run"], rep["collapses_per_pass"], rep["n_short_before"], rep["n_short_after"],
          [rep[k] for k in CE.BLOCKS])


def test_small_solids_stay_whole():
    v, f, ov, of, origin, target, rep, _ = collapsed("tetrahedron")
    assert rep["n_collapses"] == 0 and rep["blocked_valence"] == 6 == rep["n_short_before"] and np.array_equal(of, f)
    v, f, ov, of, origin, target, rep, _ = collapsed("octahedron")
    assert rep["n_collapses"] == 0 and rep["n_short_before"] == 12 and rep["blocked_valence"] == 0 and np.array_equal(of, f)
    assert np.array_equal(origin, np.arange(6)) and np.array_equal(target, np.arange(6)) and same_bits(ov, v)


def test_the_refined_tube_takes_dozens_of_passes_and_chains():
    v, f, ov, of, origin, target, rep, passes = collapsed("refined_tube")
    assert (len(v), len(f)) == (1460, 2916) and rep["converged"] == 1 and rep["passes_run"] >= 24
    assert rep["n_collapses"] > 500 and rep["n_short_after"] < rep["n_short_before"] // 4
    removed = {e["r"] for p in passes for e in p["collapsed"]}
    assert any(e["k"] in removed for p in passes for e in p["collapsed"])  # a kept end that a later pass removes: a chain
    assert abs(rep["volume_after"] - rep["volume_before"]) < 0.05 * abs(rep["volume_before"])


def test_each_guard_on_its_shape():
    rep, passes = collapsed("patch")[6:]
    assert rep["n_collapses"] == 1 and sum(rep[b] for b in CE.BLOCKS) == 0 and passes[0]["collapsed"][0]["r"] == 1   # a tie: r = hi
    rep, passes = collapsed("link")[6:]
    assert passes[0]["reason"] == {(0, 1): "blocked_link"} and rep["n_collapses"] == 0
    rep, passes = collapsed("long")[6:]
    assert passes[0]["reason"] == {(0, 1): "blocked_long"} and rep["n_collapses"] == 0
    v, f = long_shape()
    assert CE.collapse(v, f, 1.0, max_ratio=2.0)[4]["n_collapses"] == 1   # the same edge with the bound out of the way
    rep, passes = collapsed("fold")[6:]
    assert passes[0]["reason"][(0, 1)] == "blocked_normal" and rep["n_collapses"] == 0
    rep, passes = collapsed("needle")[6:]
    assert passes[0]["reason"][(0, 3)] == passes[0]["reason"][(0, 4)] == "blocked_quality"
    v, f = needle_shape()
    free = CE.collapse(v, f, 1.0, mask=PINNED_B, quality_keep=0.0, trace=True)[5][0]
    assert "blocked_quality" not in free["reason"].values() and {(e["lo"], e["hi"]) for e in free["candidates"]} >= {(0, 3), (0, 4)}
    rep = collapsed("refined_tube")[6]
    assert all(rep[b] > 0 for b in ("blocked_link", "blocked_long", "blocked_normal", "blocked_quality"))
    assert collapsed("refined_open_tube")[6]["blocked_fixed"] > 0 and collapsed("messy")[6]["blocked_fixed"] == 9


def test_borders_masks_and_bands():
    v, f, ov, of, origin, target, rep, _ = collapsed("refined_open_tube")
    assert rep["n_open_edges"] > 0 and rep["n_collapses"] > 0
    border = FE.valence(f, len(v))[1]
    assert np.isin(np.flatnonzero(border), origin).all() and FE.valence(of, len(ov))[1].sum() == border.sum()
    v, f = refined_tube()
    mask = np.zeros(len(v), dtype=bool)
    mask[::3] = True
    ov, of, origin, target, rep = CE.collapse(v, f, 0.6, mask=mask, max_passes=3)
    assert rep["n_collapses"] > 0 and np.isin(np.flatnonzero(mask), origin).all()
    assert rep["bytes_uploaded"] == 25 * len(v) + 12 * len(f)
    ring = SMO.rings(f, len(v), [700], 3)[0]
    ov, of, origin, target, rep = CE.collapse(v, f, 0.6, mask=ring < 0, max_passes=3)
    gone = np.setdiff1d(np.arange(len(v)), origin)
    assert len(gone) > 0 and (ring[gone] >= 0).all()


def test_passes_and_an_empty_mesh():
    v, f = refined_tube()
    full = collapsed("refined_tube")[6]
    ov, of, origin, target, rep = CE.collapse(v, f, 0.6, max_passes=0)
    assert np.array_equal(of, f) and same_bits(ov, v) and rep["passes_run"] == 0 and rep["converged"] == 0
    assert rep["n_short_before"] == rep["n_short_after"] == full["n_short_before"] and rep["n_edges"] == 4374
    assert rep["n_launches"] == 2 + 9 + 2 * SMO.volume_launches(len(f))
    ov, of, origin, target, rep = CE.collapse(v, f, 0.6, max_passes=1)
    assert rep["passes_run"] == 1 and rep["converged"] == 0 and rep["n_collapses"] == full["collapses_per_pass"][0]
    assert rep["n_launches"] == 10 + 2 + 9 + SMO.volume_launches(len(f)) + SMO.volume_launches(len(of))
    assert rep["bytes_downloaded"] == 28 * len(ov) + 12 * len(of) + 4 * len(v) + 128
    ov, of, origin, target, rep = CE.collapse(v, np.zeros((0, 3), dtype=np.int64), 0.6)
    assert rep["n_launches"] == 0 and rep["bytes_uploaded"] == 0 and same_bits(ov, v) and np.array_equal(origin, np.arange(len(v)))


def test_the_split_and_the_collapse_do_not_undo_each_other():
    v, f = refined_tube()
    L = 0.6
    rv, rf = R.refine(v, f, L)[:2]                                        # no edge longer than 4/3 L
    ov, of, origin, target, rep = CE.collapse(rv, rf, L)
    assert rep["n_collapses"] > 0 and rep["converged"] == 1
    assert longest_edge_sq(ov, of) <= R.threshold_sq(L)                   # nothing the split would cut again
    again = R.refine(ov, of, L)
    assert len(again[0]) == len(ov) and np.array_equal(again[1], of)
    # a second call on the converged result collapses nothing
    ov2, of2, origin2, target2, rep2 = CE.collapse(ov, of, L)
    assert rep2["n_collapses"] == 0 and rep2["passes_run"] == 1 and rep2["converged"] == 1
    assert np.array_equal(of2, of) and same_bits(ov2, ov) and rep2["n_short_before"] == rep["n_short_after"]


def test_the_float_arithmetic_is_the_other_checkers():
    r = np.random.default_rng(3)
    for scale in (1.0, 1e-160, 1e160):
        p = (r.uniform(-3, 3, (40, 3)) * scale)
        pl = [tuple(x) for x in p.tolist()]
        for i in range(0, 36, 3):
            with np.errstate(all="ignore"):
                n = FE.cross(FE.sub(p[i + 1], p[i]), FE.sub(p[i + 2], p[i]))
                want = (R.len_sq(p[i], p[i + 1]), FE.dot(n, n), FE.quality(p, i, i + 1, i + 2, n))
            m = CE.cross(CE.sub(pl[i + 1], pl[i]), CE.sub(pl[i + 2], pl[i]))
            got = (CE.len_sq(pl[i], pl[i + 1]), CE.dot(m, m), CE.quality(pl, i, i + 1, i + 2, m))
            assert all(same_bits(np.float64(a), np.float64(b)) for a, b in zip(got, want)) and same_bits(np.array(m), np.array(n))


# ---- public surface ------------------------------------------------------------------------------------------------------

def test_public_names_defaults_and_report_size():
    for name in ("collapse_edges", "isotropic_remesh"):
        assert name in mm.__all__ and callable(getattr(mm, name))
    p = inspect.signature(mm.collapse_edges).parameters
    assert list(p) == ["mesh", "target_edge_length_mm", "min_ratio", "max_ratio", "crease_deg", "quality_keep", "passes", "pinned",
                       "band", "engine"]
    assert p["target_edge_length_mm"].default is None and p["min_ratio"].default == 4 / 5 and p["max_ratio"].default == 4 / 3
    assert p["crease_deg"].default == 30.0 and p["quality_keep"].default == 0.5 and p["passes"].default == 50
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    p = inspect.signature(mm.isotropic_remesh).parameters
    assert list(p) == ["mesh", "target_edge_length_mm", "iterations", "reference", "pinned", "band", "crease_deg", "quality_keep",
                       "relax", "engine"]
    assert p["iterations"].default == 10 and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    for fn in (mm.stitch, mm.stitch_conditioned):
        assert inspect.signature(fn).parameters["collapse"].default is False
    assert C.sizeof(mm._native.MMCollapseReport) == 448                   # 54 integers, 2 doubles
    scalars = [n for n, t in mm._native.MMCollapseReport._fields_ if n not in ("collapses_per_pass", "candidates_per_pass")]
    assert scalars == list(mm.ccta.COLLAPSE_REPORT_KEYS)
    header = open(os.path.join(ROOT, "include", "mm_ccta.h")).read()
    assert "mm_collapse_report;" in header and "/* 448 bytes */" in header and "#define MM_COLLAPSE_PASS_SLOTS 16" in header
    assert "int     mm_mesh_collapse_edges(" in header and "mm_mesh_collapse_edges" in mm._native.EXPORTS_CCTA
    assert hasattr(mm._native.lib(), "mm_mesh_collapse_edges")
    with pytest.raises(NotImplementedError, match="isotropic_remesh"):
        mm.postprocess_stitched_mesh(octahedron(), postprocessing=True, remesh_iterations=3)
    assert "isotropic_remesh" in mm.postprocess_stitched_mesh.__doc__


def test_collapse_edges_rejects_bad_arguments_before_the_device():
    mesh = octahedron()
    with pytest.raises(ValueError, match="out of range"):
        mm.collapse_edges((mesh[0], [[0, 1, 6]]), 1.0)
    with pytest.raises(ValueError, match="negative"):
        mm.collapse_edges(mesh, 1.0, passes=-1)
    for bad in (-1.0, 91.0, float("nan")):
        with pytest.raises(ValueError, match="crease_deg"):
            mm.collapse_edges(mesh, 1.0, crease_deg=bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="quality_keep"):
            mm.collapse_edges(mesh, 1.0, quality_keep=bad)
    for bad in (0.0, 1.1, float("nan")):
        with pytest.raises(ValueError, match="min_ratio"):
            mm.collapse_edges(mesh, 1.0, min_ratio=bad)
    for bad in (0.9, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_ratio"):
            mm.collapse_edges(mesh, 1.0, max_ratio=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="target_edge_length_mm"):
            mm.collapse_edges(mesh, bad)
    with pytest.raises(ValueError, match="one entry per vertex"):
        mm.collapse_edges(mesh, 1.0, pinned=np.zeros(5, dtype=bool))
    with pytest.raises(ValueError, match="non-finite"):
        mm.collapse_edges((np.full((6, 3), np.nan), mesh[1]), 1.0)
    with pytest.raises(ValueError, match="negative"):
        mm.isotropic_remesh(mesh, 1.0, iterations=-1)


# ---- the kernels' resources -------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_collapse_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_collapse_kernels.hip" in b.SOURCES and "mm_collapse.cpp" in b.SOURCES and "-ffp-contract=off" in b.FLAGS
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_collapse_kernels.hip")
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
