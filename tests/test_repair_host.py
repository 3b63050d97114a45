"""The mesh repair on the host (no GPU): the checker tests/mm_checkers/repair_mesh.py against the invariants of the
rule in include/mm_ccta.h ("mesh repair") -- stage (d) as the literal walk equals the closed form the device computes,
no edge keeps more than two owners, every vertex's corners hang together afterwards, a second run finds nothing --,
the claim the feature exists for (repair, then the hole filling, closes a pinched rim that the hole filling alone leaves
open), the public surface, the argument checks that need no device, and the kernels' resources from the compiler's
remarks.  The shapes are shared with tests/test_gpu_repair.py."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from mm_checkers import close_mesh as CM
from mm_checkers import repair_mesh as RM
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, messy, wound_tube, open_tube
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm

KERNELS = ("k_rep_vertex_insert", "k_rep_vertex_rep", "k_rep_face_classify", "k_rep_face_rep", "k_rep_edge_insert",
           "k_rep_edge_rank", "k_rep_face_remove", "k_rep_hook", "k_rep_vertex_min", "k_rep_open", "k_rep_vertex_keep",
           "k_rep_out_vertices", "k_rep_out_corners")


# ---- shapes -----------------------------------------------------------------------------------------------------------------

def five_on_an_edge(heights=(1.0, 2.0, 3.0, 4.0, 5.0), order=None):
    """Five triangles on the edge 0 - 1, apex k at height heights[k] in its own half plane: q = heights[k]^2."""
    v = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    for k, h in enumerate(heights):
        a = 0.4 + 1.1 * k
        v.append([0.5, h * np.cos(a), h * np.sin(a)])
    f = np.array([[0, 1, 2 + k] if k % 2 == 0 else [1, 0, 2 + k] for k in range(len(heights))])
    return np.array(v), (f if order is None else f[list(order)])


def kept_by_one_edge_removed_by_another():
    """Face 0 = (0, 1, 2) is the smallest of three on 0 - 1 and the largest of three on 1 - 2: it goes, and so does the
    smallest on 1 - 2, which leaves 1 - 2 with one owner."""
    v = np.array([[0.0, 0, 0], [2.0, 0, 0], [2.0, 2.0, 0], [1.0, -3.0, 1.0], [1.0, -4.0, -2.0], [3.0, 1.0, 0.5],
                  [2.5, 1.0, -0.25]])
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5], [1, 2, 6]])
    return v, f


def solids_at_a_vertex(n=2, shuffle=None):
    """n tetrahedra that share vertex 0 and nothing else; `shuffle`: a seed for the face order."""
    tv, tf = tetrahedron()
    v, f = [tv[0]], []
    for k in range(n):
        rot = np.array([[np.cos(2.0 * k), -np.sin(2.0 * k), 0], [np.sin(2.0 * k), np.cos(2.0 * k), 0], [0, 0, 1.0]])
        base = len(v)
        v.extend((tv[0] + (tv[1:] - tv[0]) @ rot.T).tolist())
        index = np.array([0, base, base + 1, base + 2])
        f.extend(index[tf].tolist())
    f = np.array(f)
    if shuffle is not None:
        f = f[np.random.default_rng(shuffle).permutation(len(f))]
    return np.array(v), f


def solids_at_an_edge():
    """Two tetrahedra that share the edge 0 - 1: four owners."""
    v = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.5, 1.0, 0.2], [0.5, 0.8, 1.0], [0.5, -1.5, -0.3], [0.5, -1.0, -1.9]])
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 2, 3], [2, 1, 3], [1, 0, 4], [0, 1, 5], [0, 4, 5], [4, 1, 5]])
    return v, f


def pinched_rim():
    """Two open hexagonal fans whose rims share vertex 1."""
    ang = np.arange(6) * (np.pi / 3.0)
    a = np.stack([np.cos(ang), np.sin(ang), np.zeros(6)], 1) + [-1.0, 0, 0]      # rim of A: vertices 1 .. 6, A[0] = origin
    b = np.stack([-np.cos(ang), np.sin(ang), 0.5 * np.sin(ang)], 1) + [1.0, 0, 0]    # rim of B: B[0] = origin too
    v = np.concatenate([[[-1.0, 0, 0]], a, [[1.0, 0, 0.1]], b[1:]])
    ra = [1, 2, 3, 4, 5, 6]
    rb = [1, 8, 9, 10, 11, 12]
    f = [[0, ra[k], ra[(k + 1) % 6]] for k in range(6)] + [[7, rb[(k + 1) % 6], rb[k]] for k in range(6)]
    return v, np.array(f)


def cone(n, apex, first, shuffle=None):
    faces = np.array([[apex, first + k, first + (k + 1) % n] for k in range(n)])
    return faces if shuffle is None else faces[np.random.default_rng(shuffle).permutation(n)]


def cones(n=5000, second=True):
    """A cone of n faces about vertex 0, shuffled with a fixed seed, and a second one that shares the apex only."""
    ang = np.arange(n) * (2.0 * np.pi / n)
    ring = np.stack([np.cos(ang), np.sin(ang), np.ones(n)], 1)
    v = np.concatenate([[[0.0, 0, 0]], ring] + ([ring * [1.5, 1.5, -1.0]] if second else []))
    f = cone(n, 0, 1, shuffle=11)
    if second:
        f = np.concatenate([f, cone(n, 0, 1 + n)])
    return v, f


def duplicates():
    """messy() with a bit-equal copy of vertex 2 (used by a face), -0.0 against 0.0, a vertex one ulp off, an
    unreferenced copy, a collinear null face and a repeated face rotated and reversed."""
    v, f = messy()
    v = np.concatenate([v, [v[2], [-0.0, -0.0, 0.0], [np.nextafter(2.0, 3.0), 0, 0], v[4], [3.0, 0, 0]]])
    f = np.concatenate([f, [[0, 1, 6], [7, 1, 3], [8, 2, 4], [0, 1, 10], [4, 0, 1], [1, 4, 0], [3, 0, 1]]])
    return v, f


def soup(seed):
    """30 .. 300 faces over 8 .. 40 vertices at integer coordinates: many tied areas, edges with many owners."""
    r = np.random.default_rng(seed)
    nv, nf = int(r.integers(8, 41)), int(r.integers(30, 301))
    return r.integers(-2, 3, (nv, 3)).astype(np.float64), r.integers(0, nv, (nf, 3))


SHAPES = {
    "five_on_an_edge": five_on_an_edge,
    "five_tied": lambda: five_on_an_edge((1.0, 3.0, 2.0, 3.0, 1.0)),
    "five_shuffled": lambda: five_on_an_edge(order=(3, 0, 4, 2, 1)),
    "kept_and_removed": kept_by_one_edge_removed_by_another,
    "two_solids_at_a_vertex": solids_at_a_vertex,
    "three_solids_out_of_order": lambda: solids_at_a_vertex(3, shuffle=5),
    "two_solids_at_an_edge": solids_at_an_edge,
    "pinched_rim": pinched_rim,
    "duplicates": duplicates,
    "messy": messy,
    "cone_257": lambda: cones(257, second=False),
    "soup": lambda: soup(3),
}
CLEAN = {"tetrahedron": tetrahedron, "octahedron": octahedron, "wound_tube": lambda: wound_tube(15, 17), "open_tube": open_tube}


def same_result(a, b):
    return (same_bits(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])) and a[4] == b[4])


# ---- the checker ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_checker_invariants(name):
    v, f = SHAPES[name]()
    walk = RM.repair(v, f)
    assert same_result(walk, RM.repair(v, f, closed_form=True))            # (d): the walk is its closed form
    ov, of, origin, target, rep = walk
    assert same_bits(ov, np.asarray(v, dtype=np.float64)[origin]) and rep["n_vertices"] == len(ov) and rep["n_faces"] == len(of)
    rows = of.tolist()
    alive = [True] * len(rows)
    own = RM.edge_owners(rows, alive)
    assert max((len(o) for o in own.values()), default=0) <= 2 and rep["n_nonmanifold_edges_after"] == 0
    root = RM.corner_components(rows, alive)                               # (e): one component a vertex
    per_vertex = {}
    for c, r in root.items():
        per_vertex.setdefault(rows[c // 3][c % 3], set()).add(r)
    assert all(len(s) == 1 for s in per_vertex.values())
    assert RM.edge_counts(rows, alive) == (rep["n_open_edges_after"], 0)   # (e) changed no edge count
    assert (target[origin[:len(ov) - rep["n_new_vertices"]]] == np.arange(len(ov) - rep["n_new_vertices"])).all()
    again = RM.repair(ov, of)                                              # the mesh is a fixed point
    assert same_bits(again[0], ov) and np.array_equal(again[1], of)
    assert again[4]["n_open_edges_before"] == again[4]["n_open_edges_after"] == rep["n_open_edges_after"]
    assert again[4]["n_faces_removed"] == again[4]["n_nonmanifold_edges_before"] == 0
    assert again[4]["n_degenerate_faces"] == again[4]["n_null_faces"] == again[4]["n_duplicate_faces"] == 0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_a_second_run_finds_nothing(name):
    """repair(repair(x)) == repair(x) bit for bit, with origin = target = the identity and all counts zero on the second
    run.  Stage (e) gives a new vertex its parent's bits, so stage (a) of the second run finds it equal to its parent; the
    rule does not make a weld that the split would only undo (include/mm_ccta.h, stage (e)), which is what lets this hold
    on the shapes with a split too."""
    ov, of = RM.repair(*SHAPES[name]())[:2]
    again = RM.repair(ov, of)
    print(name, {k: again[4][k] for k in RM.COUNT_KEYS})
    assert same_bits(again[0], ov) and np.array_equal(again[1], of)
    assert np.array_equal(again[2], np.arange(len(ov))) and np.array_equal(again[3], np.arange(len(ov)))
    assert all(again[4][k] == 0 for k in RM.COUNT_KEYS if k not in ("n_vertices", "n_faces", "n_open_edges_before",
                                                                      "n_open_edges_after"))


def test_the_walk_equals_the_closed_form_on_random_soups():
    removed = 0
    for seed in range(200):
        v, f = soup(seed)
        walk = RM.repair(v, f)
        assert same_result(walk, RM.repair(v, f, closed_form=True)), seed
        removed += walk[4]["n_faces_removed"]
    assert removed > 2000                                                  # the soups do have edges with many owners


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_clean_meshes_come_back_bit_for_bit(name):
    v, f = CLEAN[name]()
    ov, of, origin, target, rep = RM.repair(v, f)
    assert same_bits(ov, v) and np.array_equal(of, f)
    assert np.array_equal(origin, np.arange(len(v))) and np.array_equal(target, np.arange(len(v)))
    assert all(rep[k] == 0 for k in RM.COUNT_KEYS if k not in ("n_vertices", "n_faces", "n_open_edges_before",
                                                                 "n_open_edges_after"))
    assert rep["n_open_edges_before"] == rep["n_open_edges_after"] == (30 if name == "open_tube" else 0)


def test_the_named_shapes_do_what_the_rule_says():
    _, of, _, _, rep = RM.repair(*five_on_an_edge())
    assert of.tolist() == [[1, 0, 5], [0, 1, 6]] and rep["n_faces_removed"] == 3 and rep["n_nonmanifold_edges_before"] == 1
    _, of, _, _, rep = RM.repair(*five_on_an_edge((1.0, 3.0, 2.0, 3.0, 1.0)))
    assert of.tolist() == [[1, 0, 3], [1, 0, 5]]                          # q tied at 9: both stay; at 1 none does
    tied = RM.repair(*five_on_an_edge((3.0, 3.0, 3.0, 1.0, 1.0)))[1]
    assert tied.tolist() == [[1, 0, 3], [0, 1, 4]]                        # three tied: the two larger indices
    a = {tuple(r) for r in RM.repair(*five_on_an_edge())[1].tolist()}
    b = {tuple(r) for r in RM.repair(*five_on_an_edge(order=(3, 0, 4, 2, 1)))[1].tolist()}
    assert a == b
    _, of, _, _, rep = RM.repair(*kept_by_one_edge_removed_by_another())
    assert of.tolist() == [[1, 0, 3], [0, 1, 4], [2, 7, 5]] and rep["n_faces_removed"] == 2
    assert rep["n_open_edges_after"] == 7 and rep["n_nonmanifold_edges_before"] == 2
    ov, of, origin, _, rep = RM.repair(*solids_at_a_vertex())
    assert rep["n_nonmanifold_vertices"] == 1 and rep["n_new_vertices"] == 1 and origin[-1] == 0 and same_bits(ov[-1], ov[0])
    assert (of[:4] != 7).all() and sorted(set(of[4:].ravel().tolist())) == [4, 5, 6, 7]
    v3, f3 = solids_at_a_vertex(3, shuffle=5)
    ov, of, origin, _, rep = RM.repair(v3, f3)
    assert rep["n_nonmanifold_vertices"] == 1 and rep["n_new_vertices"] == 2 and origin[-2:].tolist() == [0, 0]
    firsts = [min(i for i, row in enumerate(of.tolist()) if x in row) for x in (0, 10, 11)]
    assert firsts == sorted(firsts)                                       # numbered by the smallest corner
    _, _, _, _, rep = RM.repair(*solids_at_an_edge())
    assert rep["n_nonmanifold_edges_before"] == 1 and rep["n_faces_removed"] == 2 and rep["n_open_edges_after"] == 4
    ov, of, origin, target, rep = RM.repair(*duplicates())
    assert rep["n_welded_vertices"] == 3 and target[[6, 7, 9]].tolist() == [2, 0, 4] and target[8] == 8 - 2
    assert rep["n_degenerate_faces"] == 2 and rep["n_null_faces"] == 1 and rep["n_duplicate_faces"] == 6
    assert bits_of(ov[0]) == bits_of(np.zeros(3))                         # the survivor's own bits, not the -0.0's
    assert RM.repair(*duplicates(), drop_unreferenced=True)[4]["n_unreferenced_dropped"] == 2


def test_a_weld_that_the_split_would_undo_is_not_made():
    v, f = RM.repair(*solids_at_a_vertex())[:2]                            # vertex 7 has the bits of vertex 0
    for kw in ({}, {"nonmanifold_vertices": False}):                       # with the split off too: no pinch is made
        ov, of, origin, target, rep = RM.repair(v, f, **kw)
        assert same_bits(ov, v) and np.array_equal(of, f) and origin.tolist() == target.tolist() == list(range(8))
        assert rep["n_welded_vertices"] == rep["n_new_vertices"] == rep["n_nonmanifold_vertices"] == 0
    g = f.copy()
    g[0][g[0] == 0] = 7                                                    # one face of the first solid names the copy:
    ov, of, origin, target, rep = RM.repair(v, g)                          # its corner hangs with vertex 0's, so 7 is welded
    assert rep["n_welded_vertices"] == 1 and target[7] == 0 and np.array_equal(of[0], f[0])
    assert rep["n_new_vertices"] == 1 and origin[-1] == 0 and len(ov) == 8 # and the second solid is split off as before
    ov, of, origin, target, rep = RM.repair(np.concatenate([v, v[:1]]), f) # an unreferenced copy is welded
    assert rep["n_welded_vertices"] == 1 and target[8] == 0 and len(ov) == 8


def bits_of(p):
    return np.asarray(p, dtype=np.float64).view(np.uint64).tolist()


def test_repair_then_close_makes_the_pinched_rim_watertight():
    v, f = pinched_rim()
    alone = CM.fill_holes(v, f, True)[2]
    assert alone["n_irregular_components"] > 0 and not alone["watertight"]
    rv, rf, _, _, rep = RM.repair(v, f)
    assert rep["n_new_vertices"] == 1 and rep["n_nonmanifold_vertices"] == 1
    closed = CM.fill_holes(rv, rf, True)[2]
    assert closed["n_irregular_components"] == 0 and closed["watertight"] and closed["n_loops_filled"] == 2


# ---- public surface ---------------------------------------------------------------------------------------------------------

def test_public_names_defaults_and_report_size():
    for name in ("repair_mesh", "mesh_manifold_report", "fix_and_remesh_stitched_mesh"):
        assert name in mm.__all__ and callable(getattr(mm, name))
    p = inspect.signature(mm.repair_mesh).parameters
    assert list(p) == ["mesh", "duplicate_vertices", "null_faces", "duplicate_faces", "nonmanifold_edges",
                       "nonmanifold_vertices", "drop_unreferenced", "engine"]
    assert [p[k].default for k in list(p)[1:]] == [True, True, True, True, True, False, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert list(inspect.signature(mm.mesh_manifold_report).parameters) == ["mesh", "engine"]
    p = inspect.signature(mm.fix_and_remesh_stitched_mesh).parameters
    assert list(p) == ["mesh", "target_edge_length_mm", "remesh_iterations", "verbose", "pinned", "band", "return_report", "engine"]
    assert [p[k].default for k in list(p)[1:]] == [None, 10, False, None, None, False, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    for fn in (mm.stitch, mm.stitch_conditioned):
        assert inspect.signature(fn).parameters["repair"].default is False
    assert C.sizeof(mm._native.MMRepairReport) == 144
    assert [n for n, _ in mm._native.MMRepairReport._fields_] == list(mm.ccta.REPAIR_REPORT_KEYS)
    assert set(RM.COUNT_KEYS) < set(mm.ccta.REPAIR_REPORT_KEYS)
    assert [name for name, _ in mm.ccta.REPAIR_FLAGS] == list(RM.FLAGS)
    header = open(os.path.join(ROOT, "include", "mm_ccta.h")).read()
    assert "mm_repair_report;" in header and "/* 144 bytes */" in header and "int     mm_mesh_repair(" in header
    assert f"#define MM_REPAIR_LAUNCHES             {RM.LAUNCHES}" in header
    for (name, bit) in mm.ccta.REPAIR_FLAGS:
        macro = {"drop_unreferenced": "MM_REPAIR_DROP_UNREFERENCED"}.get(name, "MM_REPAIR_" + name.upper())
        assert re.search(r"#define " + macro + r"\s+" + str(bit) + r"\n", header), name
    assert "mm_mesh_repair" in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), "mm_mesh_repair")
    for fn in (mm.isotropic_remesh, mm.postprocess_stitched_mesh):
        assert "not part of this project" not in fn.__doc__
    assert "fix_and_remesh_stitched_mesh" in mm.postprocess_stitched_mesh.__doc__
    for word in ("centroid", "maxholesize", "half-edge", "checksurfdist", "welds first"):
        assert word in mm.fix_and_remesh_stitched_mesh.__doc__, word


def test_bad_arguments_raise_before_the_device():
    mesh = octahedron()
    for call in (mm.repair_mesh, mm.mesh_manifold_report, mm.fix_and_remesh_stitched_mesh):
        with pytest.raises(ValueError, match="out of range"):
            call((mesh[0], [[0, 1, 6]]))
        with pytest.raises(ValueError, match="non-finite"):
            call((np.full((6, 3), np.inf), mesh[1]))
    with pytest.raises(ValueError, match="nonmanifold_edges must be True or False"):
        mm.repair_mesh(mesh, nonmanifold_edges=2)
    with pytest.raises(ValueError, match="negative"):
        mm.fix_and_remesh_stitched_mesh(mesh, remesh_iterations=-1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="target_edge_length_mm"):
            mm.fix_and_remesh_stitched_mesh(mesh, target_edge_length_mm=bad)
    with pytest.raises(ValueError, match="one entry per vertex"):
        mm.fix_and_remesh_stitched_mesh(mesh, target_edge_length_mm=1.0, pinned=np.zeros(5, dtype=bool))


# ---- the kernels' resources -------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_repair_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_repair_kernels.hip" in b.SOURCES and "mm_repair.cpp" in b.SOURCES and "-ffp-contract=off" in b.FLAGS
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_repair_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                 # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 8, name
        print(name, get("VGPRs"), get(r"Occupancy \[waves/SIMD\]"))
        seen.update(k for k in KERNELS if k in name)
    assert seen == set(KERNELS)
    assert not re.search(r"\bglobal_atomic_\w*_f(16|32|64)\b", text)
    assert not re.search(r"\batomic\w*_(f16|f32|f64)\b", text)
    assert "global_atomic_umax_x2" in text and not re.search(r"\bv_fmac?_f64\b", text)  # the 64-bit max; nothing fused
    assert not re.search(r"\basm\b", open(src).read())
