"""CCTA mesh closing without a device: the public names, the host walk over the rim (mm_hole_loops) against the checker
(tests/mm_checkers/close_mesh.py) and against hand-written answers, the checker's own smoothing on small cases, and the
inputs the GPU tests use for the "no open edge is left" property (so that it is not vacuous there)."""
import numpy as np
import pytest

from mm_checkers import close_mesh as CM
from test_trim_host import octahedron, capped_tube

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta


def open_box():
    """The unit box without its two top faces (the reference's test_adds_faces_to_open_mesh, as data)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=float)
    f = np.array([[0, 2, 1], [0, 3, 2], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4],
                  [3, 4, 7]])
    return v, f


def two_bodies():
    """An open box and, shifted, a capped tube without its bottom cap."""
    bv, bf = open_box()
    tv, tf = capped_tube(8, 4)
    tf = tf[:-16].tolist() + tf[-8:].tolist()
    return np.concatenate([bv, tv + [5.0, 0, 0]]), np.concatenate([bf, np.array(tf) + len(bv)])


def pinched():
    """Two square holes of a sheet that share the vertex 12 (a 5 x 5 grid without the quads (1,1) and (2,2))."""
    n = 5
    v = np.array([[i, j, 0.0] for j in range(n) for i in range(n)])
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            if (i, j) in ((1, 1), (2, 2)):
                continue
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            f += [[a, b, c], [a, c, d]]
    return v, np.array(f)


def host_walk(v, f):
    he = CM.open_half_edges(f)
    loops, centroids, info = ccta.hole_loops(he, v)
    want = CM.hole_loops(he)
    assert [r.tolist() for r in loops] == want[0]
    assert (info["n_irregular_components"], info["n_irregular_edges"], info["n_short_loops"]) == want[1:]
    for c, loop in zip(centroids, want[0]):
        assert np.array_equal(c.view(np.uint64), np.array(CM.centroid(v, loop)).view(np.uint64))
    # the walk does not depend on the order of the list
    r = np.random.default_rng(len(he))
    again = ccta.hole_loops([he[i] for i in r.permutation(len(he))], v)
    assert [x.tolist() for x in again[0]] == want[0] and again[2] == info
    return loops, centroids, info


def test_public_names():
    for name in ("manual_hole_fill", "fill_holes", "create_wall_mesh", "smooth_mesh_labels"):
        assert callable(getattr(mm, name)) and name in mm.__all__
    for sym in ("mm_hole_loops", "mm_fill_holes", "mm_smooth_labels_faces", "mm_smooth_labels_csr"):
        assert sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)


def test_box_one_loop_of_four():
    v, f = open_box()
    loops, centroids, info = host_walk(v, f)
    assert [r.tolist() for r in loops] == [[4, 7, 6, 5]]
    assert centroids.tolist() == [[0.5, 0.5, 1.0]]
    assert info == {"n_irregular_components": 0, "n_irregular_edges": 0, "n_short_loops": 0}
    wv, wf, rep = CM.fill_holes(v, f)
    assert len(f) == 10 and len(wf) == 14 and rep["n_loops_filled"] == 1 and rep["n_fan_faces"] == 4
    assert wv[8].tolist() == [0.5, 0.5, 1.0] and rep["watertight"] and rep["inverted"] == 0 and rep["volume"] == 1.0
    assert wf[10:].tolist() == [[7, 4, 8], [6, 7, 8], [5, 6, 8], [4, 5, 8]]


def test_two_loops_in_order_of_their_smallest_vertex():
    v, f = capped_tube(6, 3)
    f = f[:-12]                                                       # both caps off
    loops, _, info = host_walk(v, f)
    assert [sorted(r.tolist()) for r in loops] == [list(range(0, 6)), list(range(12, 18))]
    assert loops[0][0] == 0 and loops[1][0] == 12 and info["n_irregular_components"] == 0
    _, wf, rep = CM.fill_holes(v, f)
    assert rep["n_loops_filled"] == 2 and rep["watertight"] and len(wf) == len(f) + 12


def test_pinch_vertex_leaves_both_holes():
    v, f = pinched()
    loops, _, info = host_walk(v, f)
    # the outer rim of the sheet is a regular loop of 16; the two holes meet in vertex 12: one component of 8 edges
    assert [len(r) for r in loops] == [16] and loops[0][0] == 0
    assert info == {"n_irregular_components": 1, "n_irregular_edges": 8, "n_short_loops": 0}
    _, _, rep = CM.fill_holes(v, f, fix_normals=False)
    assert rep["n_open_edges"] == 8 and rep["n_open_edges_before"] == 24 and not rep["watertight"]


def test_reversed_face_on_the_rim_is_irregular():
    v, f = open_box()
    g = f.copy()
    g[3] = g[3][::-1]                                                 # (0, 5, 4) owns the rim edge 5 -> 4
    loops, _, info = host_walk(v, g)
    assert loops == [] and info["n_irregular_components"] == 1 and info["n_irregular_edges"] == 4
    _, wf, rep = CM.fill_holes(v, g, fix_normals=False)
    assert len(wf) == 10 and rep["n_irregular_edges"] == 4
    _, wf, rep = CM.fill_holes(v, g, fix_normals=True)                # the winding stage mends it first
    assert len(wf) == 14 and rep["n_flipped_faces"] == 1 and rep["watertight"]


def test_closed_mesh_has_no_loops():
    v, f = octahedron()
    assert CM.open_half_edges(f) == []
    loops, centroids, info = ccta.hole_loops([], v)
    assert loops == [] and centroids.shape == (0, 3) and info["n_irregular_components"] == 0
    wv, wf, rep = CM.fill_holes(v, f)
    assert len(wv) == len(v) and np.array_equal(wf, f) and rep["n_loops_filled"] == 0 and rep["watertight"]


def test_short_loop_and_bad_index():
    loops, _, info = ccta.hole_loops([(3, 3), (0, 1), (1, 0)], np.zeros((4, 3)))
    assert loops == [] and info == {"n_irregular_components": 0, "n_irregular_edges": 0, "n_short_loops": 2}
    with pytest.raises(ValueError, match="out of range"):
        ccta.hole_loops([(0, 4)], np.zeros((4, 3)))


def test_property_inputs_are_regular():
    """The GPU tests assert 'no open edge is left' wherever the checker finds no irregular component and no non-manifold
    edge: the box, the tubes, the two bodies and the take-off sub-mesh are of that kind."""
    tv, tf = capped_tube(12, 6)
    v, f, *_ = mm.synth.synthetic_takeoff_mesh()
    na = 96 * 61
    sub = f[(f < na).all(axis=1)]                                     # the aortic cylinder: two rims, two ostia
    for vv, ff in (open_box(), (tv, tf[:-12]), (tv, tf[:-24]), two_bodies(), (v[:na], sub)):
        _, wf, rep = CM.fill_holes(vv, ff)
        assert rep["n_loops_filled"] >= 1 and rep["n_irregular_components"] == 0 and rep["n_nonmanifold_edges"] == 0
        assert rep["n_open_edges"] == 0 and rep["watertight"]


# ---- the checker's smoothing ----------------------------------------------------------------------------------------------

def test_smoothing_docstring_case():
    rows = CM.adjacency_of_faces([[0, 1, 2], [1, 2, 3]], 4)
    assert rows[1] == {0, 2, 3}
    out, info = CM.smooth_labels([0, 1, 0, 0], rows, 3)
    assert out.tolist() == [0, 0, 0, 0] and out.dtype == np.uint8
    assert info == {"iterations_run": 2, "n_flips": 1, "n_flips_last": 0}


def test_smoothing_isolated_vertex_and_repeated_corner():
    rows = CM.adjacency_of_faces([[0, 1, 2]], 4)
    assert rows[3] == set()
    assert CM.smooth_labels([5, 5, 5, 9], rows, 4)[0].tolist() == [5, 5, 5, 9]
    rows = CM.adjacency_of_faces([[0, 0, 1]], 2)                      # 0 is its own neighbour: its vote is never unanimous
    assert rows[0] == {0, 1} and rows[1] == {0}
    assert CM.smooth_labels([1, 2], rows, 1)[0].tolist() == [1, 1]


def test_smoothing_two_vertex_swap_through_rows():
    rows = [[1], [0]]
    for it in range(6):
        out, info = CM.smooth_labels([3, 7], rows, it)
        assert out.tolist() == ([7, 3] if it % 2 else [3, 7])
        assert info["iterations_run"] == it and info["n_flips"] == 2 * it


def test_wall_mesh_needs_frames_or_a_scaling():
    with pytest.raises(ValueError, match="Either provide frames or aortic scaling"):
        mm.create_wall_mesh(None, None, None, None, {}, aortic_scaling=None)
