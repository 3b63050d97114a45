"""Mesh refinement without a device: the public names, and the checker (tests/mm_checkers/refine_mesh.py) against the
properties the edge split must have -- closed manifold meshes stay closed and manifold with one winding, the Euler
characteristic and (up to rounding) the volume stay, input vertices keep their bits and index, every new vertex is used,
a converged run leaves no edge above the threshold, the children of an open edge are open -- the pass sizes of two
shapes, all four templates, and a messy face list.  The kernels' resources come from the compiler's remarks."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from mm_checkers import refine_mesh as R
from test_trim_host import octahedron, capped_tube
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm

KERNELS = ("k_refine_edge_insert", "k_refine_mark", "k_refine_count", "k_refine_scan_tiles", "k_refine_offsets",
           "k_refine_children")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def jitter(v, seed):
    return v + 0.05 * np.random.default_rng(seed).standard_normal(v.shape)


def wound_tube(n_around, n_rings):
    """capped_tube with its caps, which it winds against the wall, reversed: one winding all over."""
    v, f = capped_tube(n_around, n_rings)
    f = f.copy()
    f[-2 * n_around:] = f[-2 * n_around:, ::-1]
    return v, f


def stretched_tube():
    v, f = wound_tube(12, 3)
    return v * [1.0, 1.0, 4.0], f


def open_tube(n_around=15, n_rings=17):
    v, f = wound_tube(n_around, n_rings)
    return v[:-2], f[:-2 * n_around]                                      # the caps are the last faces and vertices


def messy():
    """An (a, a, b) face, an (a, b, a) face, a repeated face and an edge (0 - 1) with three owners."""
    v = np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 2.0, 0], [1.0, -2.0, 0], [1.0, 0, 2.0], [5.0, 5.0, 5.0]])
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [0, 1, 2], [3, 3, 4], [2, 4, 2]])
    return v, f


SHAPES = {
    "octahedron": (octahedron, 0.3, True),
    "stretched_tube": (stretched_tube, 0.3, True),
    "tube_257": (lambda: wound_tube(15, 17), 0.4, True),
    "jittered_tube": (lambda: (jitter(wound_tube(15, 17)[0], 17), wound_tube(15, 17)[1]), 0.4, True),
    "open_tube": (open_tube, 0.3, False),                                 # its rim edges (0.416) are split too
}


def directed_edges(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return [tuple(x) for x in e.tolist()]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_checker_invariants(name):
    make, L, closed = SHAPES[name]
    v, f = make()
    out_v, out_f, parents, rep = R.refine(v, f, L)
    thr2 = R.threshold_sq(L)
    nv = len(v)
    assert rep["converged"] == 1 and rep["stopped_by_cap"] == 0 and rep["longest_sq_after"] <= thr2 < rep["longest_sq_before"]
    assert rep["n_vertices"] == len(out_v) == nv + len(parents) == nv + sum(rep["splits_per_pass"]) > nv
    t = rep["faces_by_template"]
    assert rep["n_faces"] == len(out_f) == len(f) + t[1] + 2 * t[2] + 3 * t[3]     # a face with k marked corners: k + 1 children
    assert same_bits(out_v[:nv], v)                                       # bits and index kept
    assert np.array_equal(np.unique(out_f), np.arange(len(out_v)))       # every vertex, the new ones too, is used
    assert (parents[:, 0] < parents[:, 1]).all() and (parents.max(axis=1) < nv + np.arange(len(parents))).all()
    with np.errstate(all="ignore"):
        assert same_bits(out_v[nv:], (out_v[parents[:, 0]] + out_v[parents[:, 1]]) * 0.5)
    # V - E + F
    assert nv - rep["n_edges_before"] + len(f) == len(out_v) - rep["n_edges_after"] + len(out_f)
    assert len(set(directed_edges(f))) == 3 * len(f)
    d = directed_edges(out_f)
    assert len(set(d)) == len(d)                                          # no edge twice in one direction: one winding
    assert rep["n_nonmanifold_edges_before"] == rep["n_nonmanifold_edges_after"] == 0
    if closed:
        assert rep["n_open_edges_before"] == rep["n_open_edges_after"] == 0
        assert set(d) == {(b, a) for a, b in d}
    assert abs(rep["volume_after"] - rep["volume_before"]) <= 1e-9 * abs(rep["volume_before"])
    assert rep["volume_before"] != 0.0
    # the launch count: 6 a splitting pass, 4 the pass that marks nothing, and the two volumes
    assert rep["n_launches"] == 6 * (rep["passes_run"] - 1) + 4 + R.volume_launches(len(f)) + R.volume_launches(len(out_f))


def test_children_of_an_open_edge_are_open():
    v, f = open_tube()
    L = 0.3
    thr2 = R.threshold_sq(L)
    cv, cf = v.tolist(), [tuple(t) for t in f.tolist()]
    on_open = 0
    for _ in range(10):
        table, marked = R.one_pass(cv, cf, thr2)
        if not marked:
            break
        on_open += sum(1 for k in marked if table[k][0] == 1)
        cv, cf, _, _ = R.emit(cv, cf, marked)
    out_v, out_f, _, rep = R.refine(v, f, L)
    assert same_bits(out_v, np.array(cv)) and np.array_equal(out_f, np.array(cf))
    assert rep["n_open_edges_before"] == 2 * 15 and on_open > 0
    assert rep["n_open_edges_after"] == rep["n_open_edges_before"] + on_open


def test_pinned_pass_sizes():
    v, f = octahedron()
    out_v, out_f, _, rep = R.refine(v, f, 0.3)
    assert rep["splits_per_pass"][:4] == [12, 48, 0, 0] and rep["passes_run"] == 3
    assert len(out_v) == 66 and len(out_f) == 128 and rep["faces_by_template"] == [128, 0, 0, 40]
    assert rep["longest_sq_before"] == 2.0 and rep["longest_sq_after"] == 0.125 and rep["volume_before"] == 4.0 / 3.0
    assert rep["bytes_uploaded"] == 24 * 6 + 12 * 8 and rep["bytes_downloaded"] == 24 * 66 + 8 * 60 + 12 * 128
    v, f = stretched_tube()
    _, _, _, rep = R.refine(v, f, 0.3)
    assert rep["splits_per_pass"][:6] == [108, 288, 576, 1728, 0, 0] and rep["passes_run"] == 5 and rep["converged"] == 1


def test_all_four_templates():
    v, f = stretched_tube()
    _, _, _, rep = R.refine(jitter(v, 3), f, 0.25)
    assert all(n > 0 for n in rep["faces_by_template"]), rep["faces_by_template"]


def test_the_two_marked_template_cuts_the_shorter_diagonal():
    v = np.array([[0.0, 0, 0], [4.0, 0, 0], [0.5, 3.0, 0], [2.0, 0, 0], [2.25, 1.5, 0]])       # m0 = 3, m1 = 4
    # (a, b, c) = (0, 1, 2), edges (a, b) and (b, c) marked: |m0 - c|^2 = 11.25 > |a - m1|^2 = 7.3125 -> the a - m1 cut
    assert R.children((0, 1, 2), [3, 4, -1], v) == [(3, 1, 4), (0, 3, 4), (0, 4, 2)]
    v[2] = [3.5, 3.0, 0.0]
    v[4] = [3.75, 1.5, 0.0]                                               # now m0 - c is the shorter one
    assert R.children((0, 1, 2), [3, 4, -1], v) == [(3, 1, 4), (0, 3, 2), (3, 4, 2)]
    assert R.children((2, 0, 1), [-1, 3, 4], v) == [(3, 1, 4), (0, 3, 2), (3, 4, 2)]   # the same face rotated
    v[2] = [4.0, 4.0, 0.0]
    v[4] = [4.0, 2.0, 0.0]                                                # a tie (20 = 20): the a - m1 cut
    assert R.len_sq(v[3], v[2]) == R.len_sq(v[0], v[4]) == 20.0
    assert R.children((0, 1, 2), [3, 4, -1], v) == [(3, 1, 4), (0, 3, 4), (0, 4, 2)]
    assert R.children((0, 1, 2), [3, -1, -1], v) == [(0, 3, 2), (3, 1, 2)]
    assert R.children((0, 1, 2), [-1, -1, 3], v) == [(2, 3, 1), (3, 0, 1)]


def test_messy_input_has_one_defined_result():
    v, f = messy()
    a = R.refine(v, f, 0.6)
    b = R.refine(v.copy(), f.copy(), 0.6)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    rep = a[3]
    assert rep["converged"] == 1 and rep["n_nonmanifold_edges_before"] == 1 and rep["n_nonmanifold_edges_after"] >= 2
    assert same_bits(a[0][:6], v) and rep["longest_sq_after"] <= R.threshold_sq(0.6)
    # the midpoint of the edge with three owners is one vertex for all of them: the first the walk meets
    assert a[2][0].tolist() == [0, 1] and same_bits(a[0][6], [1.0, 0.0, 0.0])
    edges, len_sq = R.edge_lengths(v, f)
    assert edges.tolist()[:3] == [[0, 1], [1, 2], [0, 2]] and [3, 3] not in edges.tolist() and len_sq[0] == 4.0
    assert len(edges) == rep["n_edges_before"] == 9


def test_passes_and_the_vertex_cap():
    v, f = octahedron()
    same, _, par, rep = R.refine(v, f, 0.3, max_passes=0)
    assert same_bits(same, v) and len(par) == 0 and rep["passes_run"] == 0 and rep["converged"] == 0
    assert rep["n_launches"] == 2 + 2 * R.volume_launches(8) and rep["n_edges_before"] == rep["n_edges_after"] == 12
    one = R.refine(v, f, 0.3, max_passes=1)
    assert len(one[0]) == 18 and one[3]["splits_per_pass"][:2] == [12, 0] and one[3]["converged"] == 0
    capped = R.refine(v, f, 0.3, max_vertices=65)
    assert same_bits(capped[0], one[0]) and np.array_equal(capped[1], one[1])
    assert capped[3]["stopped_by_cap"] == 1 and capped[3]["passes_run"] == 1 and capped[3]["converged"] == 0
    assert R.refine(v, f, 0.3, max_vertices=66)[3]["stopped_by_cap"] == 0
    far = R.refine(v, f, 10.0)
    assert same_bits(far[0], v) and np.array_equal(far[1], f) and far[3]["splits_per_pass"][0] == 0
    assert far[3]["converged"] == 1 and far[3]["passes_run"] == 1 and far[3]["faces_by_template"] == [8, 0, 0, 0]


def test_public_names():
    for name in ("mesh_edge_lengths", "edge_length_target", "refine_mesh"):
        assert callable(getattr(mm, name)) and name in mm.__all__
    for sym in ("mm_mesh_edge_lengths", "mm_mesh_refine"):
        assert sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)
    for fn in (mm.stitch, mm.stitch_conditioned):
        assert inspect.signature(fn).parameters["refine"].default is False
    sig = inspect.signature(mm.refine_mesh).parameters
    assert sig["target_edge_length_mm"].default is None and sig["ratio"].default == 4.0 / 3.0 and sig["passes"].default == 10
    assert sig["max_vertices"].default is None and inspect.signature(mm.edge_length_target).parameters["q"].default == 25.0
    import ctypes as C
    assert C.sizeof(mm._native.MMRefineReport) == 8 * (34 + 4)                # 34 integers, 4 doubles


def test_refine_mesh_rejects_bad_arguments_before_the_device():
    mesh = octahedron()
    with pytest.raises(ValueError, match="out of range"):
        mm.refine_mesh((mesh[0], [[0, 1, 6]]), 0.3)
    with pytest.raises(ValueError, match="negative"):
        mm.refine_mesh(mesh, 0.3, passes=-1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            mm.refine_mesh(mesh, bad)
        with pytest.raises(ValueError, match="finite"):
            mm.refine_mesh(mesh, 0.3, ratio=bad)


def test_edge_length_target_is_the_percentile_of_the_edge_lengths(monkeypatch):
    v, f = stretched_tube()
    v = jitter(v, 5)
    edges, len_sq = R.edge_lengths(v, f)
    monkeypatch.setattr(mm.ccta, "mesh_edge_lengths", lambda mesh, engine=None: (edges, np.sqrt(len_sq)))
    assert mm.edge_length_target((v, f)) == float(np.percentile(np.sqrt(len_sq), 25.0))
    assert mm.edge_length_target((v, f), q=60.0) == float(np.percentile(np.sqrt(len_sq), 60.0))


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_refine_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_refine_kernels.hip" in b.SOURCES and "mm_refine.cpp" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_refine_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                 # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        seen.add(name)
    for k in KERNELS:
        assert any(k in n for n in seen), k
    assert len(seen) == len(KERNELS) + 1                                  # k_refine_offsets: the pass and the edge list
    assert not re.search(r"\bglobal_atomic_\w*_f(16|32|64)\b", text)
    assert not re.search(r"\batomic\w*_(f16|f32|f64)\b", text)
    assert not re.search(r"\basm\b", open(src).read())
