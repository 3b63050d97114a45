"""CCTA mesh finishing without a device: the public names, and the checker (tests/mm_checkers/smooth_mesh.py) against
hand-written answers -- the octahedron under Taubin, the tetrahedron under one Laplacian step, the CSR of a messy face
list, rings along a capped tube -- and against scipy's sorted-CSR product on a noisy icosphere, where Taubin must also
keep the volume better than the Laplacian does."""
import numpy as np
import pytest

from mm_checkers import smooth_mesh as SMO
from test_trim_host import octahedron, capped_tube

import multimoda_rs_amd as mm


def tetrahedron():
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * [0.3, 1.7, 2.9] + 0.1
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    return v, f


def icosphere(level=3):
    """The icosahedron subdivided `level` times onto the unit sphere: 10 * 4**level + 2 vertices."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1],
         [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
         [9, 8, 1]]
    v = [np.array(p, dtype=float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    return np.array(v), np.array(f)


def noisy_icosphere():
    v, f = icosphere(3)
    r = np.random.default_rng(642)
    return v * (1.0 + 0.03 * r.standard_normal(len(v)))[:, None], f


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_public_names():
    for name in ("smooth_mesh", "filter_taubin", "filter_laplacian", "mesh_adjacency_csr", "vertex_rings",
                 "postprocess_stitched_mesh"):
        assert callable(getattr(mm, name)) and name in mm.__all__
    for sym in ("mm_mesh_adjacency_csr", "mm_mesh_smooth", "mm_mesh_vertex_rings"):
        assert sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)
    import inspect
    for fn in (mm.stitch, mm.stitch_conditioned):
        assert inspect.signature(fn).parameters["smooth"].default is False


def test_postprocess_flag_and_remesh_keywords():
    mesh = octahedron()
    assert mm.postprocess_stitched_mesh(mesh) is mesh
    assert mm.postprocess_stitched_mesh(mesh, postprocessing=False, iterations=3) is mesh
    for kw in ({"target_edge_length_mm": 0.5}, {"remesh_iterations": 3}):
        with pytest.raises(NotImplementedError, match="remesh"):
            mm.postprocess_stitched_mesh(mesh, postprocessing=True, **kw)


def test_octahedron_taubin_is_exact():
    v, f = octahedron()
    out, rep = SMO.smooth(v, f, SMO.taubin_factors(0.5, 0.5, 10))
    assert 0.75 ** 5 == 0.2373046875 and same_bits(out, v * 0.2373046875)
    assert rep["n_edges"] == 12 and rep["max_degree"] == 4 and rep["n_isolated"] == 0 and rep["steps_run"] == 10
    assert rep["volume_before"] == 4.0 / 3.0 and rep["launches"] == 7 + 10 + 2 * 2 + 1
    assert SMO.taubin_factors(0.5, 0.25, 3) == [0.5, -0.25, 0.5]


def test_tetrahedron_one_laplacian_step_is_the_mean_of_the_others():
    v, f = tetrahedron()
    out, rep = SMO.smooth(v, f, [1.0])
    w = 1.0 / 3.0
    for i in range(4):
        others = [j for j in range(4) if j != i]
        for c in range(3):
            acc = 0.0
            for j in others:
                acc = acc + w * v[j, c]
            assert out[i, c] == v[i, c] + 1.0 * (acc - v[i, c])
    assert rep["max_displacement_sq"] == max(float(((out[i] - v[i])[0] ** 2 + (out[i] - v[i])[1] ** 2) + (out[i] - v[i])[2] ** 2)
                                             for i in range(4))


def test_csr_of_a_messy_face_list():
    f = [[0, 1, 2], [2, 1, 0], [0, 1, 2], [3, 3, 4], [5, 2, 5]]            # a repeat (twice), (a, a, b), (a, b, a); 6 unreferenced
    off, nb, info = SMO.csr(f, 7)
    rows = [nb[off[i]:off[i + 1]].tolist() for i in range(7)]
    assert rows == [[1, 2], [0, 2], [0, 1, 5], [4], [3], [2], []]
    assert info == {"entries": 10, "max_degree": 3, "isolated": 1, "n_edges": 5, "launches": 7}
    off, nb, info = SMO.csr(np.zeros((0, 3), dtype=np.int64), 3)
    assert off.tolist() == [0, 0, 0, 0] and nb.size == 0 and info["isolated"] == 3 and info["launches"] == 0


def test_isolated_and_pinned_vertices_keep_their_bits():
    v, f = octahedron()
    v = np.concatenate([v, [[7.0, -0.0, 3.0]]])                             # unreferenced: trimesh would pull it to the origin
    pinned = np.zeros(7, dtype=bool)
    pinned[4] = True
    out, rep = SMO.smooth(v, f, [0.5, -0.25, 0.0], pinned)
    assert same_bits(out[6], v[6]) and same_bits(out[4], v[4]) and rep["n_isolated"] == 1 and rep["n_pinned"] == 1
    assert not np.array_equal(out[0], v[0])
    free, _ = SMO.smooth(v, f, [0.5, -0.25, 0.0])
    assert not np.array_equal(free[0], out[0])                              # the pinned apex still pulls its neighbours
    same, rep0 = SMO.smooth(v, f, [])
    assert same_bits(same, v) and rep0["volume_before"] == rep0["volume_after"] and rep0["max_displacement_sq"] == 0.0


def test_rings_along_a_capped_tube():
    n_around, n_rings = 7, 5
    v, f = capped_tube(n_around, n_rings)
    centre = n_around * n_rings
    ring, info = SMO.rings(f, len(v), [centre], 100)
    want = np.concatenate([np.repeat(np.arange(1, n_rings + 1), n_around), [0, n_rings + 1]])
    assert ring.tolist() == want.tolist() and ring.dtype == np.int32
    assert info == {"reached": len(v), "rounds": n_rings + 2, "launches": 7 + 1 + n_rings + 2}
    cut, info = SMO.rings(f, len(v), [centre], 2)
    assert cut.tolist() == np.where(want <= 2, want, -1).tolist() and info["rounds"] == 2
    assert SMO.rings(f, len(v), [centre], 0)[0].tolist() == np.where(want == 0, 0, -1).tolist()
    # a second body no seed touches
    ov, of = octahedron()
    both_f = np.concatenate([f, of + len(v)])
    far, info = SMO.rings(both_f, len(v) + 6, [centre, centre], 100)
    assert far[:len(v)].tolist() == want.tolist() and (far[len(v):] == -1).all() and info["reached"] == len(v)


def test_checker_equals_sorted_scipy_csr_and_taubin_keeps_the_volume():
    import scipy.sparse as sp
    v, f = noisy_icosphere()
    assert len(v) == 642
    off, nb, _ = SMO.csr(f, len(v))
    deg = np.diff(off)
    L = sp.csr_matrix((np.repeat(1.0 / deg, deg), nb, off), shape=(len(v), len(v)))
    assert L.has_sorted_indices
    factors = SMO.taubin_factors(0.5, 0.5, 10)
    x = v.copy()
    for fac in factors:
        d = L.dot(x) - x
        x = x + fac * d
    taubin, rt = SMO.smooth(v, f, factors)
    assert same_bits(taubin, x)
    # the (sum x_j) / deg form is another function: the rule is w * x_j
    y = v.copy()
    A = sp.csr_matrix((np.ones(len(nb)), nb, off), shape=(len(v), len(v)))
    for fac in factors:
        y = y + fac * (A.dot(y) / deg[:, None] - y)
    assert not same_bits(taubin, y) and np.allclose(taubin, y, rtol=0, atol=1e-12)
    lap, rl = SMO.smooth(v, f, [0.5] * 10)
    assert rt["volume_before"] == rl["volume_before"] > 4.0
    assert abs(rt["volume_after"] - rt["volume_before"]) < abs(rl["volume_after"] - rl["volume_before"])
    assert rl["volume_after"] < rt["volume_after"]
