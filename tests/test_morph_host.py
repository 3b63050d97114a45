"""CCTA mesh morphing, host side: the Python checker (tests/mm_checkers/scale_coronary.py) and the host C ABI
(mm_keep_largest_component, mm_match_points) with the package's keep_largest_connected_component,
sync_results_to_mesh and the no-match path of scale_region_centerline_morphing, against known answers restated from the
reference's own tests (tests/test_ccta.py TestKeepLargestConnectedComponent / TestSyncResultsToMesh /
TestScaleRegionCenterlineMorphing / test_sync_results_to_mesh_remaps_per_ring_keys; scale_coronary.rs:414) and against
each other on random meshes.  No GPU."""
import math
import types

import numpy as np
import pytest

from mm_checkers import scale_coronary as SC

import multimoda_rs_amd as mm

N = mm._native
MM_ERR_INVALID = -2                                                          # include/mm_hausdorff.h
GRID_V = [(float(x), float(y), 0.0) for y in range(3) for x in range(3)]          # 3 x 3 grid, vertex 4 in the centre
GRID_F = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [3, 4, 6], [4, 7, 6], [4, 5, 7], [5, 8, 7]]


def grid_mesh():
    return types.SimpleNamespace(vertices=np.array(GRID_V), faces=np.array(GRID_F))


def grid_results(mesh):
    v = [tuple(p) for p in mesh.vertices]
    return {"mesh": mesh, "aorta_points": v[6:9], "rca_points": v[0:3], "lca_points": v[3:6], "rca_removed_points": [],
            "lca_removed_points": []}


def rows(a):
    return {tuple(r) for r in np.asarray(a, dtype=np.float64).reshape(-1, 3).tolist()}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3)).view(np.uint64)


# ---- TestKeepLargestConnectedComponent (test_ccta.py:556-587), on the package and on the checker ------------------
@pytest.mark.parametrize("impl", ["package", "checker"])
class TestKeepLargestConnectedComponent:
    @staticmethod
    def call(impl, points):
        f = mm.keep_largest_connected_component if impl == "package" else SC.keep_largest_connected_component
        return f(GRID_V, GRID_F, points)

    def test_drops_isolated_point(self, impl):
        r = self.call(impl, [GRID_V[i] for i in (0, 1, 3, 4, 8)])
        assert rows(r) == {GRID_V[i] for i in (0, 1, 3, 4)} and len(r) == 4

    def test_fully_connected_set_unchanged(self, impl):
        pts = [GRID_V[i] for i in (0, 1, 3)]
        assert rows(self.call(impl, pts)) == set(pts)

    def test_empty_input_returns_empty(self, impl):
        assert len(self.call(impl, [])) == 0

    def test_single_point_returns_unchanged(self, impl):
        assert rows(self.call(impl, [GRID_V[0]])) == {GRID_V[0]}

    def test_points_not_on_mesh_returned_unchanged(self, impl):
        pts = [(99.0, 99.0, 99.0), (100.0, 100.0, 100.0)]
        r = self.call(impl, pts)
        assert [tuple(p) for p in np.asarray(r).tolist()] == pts


def test_keep_largest_returns_vertices_ascending_and_breaks_ties_by_smallest_vertex():
    # {0, 1} and {7, 8} are two components of 2 (0-1 share faces; 7-8 share one): the one holding vertex 0 stays
    pts = [GRID_V[8], GRID_V[7], GRID_V[1], GRID_V[0]]
    want = [GRID_V[0], GRID_V[1]]
    assert [tuple(p) for p in mm.keep_largest_connected_component(GRID_V, GRID_F, pts).tolist()] == want
    assert SC.keep_largest_connected_component(GRID_V, GRID_F, pts) == want


def test_keep_largest_abi_contract():
    L = N.lib()
    v, f = np.array(GRID_V), np.array(GRID_F, dtype=np.int64)
    p = v[[0, 1, 3, 8]].copy()
    keep = np.zeros(4, dtype=np.int64)
    assert L.mm_keep_largest_component(N._ptr(v), 9, N._ptr(f), 8, N._ptr(p), 4, N._ptr(keep)) == 3
    assert keep[:3].tolist() == [0, 1, 3]
    assert L.mm_keep_largest_component(N._ptr(v), 9, N._ptr(f), 8, N._ptr(p), 1, N._ptr(keep)) == 0     # unchanged
    far = np.full((2, 3), 50.0)
    assert L.mm_keep_largest_component(N._ptr(v), 9, N._ptr(f), 8, N._ptr(far), 2, N._ptr(keep)) == 0   # unchanged
    big = f.copy()
    big[0] = [0, 1, 99]                                                    # an index >= nv is never in the subset
    assert L.mm_keep_largest_component(N._ptr(v), 9, N._ptr(big), 8, N._ptr(p), 4, N._ptr(keep)) == 3
    neg = f.copy()
    neg[2, 1] = -1
    assert L.mm_keep_largest_component(N._ptr(v), 9, N._ptr(neg), 8, N._ptr(p), 4, N._ptr(keep)) == MM_ERR_INVALID
    with pytest.raises(RuntimeError):
        mm.keep_largest_connected_component(GRID_V, neg, p)


# ---- TestSyncResultsToMesh (test_ccta.py:769-802) and the per-ring key case (:1856-1870) -------------------------
class TestSyncResultsToMesh:
    def test_mesh_replaced(self):
        g = grid_mesh()
        new = types.SimpleNamespace(vertices=g.vertices + 1.0, faces=g.faces)
        assert mm.sync_results_to_mesh(grid_results(g), g, new)["mesh"] is new

    def test_coordinate_lists_updated(self):
        g = grid_mesh()
        new = types.SimpleNamespace(vertices=g.vertices + np.array([10.0, 0.0, 0.0]), faces=g.faces)
        up = mm.sync_results_to_mesh(grid_results(g), g, new)
        assert all(p[0] >= 10.0 for p in up["rca_points"])

    def test_preserves_number_of_labeled_points(self):
        g = grid_mesh()
        res = grid_results(g)
        up = mm.sync_results_to_mesh(res, g, types.SimpleNamespace(vertices=g.vertices * 2, faces=g.faces))
        assert len(up["rca_points"]) == len(res["rca_points"])


def test_sync_results_to_mesh_remaps_per_ring_keys():
    g = grid_mesh()
    ring = [tuple(g.vertices[i]) for i in (0, 1, 2, 5, 8, 7, 6, 3)]
    res = {"mesh": g, "boundary_points": ring, "boundary_points_1": ring, "boundary_points_2": ring[:3],
           "rca_points_main": ring, "aorta_points": []}
    moved = types.SimpleNamespace(vertices=g.vertices + np.array([0.0, 0.0, 5.0]), faces=g.faces)
    up = mm.sync_results_to_mesh(res, g, moved)
    for key in ("boundary_points", "boundary_points_1", "boundary_points_2"):
        assert len(up[key]) == len(res[key])
        assert all(p[2] == q[2] + 5.0 for p, q in zip(up[key], res[key]))
    assert up["rca_points_main"] is res["rca_points_main"] and up["aorta_points"] == []   # not remapped / empty
    assert res["mesh"] is g                                                                  # a new dict


def test_sync_results_last_old_index_wins_and_unmatched_points_drop():
    old = np.array([[0.0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]])
    new = old + np.arange(4)[:, None] * 10.0
    res = {"rca_points": [(0.0, 0.0, 0.0), (5.0, 5.0, 5.0), (-0.0, 0.0, 0.0), (math.nan, 0.0, 0.0), (2.0, 0.0, 0.0)]}
    up = mm.sync_results_to_mesh(res, (old, None), (new, None))
    want = SC.sync_results_to_mesh(res, old, new)["rca_points"]
    assert up["rca_points"].tolist() == [list(p) for p in want] == [[20.0, 20.0, 20.0], [20.0, 20.0, 20.0],
                                                                    [32.0, 30.0, 30.0]]


# ---- TestScaleRegionCenterlineMorphing (test_ccta.py:842-857): the no-match path never reads the centerline -------
class TestScaleRegionCenterlineMorphing:
    def test_no_matching_vertices_returns_copy(self):
        g = grid_mesh()
        r = mm.scale_region_centerline_morphing(g, [(999.0, 999.0, 999.0)], None, 1.0)
        assert len(r.vertices) == len(g.vertices) and r is not g
        assert np.array_equal(r.vertices, g.vertices) and r.vertices is not g.vertices

    def test_tuple_mesh_gives_tuple(self):
        v, f = np.array(GRID_V), np.array(GRID_F)
        r = mm.scale_region_centerline_morphing((v, f), [], None, 1.0)
        assert isinstance(r, tuple) and r[1] is f and np.array_equal(r[0], v) and r[0] is not v


# ---- the morph KAT of scale_coronary.rs:414-460, on the checker ----------------------------------------------------
def test_morph_kat_on_checker():
    out, idx = SC.diameter_morphing([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)], [(1.0, 1.0, 0.0)], 1.0)
    assert idx == [1]
    assert abs(out[0][0] - 1.0) < 1e-6 and abs(out[0][1] - 2.0) < 1e-6 and abs(out[0][2]) < 1e-6


def test_checker_morph_rules():
    cl = [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0)]
    assert SC.closest_index(cl, (1.0, 3.0, 0.0)) == 0                       # a tie keeps the lowest index
    assert SC.closest_index(cl, (math.nan, 0.0, 0.0)) == 0                  # no distance below f64::MAX: index 0
    assert SC.closest_index([(math.nan, 0, 0), (5.0, 0, 0)], (0.0, 0, 0)) == 1   # a NaN distance never wins
    assert SC.move((2.0, 0.0, 0.0), (2.0, 0.0, 0.0), 3.0) == (2.0, 0.0, 0.0)     # on its centerline point: stays
    q = SC.move((math.inf, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    assert math.isnan(q[0]) and q[1:] == (0.0, 0.0)                          # |v| = inf > 0: inf / inf = NaN
    q = SC.move((math.nan, 1.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    assert math.isnan(q[0]) and q[1:] == (1.0, 0.0)                          # a NaN norm keeps the point
    cl3 = np.random.default_rng(1).normal(size=(40, 3))
    pts = np.random.default_rng(2).normal(size=(300, 3))
    assert SC.nearest_indices(cl3, pts).tolist() == [SC.closest_index(SC.tuples(cl3), p) for p in SC.tuples(pts)]


def test_checker_morph_matches_host_abi():
    """The checker against the host mm_diameter_morphing (the same fold and move, no GPU)."""
    r = np.random.default_rng(3)
    cl = mm.Centerline.from_contour_points(np.cumsum(r.normal(size=(50, 3)), axis=0))
    pts = r.normal(scale=4.0, size=(400, 3))
    got = mm.adjust_diameter_centerline_morphing_simple(cl, pts, 0.7)
    want, _ = SC.diameter_morphing(cl.xyz(), SC.tuples(pts), 0.7)
    assert np.array_equal(bits(got), bits(want))


# ---- mm_match_points ------------------------------------------------------------------------------------------------
def test_match_points_is_bitwise_and_last_index_wins():
    L = N.lib()
    keys = np.array([[1.0, 2, 3], [0.0, 0, 0], [1.0, 2, 3], [-0.0, 0, 0], [math.nan, 0, 0]])
    q = np.array([[1.0, 2, 3], [0.0, 0, 0], [-0.0, 0, 0], [math.nan, 0, 0], [7.0, 7, 7]])
    idx = np.zeros(5, dtype=np.int64)
    assert L.mm_match_points(N._ptr(keys), 5, N._ptr(q), 5, N._ptr(idx)) == 4
    assert idx.tolist() == [2, 1, 3, 4, -1]                                  # bit patterns: NaN matches its own bits
    assert mm.ccta._match(keys, q).tolist() == [2, 3, 3, -1, -1]             # by value: -0.0 == 0.0, NaN equals nothing
    assert L.mm_match_points(N._ptr(keys), 5, None, 0, None) == 0
    assert L.mm_match_points(None, 1, N._ptr(q), 5, N._ptr(idx)) == MM_ERR_INVALID


# ---- the checker against the host ABI on random meshes --------------------------------------------------------------
def random_mesh(seed, nv=60, nf=90):
    r = np.random.default_rng(seed)
    v = r.integers(0, 6, size=(nv, 3)).astype(np.float64)                   # a coarse lattice: duplicated coordinates
    v[r.random(nv) < 0.1] *= -1.0                                            # -0.0 where a coordinate is 0
    f = r.integers(0, nv, size=(nf, 3))
    f[r.random(nf) < 0.05, 2] = nv + 7                                       # out-of-range corners
    return v, f


@pytest.mark.parametrize("seed", range(12))
def test_keep_largest_checker_vs_abi_random(seed):
    v, f = random_mesh(seed)
    r = np.random.default_rng(100 + seed)
    pts = v[r.choice(v.shape[0], size=25, replace=True)].copy()
    pts[0, 1] = math.nan
    pts[1] = [0.0, -0.0, 9.0]
    pts[2] = [42.0, 42.0, 42.0]
    got = mm.keep_largest_connected_component(v, f, pts)
    want = SC.keep_largest_connected_component(v, f, SC.tuples(pts))
    assert np.array_equal(bits(got), bits(np.array(want)))


def test_keep_largest_equal_components_keep_smallest_vertex():
    v = np.array([[float(i), 0.0, 0.0] for i in range(9)])
    f = np.array([[6, 7, 8], [0, 1, 2], [3, 4, 5]])                          # three triangles, three equal components
    pts = v[[8, 7, 6, 5, 4, 3, 2, 1, 0]]
    got = mm.keep_largest_connected_component(v, f, pts)
    assert got.tolist() == v[:3].tolist() == [list(p) for p in SC.keep_largest_connected_component(v, f, SC.tuples(pts))]


@pytest.mark.parametrize("seed", range(6))
def test_sync_checker_vs_package_random(seed):
    v, _ = random_mesh(seed)
    new = v + np.random.default_rng(seed).normal(size=v.shape)
    r = np.random.default_rng(200 + seed)
    res = {k: SC.tuples(v[r.choice(v.shape[0], size=20)]) for k in SC_KEYS}
    res["rca_points"][0] = (math.nan, 0.0, 0.0)
    res["lca_points"][1] = (-0.0, -0.0, -0.0)
    res["lca_points"][2] = (0.0, 0.0, 0.0)
    res["boundary_points_2"] = [(99.0, 0.0, 0.0)] + res["aorta_points"][:3]
    got = mm.sync_results_to_mesh(dict(res), (v, None), (new, None))
    want = SC.sync_results_to_mesh(dict(res), v, new)
    for k in SC_KEYS + ("boundary_points_2",):
        assert np.array_equal(bits(got[k]), bits(np.array(want[k]))), k


SC_KEYS = ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "proximal_points", "boundary_points")
