"""CCTA mesh trimming without a device: the checker (tests/mm_checkers/trim_mesh.py) and the host rim logic
(mm_boundary_rings) against the known answers of the reference's own boundary tests, the host rounds of
clean_open_boundary against the checker, the dict semantics of remove / keep on the checker, build_adjacency_map,
the rejection of invalid indices, and a binary STL of type "all"."""
import ctypes as C
import itertools

import numpy as np
import pytest

from mm_checkers import trim_mesh as TM

import multimoda_rs_amd as mm

N = mm._native


def grid_with_hole(n=9, remove=None):
    """n x n grid in z = 0 (vertex j * n + i at (i, j)), two triangles per quad, without the faces of the removed
    vertices (default: the centre).  Returns (vertices, kept faces, removed, rim seeds)."""
    vid = lambda i, j: j * n + i                                                            # noqa: E731
    xs, ys = np.meshgrid(np.arange(n), np.arange(n))
    v = np.column_stack([xs.ravel().astype(float), ys.ravel().astype(float), np.zeros(n * n)])
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            f.append([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)])
            f.append([vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)])
    f = np.array(f, dtype=np.int64)
    removed = [vid(n // 2, n // 2)] if remove is None else [vid(*p) for p in remove]
    keep = ~np.any(np.isin(f, removed), axis=1)
    seeds = set(f[~keep].ravel().tolist()) - set(removed)
    return v, f[keep], removed, seeds


def full_grid(n=9):
    v, f, _, _ = grid_with_hole(n, remove=[])
    return v, f


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=float)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, f


def capped_tube(n_around=8, n_rings=5):
    v, f = mm.synth._tube(np.stack([np.zeros(n_rings), np.zeros(n_rings), np.arange(n_rings, dtype=float)], 1),
                          np.tile([1.0, 0, 0], (n_rings, 1)), np.tile([0, 1.0, 0], (n_rings, 1)), 1.0, n_around)
    nv = v.shape[0]
    v = np.concatenate([v, [[0, 0, 0], [0, 0, n_rings - 1.0]]])
    caps = [[nv, (k + 1) % n_around, k] for k in range(n_around)]
    top = (n_rings - 1) * n_around
    caps += [[nv + 1, top + k, top + (k + 1) % n_around] for k in range(n_around)]
    return v, np.concatenate([f, np.array(caps)])


CARRY_NV = 256 * 4096 + 4097                    # 258 scan tiles: the one-workgroup tile scan takes a second round


def band_across_the_carry(nv=CARRY_NV):
    """A closed band of 300 faces (two rows of 150 vertices on a circle of radius 10, one unit apart in z) whose 300
    vertices sit at the indices around 0, the first scan tile's end (4095 | 4096), the first round's end of the tile scan
    (2^20 - 1 | 2^20) and nv - 1; every other vertex is isolated, at distinct coordinates far away.  Returns
    (vertices, faces, lower row, upper row): column j of the band is (lower[j], upper[j])."""
    ids = np.concatenate([np.arange(50), np.arange(4046, 4146), np.arange(2 ** 20 - 50, 2 ** 20 + 50),
                          np.arange(nv - 50, nv)])
    lower, upper = ids[0::2], ids[1::2]
    m = len(lower)
    v = 1000.0 + np.arange(3 * nv, dtype=np.float64).reshape(nv, 3)
    a = 2.0 * np.pi * np.arange(m) / m
    v[lower] = np.column_stack([10.0 * np.cos(a), 10.0 * np.sin(a), np.zeros(m)])
    v[upper] = v[lower] + [0.0, 0.0, 1.0]
    j, k = np.arange(m), (np.arange(m) + 1) % m
    f = np.concatenate([np.column_stack([lower[j], lower[k], upper[j]]), np.column_stack([lower[k], upper[k], upper[j]])])
    return v, f.astype(np.int64), lower, upper


def open_edge_degrees(faces):
    deg = {}
    for a, b in TM.open_boundary_edges(faces).tolist():
        deg[a] = deg.get(a, 0) + 1
        deg[b] = deg.get(b, 0) + 1
    return set(deg.values())


def traces_real_edges(faces, ring):
    edges = {frozenset(e) for e in TM.open_boundary_edges(faces).tolist()}
    n = len(ring)
    return n > 0 and all(frozenset((int(ring[k]), int(ring[(k + 1) % n]))) in edges for k in range(n))


def host_clean(faces, vertices, seeds, target_n=1, despike_cos=0.0, max_rounds=64):
    """clean_open_boundary with the native host rounds (mm_boundary_rings) and the checker's face stage."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    drop, seed = set(), set(seeds)
    for _ in range(max_rounds):
        alive = f[~np.any(np.isin(f, list(drop)), axis=1)] if drop else f
        rings, cull, rim = mm.ccta.boundary_rings_from_edges(TM.open_boundary_edges(alive), vertices, seed, target_n,
                                                             despike_cos, clean=True)
        if rim.size == 0:
            return sorted(drop), []
        seed |= set(rim.tolist())
        if cull.size == 0:
            return sorted(drop), [r.tolist() for r in rings]
        drop |= set(cull.tolist())
    alive = f[~np.any(np.isin(f, list(drop)), axis=1)] if drop else f
    rings = mm.ccta.boundary_rings_from_edges(TM.open_boundary_edges(alive), vertices, seed, target_n)[0]
    return sorted(drop), [r.tolist() for r in rings]


def host_order(faces, vertices, seeds=None, target_n=None):
    rings = mm.ccta.boundary_rings_from_edges(TM.open_boundary_edges(faces), vertices, seeds, target_n)[0]
    return [r.tolist() for r in rings]


class TestOpenBoundaryEdges:
    def test_empty_faces(self):
        assert TM.open_boundary_edges(np.empty((0, 3), dtype=np.int64)).shape == (0, 2)

    def test_closed_meshes_have_none(self):
        for v, f in (octahedron(), capped_tube()):
            assert len(TM.open_boundary_edges(f)) == 0

    def test_hole_and_perimeter_are_open(self):
        _, f, _, _ = grid_with_hole()
        assert len(TM.open_boundary_edges(f)) == 32 + 6

    def test_every_returned_edge_used_once_and_sorted(self):
        _, f, _, _ = grid_with_hole()
        from collections import Counter
        counts = Counter(frozenset(e) for e in f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2).tolist())
        e = TM.open_boundary_edges(f)
        assert all(counts[frozenset(x)] == 1 for x in e.tolist())
        assert (e[:, 0] <= e[:, 1]).all() and e.tolist() == sorted(e.tolist())


class TestOrderBoundaryRings:
    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_reports_every_rim_without_seeds(self, impl):
        v, f, _, _ = grid_with_hole()
        rings = TM.order_boundary_rings(f, v) if impl == "checker" else host_order(f, v)
        assert [len(r) for r in rings] == [32, 6]

    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_seeds_select_only_the_touching_rim(self, impl):
        v, f, _, seeds = grid_with_hole()
        rings = TM.order_boundary_rings(f, v, seeds) if impl == "checker" else host_order(f, v, seeds)
        assert [len(r) for r in rings] == [6] and traces_real_edges(f, rings[0])
        assert rings[0][0] == min(rings[0])                                      # the walk starts at the smallest

    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_target_n_reduces_ring_count(self, impl):
        v, f, _, _ = grid_with_hole()
        rings = TM.order_boundary_rings(f, v, target_n=1) if impl == "checker" else host_order(f, v, target_n=1)
        assert len(rings) == 1 and len(rings[0]) == 38

    def test_no_open_boundary_returns_empty(self):
        v, f = octahedron()
        assert TM.order_boundary_rings(f, v) == [] and host_order(f, v) == []

    def test_walk_rule(self):
        v, f, _, seeds = grid_with_hole(n=5)
        ring = host_order(f, v, seeds)[0]
        assert ring == TM.order_boundary_rings(f, v, seeds)[0]
        # the hole around (2, 2): its smallest vertex first, then its smallest neighbour on the rim
        assert ring[0] == 6 and ring[1] == 7


class TestCleanOpenBoundary:
    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_clean_hole_needs_no_culling(self, impl):
        v, f, _, seeds = grid_with_hole()
        drop, rings = (TM.clean_open_boundary if impl == "checker" else host_clean)(f, v, seeds)
        assert drop == [] and [len(r) for r in rings] == [6]

    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_pinch_junction_is_culled_from_the_mesh(self, impl):
        v, f, _, seeds = grid_with_hole(remove=[(4, 4), (6, 6)])
        assert 4 in open_edge_degrees(f)
        drop, rings = (TM.clean_open_boundary if impl == "checker" else host_clean)(f, v, seeds)
        assert len(drop) == 1
        surviving = f[~np.any(np.isin(f, drop), axis=1)]
        assert open_edge_degrees(surviving) == {2}
        assert traces_real_edges(surviving, rings[0])

    @pytest.mark.parametrize("impl", ["checker", "host"])
    def test_returns_empty_when_seeds_match_nothing(self, impl):
        v, f, _, _ = grid_with_hole()
        drop, rings = (TM.clean_open_boundary if impl == "checker" else host_clean)(f, v, {10_000})
        assert rings == [] and drop == []

    @pytest.mark.parametrize("case", range(8))
    def test_host_rounds_equal_the_checker(self, case):
        r = np.random.default_rng(case)
        n = 12
        holes = {(int(a), int(b)) for a, b in r.integers(1, n - 1, size=(4 + case, 2))}
        v, f, _, seeds = grid_with_hole(n, remove=sorted(holes))
        v = v + r.normal(scale=0.2, size=v.shape) * (case % 2)
        for target_n, cos, rounds, s in itertools.product((1, 2, None), (0.0, -0.5), (64, 1, 0), (seeds, set())):
            assert host_clean(f, v, s, target_n, cos, rounds) == TM.clean_open_boundary(f, v, s, target_n, cos, rounds)
            assert host_order(f, v, s or None, target_n) == TM.order_boundary_rings(f, v, s or None, target_n)

    def test_despike_drops_a_bump(self):
        # a square rim with one vertex pushed out and back: the cosine at the tip is near +1
        V = [(0.0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (1.0, 5.0, 0), (1.0, 1.0, 0), (0, 1, 0)]
        ring = [0, 1, 2, 3, 4, 5, 6]
        out = TM.despike_ring(ring, V, 0.0)
        assert 4 not in out and len(out) < len(ring)


def grid_results():
    """The 9 x 9 grid labelled in horizontal bands, with the centre blob as the anomalous region."""
    v, f = full_grid()
    t = [tuple(x) for x in v.tolist()]
    return {"mesh": (v, f), "rca_points": np.array(t[0:27]), "lca_points": np.array(t[27:36]),
            "aorta_points": np.array(t[54:81]), "anomalous_points": np.array([t[39], t[40], t[41], t[49]]),
            "rca_removed_points": np.zeros((0, 3)), "boundary_points_7": np.ones((2, 3))}


class TestRemoveAndKeep:
    def test_remove_clears_the_key_and_stays_consistent(self):
        res = grid_results()
        out = TM.remove_labeled_points_from_mesh(res, "anomalous_points")
        v, f = out["mesh"]
        assert out["anomalous_points"].shape == (0, 3)
        assert "boundary_points_7" not in out and len(out["boundary_points_1"]) > 0
        assert len(out["boundary_points"]) == len(out["boundary_points_1"])
        vs = {tuple(x) for x in v.tolist()}
        for k in ("rca_points", "lca_points", "aorta_points", "boundary_points"):
            assert all(tuple(p) in vs for p in out[k].tolist()), k
        assert f.min() >= 0 and f.max() < len(v)
        assert len(v) == 81 - 4

    def test_string_and_one_element_list_agree(self):
        a = TM.remove_labeled_points_from_mesh(grid_results(), "anomalous_points")
        b = TM.remove_labeled_points_from_mesh(grid_results(), ["anomalous_points"])
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a if k != "mesh")
        a = TM.keep_labeled_points_from_mesh(grid_results(), "rca_points")
        b = TM.keep_labeled_points_from_mesh(grid_results(), ["rca_points"])
        assert np.array_equal(a["mesh"][0], b["mesh"][0]) and np.array_equal(a["mesh"][1], b["mesh"][1])

    def test_keep_filters_every_list(self):
        out = TM.keep_labeled_points_from_mesh(grid_results(), "rca_points")
        assert len(out["mesh"][0]) == 27 and len(out["rca_points"]) == 27
        assert out["lca_points"].shape == (0, 3) and out["aorta_points"].shape == (0, 3)
        assert len(out["anomalous_points"]) == 4                                  # not a filtered key

    def test_remove_of_another_key_leaves_anomalous_points(self):
        out = TM.remove_labeled_points_from_mesh(grid_results(), "lca_points", target_boundaries=2)
        assert len(out["anomalous_points"]) == 4

    def test_nothing_to_remove_returns_the_same_dict(self):
        res = grid_results()
        assert TM.remove_labeled_points_from_mesh(res, "rca_removed_points") is res
        res["x"] = np.array([[99.0, 99.0, 99.0]])
        assert TM.remove_labeled_points_from_mesh(res, "x") is res
        assert TM.keep_labeled_points_from_mesh(res, "x") is res


class TestBoundaryRingStorage:
    def test_per_ring_keys_and_flat_list(self):
        v, _ = full_grid(3)
        d = {"boundary_points_1": 1, "boundary_points_2": 2, "boundary_points_3": 3, "other": 4}
        mm.ccta._store_boundary_rings(d, v, [np.array([0, 1, 2]), np.array([4, 5])])
        assert sorted(d) == ["boundary_points", "boundary_points_1", "boundary_points_2", "other"]
        assert d["boundary_points_1"].tolist() == v[[0, 1, 2]].tolist()
        assert d["boundary_points"].tolist() == v[[0, 1, 2, 4, 5]].tolist()

    def test_no_rings(self):
        d = {"boundary_points_1": 1}
        mm.ccta._store_boundary_rings(d, np.zeros((3, 3)), [])
        assert list(d) == ["boundary_points"] and d["boundary_points"].shape == (0, 3)


def test_build_adjacency_map_docstring_example():
    adj = mm.build_adjacency_map([[0, 1, 2], [1, 2, 3]])
    assert adj[1] == {0, 2, 3}
    assert adj == TM.build_adjacency_map([[0, 1, 2], [1, 2, 3]])
    f = np.random.default_rng(3).integers(0, 40, size=(200, 3))
    assert mm.build_adjacency_map(f) == TM.build_adjacency_map(f)
    assert mm.build_adjacency_map([[5, 5, 6]]) == {5: {5, 6}, 6: {5}}


def test_invalid_indices_are_rejected():
    v, f, _, _ = grid_with_hole()
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError):
        mm.order_boundary_rings(bad, v)
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        mm.clean_open_boundary(bad, v, {1})
    with pytest.raises(ValueError):
        mm.build_adjacency_map(bad)
    with pytest.raises(ValueError):
        mm.remove_labeled_points_from_mesh({"mesh": (v, bad), "anomalous_points": v[:3]})
    with pytest.raises(ValueError):
        mm.ccta.boundary_rings_from_edges([[0, len(v)]], v)
    L = N.lib()
    e = np.array([[0, 1], [1, 200]], dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    buf = [np.zeros(8, dtype=np.int64) for _ in range(4)]
    assert L.mm_boundary_rings(N._ptr(e), 2, None, 0, N._ptr(v), len(v), -1, 0.0, 0, *(N._ptr(b) for b in buf),
                               N._ptr(counts)) == -2
    big = np.zeros((1, 3), dtype=np.int64)
    assert L.mm_build_adjacency(N._ptr(big), 1, 2 ** 31 + 5, None, None) == -2
    assert L.mm_trim_mesh(None, N._ptr(v), len(v), N._ptr(f), len(f), None, 0, 1, 0.0, 64, None, None, None, None,
                          None) == -2
    with pytest.raises(ValueError):
        mm.ccta.boundary_rings_from_edges([[0, 1]], v, target_n=0)


def test_export_all_writes_the_mesh_as_binary_stl(tmp_path):
    v, f = capped_tube()
    v = v + 0.25
    f = np.concatenate([f, [[0, 0, 1]]])                                           # a degenerate face: zero normal
    path = mm.export_section_stl({"mesh": (v, f)}, "all", tmp_path / "out")
    n, tri = TM.read_stl(path)
    assert path.endswith("all.stl") and tri.shape == (len(f), 3, 3)
    assert np.array_equal(tri, v[f].astype(np.float32))
    assert np.array_equal(n[-1], np.zeros(3, dtype=np.float32))
    lens = np.linalg.norm(n[:-1].astype(np.float64), axis=1)
    assert np.allclose(lens, 1.0, atol=1e-6)
    c = np.cross(v[f[:-1, 1]] - v[f[:-1, 0]], v[f[:-1, 2]] - v[f[:-1, 0]])
    assert np.allclose(n[:-1], c / np.linalg.norm(c, axis=1, keepdims=True), atol=1e-6)
    with pytest.raises(ValueError, match="Unknown export type 'x'. Choose one of: 'all', 'aorta', 'rca', 'lca'."):
        mm.export_section_stl({"mesh": (v, f)}, "x", tmp_path)
