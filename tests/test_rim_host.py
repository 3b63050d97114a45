"""Rim conditioning without a device: the host ring arithmetic of csrc/mm_rim.cpp, through the C ABI and the stage
functions of multimoda_rs_amd.ccta, against the checker (tests/mm_checkers/rim_condition.py); the checker's fans on hand
meshes against answers worked out by hand (tests/test_gpu_rim.py runs the same meshes on the device); rejections.

Coordinates that pass through the plane fit are compared at 1e-9 mm: the coordinates are below 10^3 mm, a
backward-stable normal is off by a few tens of eps over the relative singular gap (asserted >= 0.1 on the checker's own
SVD: below 1e-13), a projection moves a point by its distance times that (below 1e-12 mm for extents of ~10 mm), and
smoothing and rescaling amplify by less than 10.  Indices, counts and flags are exact."""
import ctypes as C

import numpy as np
import pytest

from mm_checkers import rim_condition as K
from test_stitch_host import same_bits

import multimoda_rs_amd as mm

N = mm._native
ccta = mm.ccta
TOL = 1e-9


def irregular_ring(n, seed, a=5.0, b=4.0, noise=0.2, centre=(100.0, -50.0, 30.0), tilt=True):
    """A seeded noisy ellipse with uneven spacing (regular polygons tie), tilted and moved off the origin."""
    r = np.random.default_rng(seed)
    t = np.sort(r.uniform(0, 2 * np.pi, n))
    p = np.stack([a * np.cos(t), b * np.sin(t), noise * r.normal(size=n)], 1)
    if tilt:
        p = p @ np.linalg.qr(r.normal(size=(3, 3)))[0]
    return p + np.asarray(centre)


# ---- hand meshes for the fans (shared with tests/test_gpu_rim.py) --------------------------------------------------------

def strip_mesh(n=4):
    """A ring 0 .. n-1 at z = 0 under a second ring n .. 2n-1: every rim edge has one owner, its apex on the ring above."""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.1
    v = np.concatenate([np.stack([np.cos(t), np.sin(t), 0 * t], 1), np.stack([np.cos(t), np.sin(t), 0 * t + 1], 1)])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, n + i], [j, n + j, n + i]]
    return v, np.array(f, dtype=np.int64)


def ear_mesh():
    """Ring 0, 1, 2, 3; face (0, 1, 2) carries the rim edges 0-1 and 1-2; (0, 2, 3) the edges 2-3 and 3-0."""
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0.5]], dtype=float)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)


HAND_CASES = {
    # name: (mesh, ring, counts)
    "one_rim_edge_per_face": (strip_mesh(4), [0, 1, 2, 3], [1, 0, 2, 0]),
    "two_rim_edges_one_subdivided": (ear_mesh(), [0, 1, 2, 3], [2, 0, 0, 0]),
    "two_subdivided_centroid_fan": (ear_mesh(), [0, 1, 2, 3], [1, 1, 0, 0]),
    "three_subdivided_centroid_fan": ((np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], dtype=float),
                                       np.array([[0, 1, 2]], dtype=np.int64)), [0, 1, 2], [1, 2, 1]),
    "rim_edge_owned_by_two_faces": ((np.array([[0, 0, 0], [2, 0, 0], [1, 2, 0], [1, -2, 0], [5, 5, 5]], dtype=float),
                                     np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int64)), [0, 1, 4], [1, 0, 0]),
    "rim_edge_owned_by_none": ((np.array([[0, 0, 0], [2, 0, 0], [1, 2, 0], [7, 7, 7], [8, 8, 8]], dtype=float),
                                np.array([[0, 1, 2]], dtype=np.int64)), [1, 3, 4], [0, 2, 0]),
    "ring_against_the_winding": (strip_mesh(5), [0, 4, 3, 2, 1], [1, 1, 0, 3, 0]),
}


class TestPlaneFit:
    @pytest.mark.parametrize("ring", [irregular_ring(40, 1), irregular_ring(17, 2, noise=0.0),
                                      np.array([[0, 0, 0], [4, 0, 1], [1, 3, 0]], dtype=float)],
                             ids=["tilted_noisy_ellipse", "exactly_planar", "three_points"])
    def test_normal_and_projection(self, ring):
        assert K.singular_gap(ring) >= 0.1
        o, n = ccta.fit_ring_plane(ring)
        kn = K.plane_normal_svd(ring)
        assert abs(np.linalg.norm(n) - 1) < 1e-15 and n[np.argmax(np.abs(n))] > 0
        assert np.abs(n - np.sign(n @ kn) * kn).max() < 1e-12              # to rounding, up to LAPACK's sign
        assert np.abs(o - ring.mean(axis=0)).max() < 1e-12
        got, want = ccta.project_to_best_fit_plane(ring), K.project_to_best_fit_plane(ring)
        assert np.abs(got - want).max() < TOL
        assert np.abs((got - o) @ n).max() < 1e-12

    def test_pass_through_and_degenerate(self):
        two = np.array([[1.0, 2, 3], [4, 5, -0.0]])
        assert same_bits(ccta.project_to_best_fit_plane(two), two) and same_bits(K.project_to_best_fit_plane(two), two)
        same = np.tile([[3.0, -1.0, 2.5]], (6, 1))
        assert same_bits(ccta.project_to_best_fit_plane(same), same)      # every distance is 0, whatever the normal
        assert np.isfinite(ccta.fit_ring_plane(same)[1]).all()

    def test_given_plane(self):
        ring = irregular_ring(12, 3)
        o, n = np.array([99.0, -50, 31]), np.array([0.6, 0.0, 0.8])
        assert np.abs(ccta.project_to_best_fit_plane(ring, o, n) - K.project_onto_plane(ring, o, n)).max() < 1e-12


class TestSmoothing:
    @pytest.mark.parametrize("n", [5, 17, 100])
    def test_keeps_the_calibre(self, n):
        ring = K.project_to_best_fit_plane(irregular_ring(n, 10 + n))
        got = ccta.smooth_ring_preserving_size(ring)
        assert np.abs(got - K.smooth_ring_preserving_size(ring)).max() < TOL
        assert abs(K.ring_calibre(got) / K.ring_calibre(ring) - 1) < 1e-12
        plain = K.smooth_ring_laplacian(ring)
        assert K.ring_calibre(plain) < K.ring_calibre(ring)               # the plain smoother does shrink it

    def test_zero_calibre_fallbacks(self):
        same = np.tile([[3.0, -1.0, 2.5]], (7, 1))                        # before == 0
        assert same_bits(ccta.smooth_ring_preserving_size(same), K.smooth_ring_preserving_size(same))
        assert same_bits(ccta.smooth_ring_preserving_size(same), same)
        sq = np.array([[1.0, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])  # alpha = 0: every point to the centre: after == 0
        got, want = ccta.smooth_ring_preserving_size(sq, 1, 0.0), K.smooth_ring_preserving_size(sq, 1, 0.0)
        assert same_bits(got, want) and K.ring_calibre(got) == 0.0
        two = sq[:2]
        assert same_bits(ccta.smooth_ring_preserving_size(two), two)


class TestRespacing:
    @pytest.mark.parametrize("n_out", [None, 9, 17, 40])
    def test_against_the_checker(self, n_out):
        ring = K.project_to_best_fit_plane(irregular_ring(17, 5))
        got, want = ccta.redistribute_ring_evenly(ring, n_out), K.redistribute_ring_evenly(ring, n_out)
        assert same_bits(got, want)                                       # same input, same operations: the same bits
        assert same_bits(got[0], ring[0]) and len(got) == (17 if n_out is None else n_out)

    def test_zero_length_segment_zero_perimeter_and_short(self):
        ring = irregular_ring(8, 6)
        ring[3] = ring[2]
        ring[1] = ring[0]                                                 # the first segment has no length
        for n_out in (None, 5, 20):
            assert same_bits(ccta.redistribute_ring_evenly(ring, n_out), K.redistribute_ring_evenly(ring, n_out))
        same = np.tile([[1.0, 2.0, 3.0]], (5, 1))
        assert same_bits(ccta.redistribute_ring_evenly(same, 9), same) and same_bits(K.redistribute_ring_evenly(same, 9), same)
        assert same_bits(ccta.redistribute_ring_evenly(ring, 2), ring) and same_bits(ccta.redistribute_ring_evenly(ring[:2], 7), ring[:2])


class TestShiftAndClamp:
    def test_shift(self):
        ring = irregular_ring(20, 7, tilt=False)
        o, n = ring.mean(axis=0), np.array([0.0, 0.0, 2.0])
        behind = ring - [0, 0, 3.0]
        so, sn, moved = ccta.shift_plane_clear_of(o, n, behind, [0, 0, 1.0], 0.5)
        assert moved == 0.0 and same_bits(so, o) and sn.tolist() == [0.0, 0.0, 1.0]
        cutting = ring + [0, 0, 0.4]
        for outward in ([0, 0, 1.0], [0, 0, -1.0]):                       # a normal against `outward` is flipped
            got, want = ccta.shift_plane_clear_of(o, n, cutting, outward, 0.5), K.shift_plane_clear_of(o, n, cutting, outward, 0.5)
            assert got[2] > 0 and abs(got[2] - want[2]) < 1e-12 and np.abs(got[0] - want[0]).max() < 1e-12
            assert got[1].tolist() == want[1].tolist() == [0.0, 0.0, float(np.sign(outward[2]))]
            assert (((cutting - got[0]) @ got[1]) <= -0.5 + 1e-12).all()

    @pytest.mark.parametrize("n", [8, 9])
    @pytest.mark.parametrize("overshoot", [0.0, 0.5])
    def test_clamp(self, n, overshoot):
        r = np.random.default_rng(n)
        ring = np.stack([r.normal(size=n), r.normal(size=n), r.uniform(0.1, 2.0, size=n)], 1)
        ring[1, 2] = -0.7                                                 # on the wrong side
        ring[2, 2] = 0.0                                                  # exactly on the plane: not "wrong"
        o, nr = np.zeros(3), np.array([0.0, 0.0, 1.0])
        got, want = ccta.clamp_to_plane(ring, o, nr, overshoot), K.clamp_to_plane(ring, o, nr, overshoot)
        assert same_bits(got, want)
        assert got[1, 2] == overshoot and got[2, 2] == overshoot and (got[:, 2] >= overshoot).all()
        assert same_bits(got[:, :2], ring[:, :2])
        flipped = ccta.clamp_to_plane(ring, o, -nr, overshoot)            # the normal's sign does not matter
        assert same_bits(flipped, got)

    def test_clamp_even_median_between_the_sides(self):
        ring = np.array([[0, 0, -1.0], [1, 0, -2.0], [0, 1, 1.0], [1, 1, 4.0]])       # median (-1 + 1) / 2 = 0: sign 0
        o, nr = np.zeros(3), np.array([0.0, 0.0, 1.0])
        assert same_bits(ccta.clamp_to_plane(ring, o, nr, 0.5), K.clamp_to_plane(ring, o, nr, 0.5))


class TestDensifyPlan:
    @pytest.mark.parametrize("target", [10, 21, 34, 37, 17, 16, 3])     # extra < n, == n, 2n + 3, ..., <= n
    def test_counts(self, target):
        ring = irregular_ring(17, 8)
        want, status, gap = K.densify_plan(ring, target)
        assert gap >= 1e-6
        got, st = ccta.densify_plan(ring, target)
        assert got.tolist() == want and st == status
        assert sum(want) == max(0, target - 17) and st == (1 if target > 17 else (0 if target == 17 else 2))

    def test_ties_keep_ring_order(self):
        sq = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
        assert ccta.densify_plan(sq, 6)[0].tolist() == [1, 1, 0, 0] == K.densify_plan(sq, 6)[0]


class TestFansOnHandMeshes:
    def test_one_rim_edge_per_face(self):
        mesh, ring, counts = HAND_CASES["one_rim_edge_per_face"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info == {"n_inserted": 3, "n_fanned_faces": 2, "n_centroid_fans": 0}
        assert dense == [0, 8, 1, 2, 9, 10, 3]
        # untouched faces in input order, then the fans of face 0 (0, 1, 4) and face 4 (2, 3, 6) about their apex
        assert f.tolist() == [[1, 5, 4], [1, 2, 5], [2, 6, 5], [3, 7, 6], [3, 0, 7], [0, 4, 7],
                              [4, 0, 8], [4, 8, 1], [6, 2, 9], [6, 9, 10], [6, 10, 3]]
        assert same_bits(v[8], mesh[0][0] + 0.5 * (mesh[0][1] - mesh[0][0])) and same_bits(v[:8], mesh[0])

    def test_two_rim_edges_one_subdivided_has_an_apex(self):
        mesh, ring, counts = HAND_CASES["two_rim_edges_one_subdivided"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info["n_centroid_fans"] == 0 and f.tolist() == [[0, 2, 3], [2, 0, 4], [2, 4, 5], [2, 5, 1]]

    def test_centroid_fans(self):
        mesh, ring, counts = HAND_CASES["two_subdivided_centroid_fan"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info == {"n_inserted": 2, "n_fanned_faces": 1, "n_centroid_fans": 1} and len(v) == 7
        assert f.tolist() == [[0, 2, 3], [6, 0, 4], [6, 4, 1], [6, 1, 5], [6, 5, 2], [6, 2, 0]]
        assert np.allclose(v[6], v[[0, 4, 1, 5, 2]].mean(axis=0), atol=1e-15)
        mesh, ring, counts = HAND_CASES["three_subdivided_centroid_fan"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info["n_centroid_fans"] == 1 and len(f) == 7 and dense == [0, 3, 1, 4, 5, 2, 6] and (f[:, 0] == 7).all()

    def test_owned_by_two_and_by_none(self):
        mesh, ring, counts = HAND_CASES["rim_edge_owned_by_two_faces"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info["n_fanned_faces"] == 2 and f.tolist() == [[2, 0, 5], [2, 5, 1], [3, 1, 5], [3, 5, 0]]
        mesh, ring, counts = HAND_CASES["rim_edge_owned_by_none"]
        (v, f), dense, info = K.split_rim_edges(mesh, ring, counts)
        assert info["n_fanned_faces"] == 0 and f.tolist() == mesh[1].tolist() and len(v) == 7 and dense == [1, 3, 5, 6, 4]

    def test_checker_densify_boundary_closes_the_ring(self):
        mesh = strip_mesh(7)
        ring = mesh[0][:7]
        for target in (8, 14, 30):
            (v, f), dense, info = K.densify_boundary(mesh, ring, target)
            assert len(dense) == target and info["n_inserted"] == target - 7 and info["n_fanned_faces"] == min(7, target - 7)
        assert K.densify_boundary(mesh, ring, 5)[2]["over_target"] == 1
        assert K.densify_boundary(mesh, ring + 1e-3, 9)[2]["off_mesh"] == 1


class TestRejections:
    def test_nulls_negative_sizes_and_nan(self):
        L = N.lib()
        ring = irregular_ring(6, 9)
        out = np.zeros((8, 3))
        o, n = np.zeros(3), np.array([0.0, 0, 1])
        cnt = np.zeros(8, dtype=np.int64)
        p = N._ptr
        assert L.mm_ring_fit_plane(None, 6, p(o), p(n)) == -2 and L.mm_ring_fit_plane(p(ring), 0, p(o), p(n)) == -2
        assert L.mm_ring_project_to_plane(None, 6, None, None, p(out)) == -2
        assert L.mm_ring_project_to_plane(p(ring), -1, None, None, p(out)) == -2
        assert L.mm_ring_project_to_plane(p(ring), 6, p(o), None, p(out)) == -2
        assert L.mm_ring_smooth_preserving_size(p(ring), 6, -1, 0.5, p(out)) == -2
        assert L.mm_ring_smooth_preserving_size(p(ring), 6, 5, 0.5, None) == -2
        assert L.mm_ring_redistribute(p(ring), 6, -2, p(out)) == -2 and L.mm_ring_redistribute(None, 6, 6, p(out)) == -2
        m = C.c_double()
        assert L.mm_plane_shift_clear_of(p(o), p(n), p(ring), 0, p(n), 0.5, p(o), p(n), C.byref(m)) == -2
        assert L.mm_plane_shift_clear_of(p(o), p(o), p(ring), 6, p(n), 0.5, p(o), p(n), C.byref(m)) == -2     # zero normal
        assert L.mm_ring_clamp_to_plane(p(ring), 6, None, p(n), 0.5, p(out)) == -2
        assert L.mm_ring_densify_plan(p(ring), 6, -1, p(cnt)) == -2 and L.mm_ring_densify_plan(p(ring), 6, 9, None) == -2
        bad = ring.copy()
        bad[2, 1] = np.nan
        for call in (lambda: ccta.fit_ring_plane(bad), lambda: ccta.project_to_best_fit_plane(bad),
                     lambda: ccta.smooth_ring_preserving_size(bad), lambda: ccta.redistribute_ring_evenly(bad),
                     lambda: ccta.clamp_to_plane(bad, o, n, 0.5), lambda: ccta.densify_plan(bad, 9),
                     lambda: ccta.shift_plane_clear_of(o, n, bad, n, 0.5)):
            with pytest.raises(ValueError):
                call()
        assert "mm_ring" in N.last_error() or "mm_plane" in N.last_error()

    def test_repeated_ring_vertex(self):
        mesh = strip_mesh(4)
        with pytest.raises(ValueError, match="twice"):
            K.split_rim_edges(mesh, [0, 1, 2, 1], [1, 0, 0, 0])
        with pytest.raises(ValueError, match="different targets"):
            K.write_ring_to_mesh(mesh, [mesh[0][0], mesh[0][0]], [[1.0, 2, 3], [1.0, 2, 4]])


def test_public_names_exist():
    for name in ("condition_boundary_rings", "stitch_conditioned"):
        assert callable(getattr(mm, name)) and name in mm.__all__
    for name in ("project_to_best_fit_plane", "smooth_ring_preserving_size", "redistribute_ring_evenly",
                 "shift_plane_clear_of", "clamp_to_plane", "write_ring_to_mesh", "enforce_layer_gap_from_plane",
                 "densify_boundary", "condition_boundary_rings", "stitch_conditioned", "locate_points", "split_rim_edges"):
        assert callable(getattr(ccta, name)), name
    for name in ("mm_ring_fit_plane", "mm_ring_project_to_plane", "mm_ring_smooth_preserving_size", "mm_ring_redistribute",
                 "mm_plane_shift_clear_of", "mm_ring_clamp_to_plane", "mm_ring_densify_plan", "mm_mesh_locate_points",
                 "mm_mesh_layer_push", "mm_mesh_split_rim_edges", "mm_condition_rims"):
        assert name in N.EXPORTS_CCTA and hasattr(N.lib(), name)
    assert C.sizeof(N.MMRimReport) == 23 * 8 and C.sizeof(N.MMRimParams) == 11 * 8
