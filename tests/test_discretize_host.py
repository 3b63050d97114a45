"""CCTA vessel discretisation, host side (no GPU): the reference's own unit tests of src/ccta/discretizing/projecting.rs
and resampling.rs restated against the numpy checker (tests/mm_checkers/discretize.py), and the host C ABI
(mm_slice_anchor_count, mm_resample_closed_contour) and DiscretizedVesselTree.calculate_ref_pts compared with the checker
bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from mm_checkers import discretize as DZ

import multimoda_rs_amd as mm
from multimoda_rs_amd.centerline import Centerline
from multimoda_rs_amd.frames import Contour

N = mm._native
M64 = (1 << 64) - 1


# ---- fixtures of the reference's tests (projecting.rs:203-290, resampling.rs:232-290) -------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def z_centerline(n):
    xyz = np.array([(0.0, 0.0, float(i)) for i in range(n)])
    return xyz, np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros(n, dtype=np.uint32)


def _lcg(s):
    v = (s * 6364136223846793005 + 1442695040888963407) & M64
    return (v >> 33) / 4294967295.0 - 0.5


def cylinder_ring(z, radius, n, jitter, seed):
    out = []
    for i in range(n):
        a = math.tau * i / n
        s = seed + i
        out.append((radius * math.cos(a) + jitter * _lcg(s), radius * math.sin(a) + jitter * _lcg(s ^ 0xdead),
                    z + jitter * _lcg(s ^ 0xbeef)))
    return out


def project(p, anchor_xyz, n):
    _, q = DZ.nearest_project([p], [tuple(anchor_xyz) + tuple(n)])
    return tuple(q[0])


def plane_dist(p, c, n):
    return ((p[0] - c[0]) * n[0] + (p[1] - c[1]) * n[1]) + (p[2] - c[2]) * n[2]


def walk(cl, cloud, step):
    anc, buckets = DZ.walk_centerline_slices(*cl, cloud, 0, step)
    return anc, buckets


# ---- projecting.rs tests --------------------------------------------------------------------------------------------
def test_projected_point_lies_on_plane():
    q = project((1.5, 2.0, 6.3), (0.0, 0.0, 5.0), (0.0, 0.0, 1.0))
    assert abs(plane_dist(q, (0.0, 0.0, 5.0), (0.0, 0.0, 1.0))) < 1e-10


def test_projection_is_idempotent():
    n = tuple(_unit([1.0, 1.0, 1.0]))
    once = project((4.0, 5.0, 7.0), (1.0, 2.0, 3.0), n)
    twice = project(once, (1.0, 2.0, 3.0), n)
    assert all(abs(a - b) < 1e-10 for a, b in zip(once, twice))


def test_straight_centerline_removes_z_jitter():
    for p in cylinder_ring(0.0, 3.0, 8, 0.5, 42):
        assert abs(project(p, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))[2]) < 1e-10


def test_tilted_normal_projection():
    sq2 = math.sqrt(2.0) / 2.0
    n = tuple(_unit([sq2, 0.0, sq2]))
    for raw in [(1.0, 0.0, 1.0), (-1.0, 0.0, -1.0), (0.0, 2.0, 0.0), (1.0, -1.5, 0.5), (0.5, 0.5, -0.5)]:
        assert abs(plane_dist(project(raw, (0.0, 0.0, 0.0), n), (0.0, 0.0, 0.0), n)) < 1e-10


@pytest.mark.parametrize("n,step,seed_mul,jitter,want", [(5, 1.0, 17, 0.3, 5), (9, 2.0, 7, 0.3, 5), (3, 0.5, 11, 0.1, 5)])
def test_walk_slice_counts(n, step, seed_mul, jitter, want):
    """test_walk_straight_step_equals_spacing / _coarser_step_fewer_slices / _finer_step_more_slices"""
    cloud = [p for i in range(n) for p in cylinder_ring(float(i), 3.0, 8, jitter, i * seed_mul)]
    anc, buckets = walk(z_centerline(n), cloud, step)
    assert len(buckets) == want
    if step >= 1.0:
        assert all(len(b) >= 5 for b in buckets)


def test_projected_points_lie_on_their_anchor_plane():
    cloud = [p for i in range(4) for p in cylinder_ring(float(i), 3.0, 8, 0.3, i * 5)]
    anc, buckets = walk(z_centerline(4), cloud, 1.0)
    for a, b in zip(anc, buckets):
        for p in b:
            assert abs(plane_dist(p, a[0:3], a[3:6])) < 1e-10


def test_voronoi_no_cross_contamination():
    cl = (np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 20.0)]), np.tile([0.0, 0.0, 1.0], (2, 1)), np.zeros(2, dtype=np.uint32))
    cloud = cylinder_ring(0.0, 3.0, 8, 0.1, 1) + cylinder_ring(20.0, 3.0, 8, 0.1, 2)
    anc, buckets = walk(cl, cloud, 20.0)
    assert len(buckets) == 2
    assert all(abs(p[2]) < 1.0 for p in buckets[0]) and all(abs(p[2] - 20.0) < 1.0 for p in buckets[1])


def test_walk_curved_centerline_points_on_planes():
    n, r = 8, 10.0
    ts = [math.pi / 2 * i / (n - 1) for i in range(n)]
    xyz = np.array([(r * math.cos(t), 0.0, r * math.sin(t)) for t in ts])
    tan = np.array([_unit([-math.sin(t), 0.0, math.cos(t)]) for t in ts])
    cloud = [(x + c[0], y + c[1], z + c[2]) for i, c in enumerate(xyz) for (x, y, z) in cylinder_ring(0.0, 2.0, 7, 0.3, i * 31)]
    anc, buckets = walk((xyz, tan, np.zeros(n, dtype=np.uint32)), cloud, 2.0)
    assert len(buckets) == math.floor(math.pi / 2 * r / 2.0) + 1
    for a, b in zip(anc, buckets):
        for p in b:
            assert abs(plane_dist(p, a[0:3], a[3:6])) < 1e-10


# ---- resampling.rs tests --------------------------------------------------------------------------------------------
def circle_ring(c, radius, n):
    return [(c[0] + radius * math.cos(math.tau * i / n), c[1] + radius * math.sin(math.tau * i / n), c[2]) for i in range(n)]


def half_circle_ring(radius, n):
    return [(radius * math.cos(math.pi * i / (n - 1)), radius * math.sin(math.pi * i / (n - 1)), 0.0) for i in range(n)]


O = (0.0, 0.0, 0.0)


def test_coverage_known_answers():
    assert not DZ.has_full_angular_coverage([], O)
    assert not DZ.has_full_angular_coverage(circle_ring(O, 3.0, 3), O)
    assert not DZ.has_full_angular_coverage(half_circle_ring(3.0, 10), O)
    assert DZ.has_full_angular_coverage(circle_ring(O, 3.0, 16), O)
    tilted = [(3.0 * math.cos(math.tau * i / 16), 0.0, 3.0 * math.sin(math.tau * i / 16)) for i in range(16)]
    assert DZ.has_full_angular_coverage(tilted, O)


def test_empty_and_half_circle_contours_removed():
    assert len(DZ.create_uniform_contours([(0, O, []), (1, O, circle_ring(O, 3.0, 16))], 50)) == 1
    assert len(DZ.create_uniform_contours([(0, O, half_circle_ring(3.0, 12)), (1, O, circle_ring(O, 3.0, 16))], 50)) == 1


def test_output_has_exact_n_points_and_metadata():
    for n in (8, 50, 200):
        assert DZ.create_uniform_contours([(0, O, circle_ring(O, 3.0, 20))], n)[0][2].shape == (n, 3)
    out = DZ.create_uniform_contours([(7, (1.0, 2.0, 3.0), circle_ring((1.0, 2.0, 3.0), 3.0, 16))], 50)
    assert out[0][0] == 7 and out[0][1] == (1.0, 2.0, 3.0)


def test_resampled_points_close_to_input_circle_and_on_its_plane():
    out = DZ.create_uniform_contours([(0, O, circle_ring(O, 3.0, 20))], 100)[0][2]
    r = np.sqrt(out[:, 0] ** 2 + out[:, 1] ** 2 + out[:, 2] ** 2)
    assert np.all(np.abs(r - 3.0) < 0.05)
    out = DZ.create_uniform_contours([(0, (0.0, 0.0, 4.0), circle_ring((0.0, 0.0, 4.0), 3.0, 20))], 100)[0][2]
    assert np.all(np.abs(out[:, 2] - 4.0) < 1e-10)


def test_point_indices_are_sequential_through_the_python_contour():
    c = Contour(0, 0, DZ.create_uniform_contours([(0, O, circle_ring(O, 3.0, 16))], 50)[0][2], O)
    assert len(c) == 50 and c.id == 0 and c.kind == "lumen"


def test_multiple_contours_pipeline():
    cs = [(0, O, circle_ring(O, 3.0, 16)), (1, (0.0, 0.0, 1.0), []), (2, (0.0, 0.0, 2.0), circle_ring((0.0, 0.0, 2.0), 3.0, 16)),
          (3, O, half_circle_ring(3.0, 10)), (4, (0.0, 0.0, 4.0), circle_ring((0.0, 0.0, 4.0), 3.0, 16))]
    out = DZ.create_uniform_contours(cs, 100)
    assert [c[0] for c in out] == [0, 2, 3, 4] and all(c[2].shape == (100, 3) for c in out)


# ---- host ABI against the checker -----------------------------------------------------------------------------------
def native_resample(pts, c, n_points):
    p = DZ.p3(pts)
    out = np.zeros((max(n_points, 0), 3))
    cen = np.array(c, dtype=np.float64)
    rc = N.lib().mm_resample_closed_contour(N._ptr(p), p.shape[0], N._ptr(cen), int(n_points), N._ptr(out))
    return rc, out


def _check_resample(pts, c, n_points):
    try:
        want = DZ.resample_spline([tuple(map(float, p)) for p in DZ.p3(pts)], tuple(c), n_points)
    except DZ.PanicError:
        assert native_resample(pts, c, n_points)[0] < 0
        return
    rc, got = native_resample(pts, c, n_points)
    if want is None:
        assert rc == 0
    else:
        assert rc == 1 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_resample_matches_checker_on_random_contours(mm):
    r = np.random.default_rng(11)
    for trial in range(60):
        n = int(r.integers(1, 40))
        c = tuple(r.normal(0, 5, 3))
        nrm = _unit(r.normal(size=3))
        u = _unit(np.cross(nrm, [0.3, 0.5, 0.7]))
        v = np.cross(nrm, u)
        a = r.uniform(0, math.tau, n)
        rad = r.uniform(0.5, 4.0, n)
        pts = np.array(c) + rad[:, None] * (np.cos(a)[:, None] * u + np.sin(a)[:, None] * v) + r.normal(0, 0.05, (n, 1)) * nrm
        if trial % 7 == 3 and n > 2:
            pts[1] = pts[0]                                       # duplicate points: equal angles, the stable sort
        if trial % 7 == 5 and n > 2:
            pts[n // 2] = pts[0]
            a[n // 2] = a[0]
        _check_resample(pts, c, int(r.choice([2, 3, 17, 100, 200])))


def test_resample_degenerate_contours(mm):
    line = [(float(i), 0.0, 0.0) for i in range(6)]
    _check_resample(line, (0.0, 0.0, 0.0), 50)                    # collinear through the centroid: no basis -> 0
    _check_resample(line, (2.5, 1.0, 0.0), 50)                    # collinear, off the centroid: a basis
    _check_resample([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], O, 50)    # fewer than 3 points
    _check_resample([O, O, O, O], O, 50)                          # all at the centroid
    _check_resample(circle_ring(O, 1e-12, 8), O, 50)              # offsets below 1e-10
    _check_resample(circle_ring(O, 3.0, 3), O, 10)
    _check_resample([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (np.nan, 0.0, 0.0)], O, 10)   # NaN angle
    assert native_resample(circle_ring(O, 3.0, 8), O, 1)[0] < 0
    assert native_resample(circle_ring(O, 3.0, 8), O, 0)[0] < 0


def _native_count(xyz, tan, bid, branch, step):
    cl = Centerline.from_arrays(xyz, tan, branch_id=bid)
    return N.lib().mm_slice_anchor_count(N._ptr(cl.points), len(cl), int(branch), float(step))


def test_slice_anchor_count_matches_checker(mm):
    r = np.random.default_rng(5)
    for trial in range(40):
        n = int(r.integers(1, 30))
        xyz = np.cumsum(r.normal(0, 1, (n, 3)), axis=0)
        if trial % 4 == 1 and n > 3:
            xyz[2] = xyz[1]                                        # duplicate centerline points
        if trial % 4 == 2:
            xyz = np.stack([np.zeros(n), np.zeros(n), np.arange(n, dtype=np.float64)], 1)   # integer cum: exact ties
        tan = r.normal(size=(n, 3))
        bid = r.integers(0, 3, n).astype(np.uint32)
        for branch in (0, 1, 2, 7):
            for step in (0.25, 0.5, 1.0, 1.7, 100.0):
                want = DZ.anchors(xyz, tan, bid, branch, step).shape[0]
                assert _native_count(xyz, tan, bid, branch, step) == want


def test_slice_anchor_count_rejects_what_the_reference_cannot_finish(mm):
    xyz, tan, bid = z_centerline(5)
    for step in (0.0, -1.0, float("nan"), float("inf"), 1e-300):
        assert _native_count(xyz, tan, bid, 0, step) < 0, step
    big = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 1e12)])
    assert _native_count(big, np.zeros((2, 3)), np.zeros(2, dtype=np.uint32), 0, 1.0) < 0       # above the cap
    assert _native_count(np.array([(0.0, 0.0, np.nan), (0.0, 0.0, 1.0)]), np.zeros((2, 3)), np.zeros(2, dtype=np.uint32), 0, 1.0) == 0
    assert _native_count(xyz, tan, bid, 3, 1.0) == 0                                           # absent branch
    assert N.lib().mm_slice_anchor_count(None, 0, 0, 1.0) == 0


# ---- calculate_ref_pts ----------------------------------------------------------------------------------------------
def _ring_contours(centres, radius, n_pts, start_id=0, seed=0):
    r = np.random.default_rng(seed)
    out = []
    for k, c in enumerate(centres):
        pts = np.array(circle_ring(tuple(c), radius, n_pts)) + r.normal(0, 0.1, (n_pts, 3))
        out.append(Contour(start_id + k, start_id + k, pts, tuple(float(v) for v in c)))
    return out


def _as_checker(cs):
    return [(c.id, c.centroid, c.points) for c in cs]


def test_calculate_ref_pts_matches_checker():
    r = np.random.default_rng(3)
    for trial in range(8):
        aorta = _ring_contours([(0.0, 0.0, float(z)) for z in range(20)], 12.0, 40, seed=trial)
        rca = _ring_contours([(14.0 + k, 0.5 * k, 10.0 + 0.3 * k) for k in range(15)], 1.5, int(r.integers(3, 30)), seed=trial + 50)
        lca = _ring_contours([(-14.0 - k, 0.2 * k, 6.0) for k in range(12)], 1.5, 24, seed=trial + 90)
        rb = [_ring_contours([(16.0 + k, 3.0 + k, 11.0) for k in range(4)], 1.0, 16, seed=trial + 7), [],
              _ring_contours([(28.0, 7.0 + k, 14.0) for k in range(3)], 1.0, 16, seed=trial + 8)]
        lb = [_ring_contours([(-14.0, -2.0 - k, 6.0) for k in range(3)], 1.0, 16, seed=trial + 9)]
        if trial == 5:
            lca = lca[:1]                                          # a single main contour: normal from the aorta
        tree = mm.DiscretizedVesselTree(aorta, rca, lca, 1.0, rb, lb).calculate_ref_pts()
        want = DZ.calculate_ref_pts(_as_checker(aorta), _as_checker(rca), _as_checker(lca),
                                    [_as_checker(b) for b in rb], [_as_checker(b) for b in lb])
        assert tree.ao_rca == want[0] and tree.ao_lca == want[1]
        got_r = [(t.main_ref, t.counter_clock_ref, t.clock_ref) for t in tree.rca_references]
        got_l = [(t.main_ref, t.counter_clock_ref, t.clock_ref) for t in tree.lca_references]
        assert got_r == want[2] and got_l == want[3]
        assert len(got_r) == 3 and len(got_l) == 2
    empty = mm.DiscretizedVesselTree([], rca, lca, 1.0).calculate_ref_pts()
    assert empty.rca_references == [] and empty.ao_rca == (0.0, 0.0, 0.0)
    assert empty.pts_cusp_rcc is None and empty.index_stj_slice is None and empty.index_aa is None


def test_b_spline_is_not_implemented():
    with pytest.raises(NotImplementedError):
        mm.discretize_vessel_tree(None, None, None, {}, b_spline=True)
