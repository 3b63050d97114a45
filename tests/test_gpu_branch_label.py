"""CCTA branch labelling on the device: the branch masks of csrc/mm_branch_kernels.hip against the checker
(tests/mm_checkers/centerline_prep.py) exactly, at sizes around the block and the LDS tile and at the boundary of the
radius; label_branches, list by list and in order, against the route it replaces (one find_centerline_bounded_points_simple
call per branch and the set logic of labeling.py:453-487); and the chain prepare_centerline -> label_branches_pair ->
discretize_vessel_tree -> get_summary on a synthetic tree, with no key written by hand."""
import numpy as np
import pytest

from mm_checkers import centerline_prep as K

import multimoda_rs_amd as mm
from multimoda_rs_amd.centerline import CL_DTYPE, Centerline

pytestmark = pytest.mark.gpu
N = mm._native


def make_cl(xyz, branch_id):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return Centerline.from_arrays(xyz, np.zeros_like(xyz), branch_id=np.asarray(branch_id, dtype=np.uint32))


def random_case(seed, n, m, n_branches, box=10.0):
    r = np.random.default_rng(seed)
    c = r.uniform(-box, box, (m, 3))
    b = r.integers(0, n_branches, m)
    b[:min(n_branches, m)] = np.arange(min(n_branches, m))                  # every branch has a point
    return make_cl(c, b), c, b, r.uniform(-box, box, (n, 3))


def tile():
    return int(N.lib().mm_branch_tile_points())


@pytest.mark.parametrize("n_branches", [1, 2, 64])
@pytest.mark.parametrize("m_kind", ["below", "above"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_masks_equal_the_checker(engine, n, m_kind, n_branches):
    m = tile() // 2 - 3 if m_kind == "below" else 2 * tile() + 37           # inside one LDS tile / two full tiles and a rest
    cl, c, b, pts = random_case(n + 7 * n_branches + (m_kind == "above"), n, m, n_branches)
    got = mm.branch_masks(cl, pts, 1.5, engine=engine)
    want = K.branch_masks(c, b, pts, 1.5)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    if n >= 63:
        assert want.any() and not want.all()                                # the case decides something


def test_tile_boundaries_and_single_points(engine):
    t = tile()
    for m in (1, t - 1, t, t + 1, 2 * t):
        cl, c, b, pts = random_case(m, 300, m, 5, box=4.0)
        assert np.array_equal(mm.branch_masks(cl, pts, 1.0, engine=engine), K.branch_masks(c, b, pts, 1.0)), m


def test_more_than_64_branches_is_an_error(engine):
    cl, c, b, pts = random_case(3, 100, 200, 64)
    cl.points["branch_id"][17] = 64
    with pytest.raises(RuntimeError, match="64"):
        mm.branch_masks(cl, pts, 1.5, engine=engine)
    with pytest.raises(RuntimeError, match="64"):
        mm.label_branches(cl, {"rca_points": pts}, engine=engine)
    with pytest.raises(ValueError):
        mm.branch_masks(cl, np.zeros((0, 3)), 1.5, engine=engine)
    with pytest.raises(ValueError):
        mm.branch_masks(Centerline(np.zeros(0, dtype=CL_DTYPE)), pts, 1.5, engine=engine)


# offsets whose squared length is an exact square in f64: |d|^2 = r^2 with no rounding anywhere
EXACT = [((3.0, 4.0, 0.0), 5.0), ((0.0, -3.0, 4.0), 5.0), ((-5.0, 0.0, 0.0), 5.0), ((2.0, 3.0, 6.0), 7.0),
         ((-6.0, 2.0, -3.0), 7.0), ((1.0, 4.0, 8.0), 9.0), ((-8.0, -4.0, 1.0), 9.0), ((0.375, 0.5, 0.0), 0.625)]


@pytest.mark.parametrize("shift", [0.0, 16.0])
def test_radius_boundary_is_inside_and_the_next_float_is_outside(engine, shift):
    for off, r in EXACT:
        # the centerline point: the origin, or 16 away on the offset's own side of every axis, so that the mesh point's
        # coordinates are the coarser ones and their last bit survives the subtraction
        c0 = shift * np.where(np.array(off) < 0.0, -1.0, 1.0)
        on = c0 + np.array(off)
        assert np.array_equal(on - c0, np.array(off))                       # the offset is recovered exactly
        a = int(np.argmax(np.abs(off)))                                     # the axis whose last bit weighs most in |d|^2
        out, inw = on.copy(), on.copy()
        out[a] = np.nextafter(on[a], np.inf if off[a] > 0 else -np.inf)     # the next representable coordinate outwards
        inw[a] = np.nextafter(on[a], c0[a])
        others = []
        for k in range(3):              # a last-bit step along a minor axis may vanish in the rounding of the sum: whatever
            if k != a and off[k] != 0.0:                                    # f64 makes of it, the kernel makes the same
                q = on.copy()
                q[k] = np.nextafter(on[k], np.inf if off[k] > 0 else -np.inf)
                others.append(q)
        pts = np.array([on, out, inw] + others)
        cl = make_cl([c0, c0 + 100.0], [0, 1])
        want = K.branch_masks([c0, c0 + 100.0], [0, 1], pts, r)
        assert want[:3].tolist() == [1, 0, 1], (off, r)                     # the construction is what it claims to be
        assert np.array_equal(mm.branch_masks(cl, pts, r, engine=engine), want), (off, r)
        inside = mm.find_centerline_bounded_points_simple(cl.get_branch(0), pts, r, engine=engine)
        assert np.array_equal(inside, pts[want == 1])                       # the existing entry point draws the same line


def test_nan_points_are_near_nothing(engine):
    cl, c, b, pts = random_case(11, 500, 300, 4, box=3.0)
    pts[[0, 77, 499], [0, 1, 2]] = np.nan
    got = mm.branch_masks(cl, pts, 2.0, engine=engine)
    assert np.array_equal(got, K.branch_masks(c, b, pts, 2.0)) and not got[[0, 77, 499]].any()


# ---- label_branches against the route it replaces ---------------------------------------------------------------------------

def line_pts(a, b, n):
    return np.linspace(np.array(a, dtype=float), np.array(b, dtype=float), n)


def four_branch_centerline():
    """main along x; side 1 up from x = 10; sides 2 and 3 up from x = 20 and x = 24, 4 mm apart"""
    parts = [line_pts((0, 0, 0), (40, 0, 0), 81), line_pts((10, 0.5, 0), (10, 18, 0), 36),
             line_pts((20, 0.5, 0), (20, 15, 0), 30), line_pts((24, 0.5, 0), (24, 12, 0), 24)]
    return make_cl(np.concatenate(parts), np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)]))


def mesh_points(seed, n=6000):
    r = np.random.default_rng(seed)
    pts = np.concatenate([r.uniform((-3, -4, -4), (43, 22, 4), (n, 3)),
                          [(22.0, 10.0, 0.0)],                              # 2 mm from side 2 and from side 3, 10 from the main
                          [(60.0, 60.0, 60.0)]])                            # near nothing
    pts = np.concatenate([pts, pts[5:400:7], pts[5:400:7]])                 # duplicated vertices, some three times
    return pts[r.permutation(len(pts))]


def parent_route(cl, results, key, branch_id, radius, engine):
    """labeling.py:453-487 with the entry point that exists without this feature: B + 1 searches and host set logic"""
    find = mm.find_centerline_bounded_points_simple
    pts = np.asarray(results[key], dtype=np.float64).reshape(-1, 3)
    ids = [branch_id] if isinstance(branch_id, int) else list(branch_id)
    main_set = set()
    for b in ids:
        main_set.update(map(tuple, find(cl.get_branch(b), pts, radius, engine=engine)))
    in_main = np.array([tuple(p) in main_set for p in pts], dtype=bool)
    out = {f"{key}_main": pts[in_main], f"{key}_side": pts[~in_main]}
    for k in range(len(cl.branch_start_indices)):
        if k not in set(ids):
            out[f"{key}_side_{k}"] = find(cl.get_branch(k), out[f"{key}_side"], radius, engine=engine)
    return out


@pytest.mark.parametrize("branch_id", [0, [0], [0, 1], [2, 0], 3])
@pytest.mark.parametrize("radius", [3.0, 1.25])
def test_label_branches_equals_the_per_branch_route(engine, branch_id, radius):
    cl = four_branch_centerline()
    pts = mesh_points(5)
    res = {"lca_points": pts, "other": 1}
    got = mm.label_branches(cl, res, results_key="lca_points", branch_id=branch_id, bounding_sphere_radius_mm=radius,
                            engine=engine)
    want = parent_route(cl, {"lca_points": pts}, "lca_points", branch_id, radius, engine)
    assert got is res and set(got) == set(want) | {"lca_points", "other"}
    for k, v in want.items():
        assert got[k].shape == v.shape and np.array_equal(got[k].view(np.uint64), v.view(np.uint64)), k
    if branch_id == 0 and radius == 3.0:
        both = np.array([22.0, 10.0, 0.0])
        for k in (2, 3):                                                    # the point between two side branches is in both
            assert (got[f"lca_points_side_{k}"] == both).all(axis=1).any()
        assert not (got["lca_points_side_1"] == both).all(axis=1).any()
        assert len(got["lca_points_main"]) + len(got["lca_points_side"]) == len(pts)        # duplicates kept
        assert len(np.unique(pts, axis=0)) < len(pts)


def test_label_branches_errors_follow_the_reference(engine):
    cl = four_branch_centerline()
    with pytest.raises(ValueError):
        mm.label_branches(cl, {"rca_points": np.zeros((0, 3))}, engine=engine)              # an empty point list
    with pytest.raises(ValueError, match="not found"):
        mm.label_branches(cl, {"rca_points": mesh_points(1, 50)}, branch_id=9, engine=engine)
    near_main = np.array([(5.0, 0.5, 0.0), (30.0, -1.0, 0.5)])
    res = {"rca_points": near_main}
    with pytest.raises(ValueError):                                         # nothing is left for the side branches
        mm.label_branches(cl, res, engine=engine)
    assert len(res["rca_points_main"]) == 2 and len(res["rca_points_side"]) == 0 and "rca_points_side_1" not in res
    one = make_cl(line_pts((0, 0, 0), (40, 0, 0), 81), np.zeros(81))
    res = mm.label_branches(one, {"rca_points": near_main}, engine=engine)  # no side branch: no search on the remainder
    assert len(res["rca_points_main"]) == 2 and len(res["rca_points_side"]) == 0


# ---- the missing link: prepared centerlines -> branch labels -> discretised tree -> morphometry ----------------------------

def tube(path, radius, n_ring=28):
    """vertices on rings around a polyline"""
    path = np.asarray(path, dtype=np.float64)
    t = np.gradient(path, axis=0)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    u = np.cross(t, [0.31, 0.2, 0.93])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(t, u)
    a = np.linspace(0, 2 * np.pi, n_ring, endpoint=False)
    return (path[:, None] + radius * (np.cos(a)[None, :, None] * u[:, None] + np.sin(a)[None, :, None] * v[:, None])).reshape(-1, 3)


def y_vessel(origin, direction, side_dir, sign):
    """A main vessel leaving `origin` and one side branch leaving it 20 mm on, as polylines 0.4 mm apart."""
    d, s = np.array(direction, dtype=float), np.array(side_dir, dtype=float)
    d, s = d / np.linalg.norm(d), s / np.linalg.norm(s)
    k = np.arange(0, 45.0, 0.4)
    main = np.array(origin) + k[:, None] * d + (0.004 * k ** 2)[:, None] * np.array([0.0, 0.0, -1.0]) * sign
    j = int(20.0 / 0.4)
    ks = np.arange(0.4, 16.0, 0.4)                                          # shorter than the stretch before it: the main stays the longest path
    side = main[j] + ks[:, None] * s
    return main, side


def test_prepared_centerlines_feed_the_tree_discretisation(engine):
    ao_path = np.stack([np.zeros(100), np.zeros(100), np.linspace(0.0, 60.0, 100)], 1)          # written bottom-up
    rca_main, rca_side = y_vessel((14.0, 0.0, 40.0), (1.0, 0.1, -0.2), (0.3, 1.0, -0.1), 1.0)
    lca_main, lca_side = y_vessel((-14.0, 0.0, 42.0), (-1.0, -0.1, -0.2), (-0.3, -1.0, -0.2), 1.0)
    # the coronaries as a CSV export writes them: far end first, the side branch after a jump
    rca_raw = np.concatenate([rca_main[::-1], rca_side])
    lca_raw = np.concatenate([lca_side[::-1], lca_main])
    step = 1.0
    ao_cl = mm.prepare_centerline(mm.load_centerline(ao_path, "Aorta"))
    rca_cl = mm.prepare_centerline(mm.load_centerline(rca_raw, "RCA"), ref_centerline=ao_cl, spacing_mm=0.5)
    lca_cl = mm.prepare_centerline(mm.load_centerline(lca_raw, "LCA"), ref_centerline=ao_cl, spacing_mm=0.5)
    assert ao_cl.xyz()[0][2] == 60.0                                        # the aorta now starts at its highest point
    for cl, main, side in ((rca_cl, rca_main, rca_side), (lca_cl, lca_main, lca_side)):
        assert len(cl.branch_start_indices) == 2
        b0, b1 = cl.get_branch(0).xyz(), cl.get_branch(1).xyz()
        assert np.linalg.norm(b0[0] - main[0]) < 0.5 and np.linalg.norm(b0[-1] - main[-1]) < 0.5     # starts at the aorta
        assert np.linalg.norm(b1[-1] - side[-1]) < 0.5 and np.linalg.norm(b1[0] - main[50]) < 1.5    # starts at the junction
    results = {"aorta_points": tube(ao_path, 13.0, 60), "rca_removed_points": np.zeros((0, 3)),
               "rca_points": np.concatenate([tube(rca_main, 1.8), tube(rca_side[4:], 1.2)]),
               "lca_points": np.concatenate([tube(lca_main, 1.9), tube(lca_side[4:], 1.1)]),
               "lca_removed_points": np.zeros((0, 3))}
    given_keys = set(results)
    results = mm.label_branches_pair(rca_cl, lca_cl, results, engine=engine)
    assert set(results) - given_keys == {f"{v}_points_{s}" for v in ("rca", "lca") for s in ("main", "side", "side_1")}
    tree = mm.discretize_vessel_tree(ao_cl, rca_cl, lca_cl, results, step_size=step, n_points=60, engine=engine)
    assert len(tree.discretized_aorta) > 20 and len(tree.discretized_rca_main) > 20 and len(tree.discretized_lca_main) > 20
    assert len(tree.rca_branches) == 1 and len(tree.lca_branches) == 1
    for contours, cl in ((tree.rca_branches[0], rca_cl), (tree.lca_branches[0], lca_cl)):
        assert len(contours) >= 10
        line = cl.get_branch(1).xyz()
        for c in contours:
            far = float(np.min(np.linalg.norm(line - np.asarray(c.centroid), axis=1)))
            ring = float(np.min(np.linalg.norm(line - c.points.mean(axis=0), axis=1)))
            print(f"side contour {c.id}: centroid {far:.3f} mm, mean of its points {ring:.3f} mm from the branch")
            assert far <= step
    summary = tree.get_summary(engine=engine)
    assert len(summary["rca_branches"]) == 1 and len(summary["lca_branches"]) == 1
    for name, r in (("rca_main", 1.8), ("lca_main", 1.9)):                  # a tube of radius r: its smallest slice is about pi r^2
        (mla, _, _), table = summary[name]
        assert len(table) > 20 and 0.5 * np.pi * r * r < mla < 1.5 * np.pi * r * r
    for name in ("rca_branches", "lca_branches"):                           # (their first slices are cut by the main vessel's share)
        (mla, _, _), table = summary[name][0]
        assert len(table) >= 10 and np.isfinite(mla) and mla > 0.0
