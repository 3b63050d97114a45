"""CCTA vessel discretisation on the device, bit for bit against the numpy checker (tests/mm_checkers/discretize.py):
the nearest-anchor pass (csrc/mm_slice_kernels.hip) with its tie and NaN rules, discretize_vessel on curved and
multi-branch centerlines and their edge cases, the batched tree against jobs run one by one, and discretize_vessel_tree
end to end on the output of label_geometry."""
import numpy as np
import pytest

from mm_checkers import discretize as DZ

import multimoda_rs_amd as mm
from multimoda_rs_amd.centerline import Centerline

pytestmark = pytest.mark.gpu
N = mm._native


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    """Bit for bit, except that a NaN only has to be a NaN: its sign and payload are the hardware's (IEEE 754 leaves
    them open; x86 makes a negative default NaN, the GPU a positive one)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def device_nearest(engine, jobs):
    """jobs: [(points (n, 3), anchors (m, 6))] -> [(idx, proj)]"""
    pts = [DZ.p3(p) for p, _ in jobs]
    anc = [np.asarray(a, dtype=np.float64).reshape(-1, 6) for _, a in jobs]
    pt_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int64)
    a_off = np.concatenate([[0], np.cumsum([a.shape[0] for a in anc])]).astype(np.int64)
    xyz, A = np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(anc))
    idx = np.zeros(int(pt_off[-1]), dtype=np.int32)
    proj = np.zeros((int(pt_off[-1]), 3))
    N.check(N.lib().mm_nearest_anchor_project(engine.handle, len(jobs), N._ptr(pt_off), N._ptr(xyz), N._ptr(a_off),
                                              N._ptr(A), N._ptr(idx), N._ptr(proj)), "nearest")
    return [(idx[pt_off[j]:pt_off[j + 1]], proj[pt_off[j]:pt_off[j + 1]]) for j in range(len(jobs))]


def assert_nearest(engine, jobs):
    for (p, a), (gi, gq) in zip(jobs, device_nearest(engine, jobs)):
        wi, wq = DZ.nearest_project(p, a)
        assert np.array_equal(gi, wi)
        assert same(gq, wq)


def curved_tube(seed, n_cl=40, n_ring=24, radius=2.0, branches=1):
    """A random smooth centerline per branch (tangents: normalised differences) and a noisy tube around it."""
    r = np.random.default_rng(seed)
    xyz, tan, bid, pts = [], [], [], []
    for b in range(branches):
        s = np.linspace(0, 1, n_cl)
        c = np.stack([10 * b + 8 * np.sin(2 * s + r.uniform(0, 3)), 5 * np.cos(3 * s + r.uniform(0, 3)), 40 * s + 3 * b], 1)
        t = np.gradient(c, axis=0)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        u = np.cross(t, [0.3, 0.2, 0.9])
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        v = np.cross(t, u)
        a = r.uniform(0, 2 * np.pi, (n_cl, n_ring))
        rr = radius + r.normal(0, 0.1, (n_cl, n_ring))
        p = c[:, None] + rr[..., None] * (np.cos(a)[..., None] * u[:, None] + np.sin(a)[..., None] * v[:, None])
        p = p.reshape(-1, 3) + r.normal(0, 0.2, (n_cl * n_ring, 3))
        xyz.append(c), tan.append(t), bid.append(np.full(n_cl, b, dtype=np.uint32)), pts.append(p)
    return np.concatenate(xyz), np.concatenate(tan), np.concatenate(bid), pts


def check_vessel(engine, xyz, tan, bid, pts, branch, step, n_points):
    cl = Centerline.from_arrays(xyz, tan, branch_id=bid)
    got = mm.discretize_vessel(cl, pts, branch, step, n_points, engine=engine)
    want = DZ.discretize_vessel(xyz, tan, bid, pts, branch, step, n_points)
    assert [c.id for c in got] == [w[0] for w in want]
    for c, (cid, cen, wp) in zip(got, want):
        assert c.original_frame == cid and c.kind == "lumen"
        assert np.array_equal(bits(c.centroid), bits(cen))
        assert np.array_equal(bits(c.points), bits(wp))
    return got


@pytest.mark.parametrize("seed,n_pts,n_anc", [(1, 1, 1), (2, 255, 3), (3, 256, 511), (4, 257, 512), (5, 3000, 513),
                                              (6, 20000, 1300)])
def test_nearest_random_matches_checker(engine, seed, n_pts, n_anc):
    r = np.random.default_rng(seed)
    pts = r.uniform(-20, 20, (n_pts, 3))
    anc = np.concatenate([r.uniform(-20, 20, (n_anc, 3)), r.normal(size=(n_anc, 3))], 1)
    assert_nearest(engine, [(pts, anc)])


def test_nearest_ties_go_to_the_lower_index(engine):
    anc = np.array([(0.0, 0.0, float(z), 0.0, 0.0, 1.0) for z in range(10)])
    pts = np.array([(float(x), float(y), z + 0.5) for z in range(-1, 10) for x in (-1.0, 0.0, 2.0) for y in (0.0, 3.0)])
    (gi, _), = device_nearest(engine, [(pts, anc)])
    assert gi.tolist() == [max(int(np.floor(p[2])), 0) for p in pts]
    dup = np.concatenate([anc, anc[::-1]])                         # equal anchors: the first copy wins
    assert_nearest(engine, [(pts, anc), (pts, dup)])


def test_nearest_nan_rules(engine):
    r = np.random.default_rng(9)
    pts = r.uniform(-5, 5, (700, 3))
    pts[[0, 300]] = np.nan
    pts[17, 1] = np.nan
    anc = np.concatenate([r.uniform(-5, 5, (600, 3)), r.normal(size=(600, 3))], 1)
    nan0, nanj = anc.copy(), anc.copy()
    nan0[0, 0] = np.nan                                            # a NaN at anchor 0 pins every point there
    nanj[[5, 513], 2] = np.nan                                     # a NaN later is never chosen
    (g0, _), (gj, _), (gp, _) = device_nearest(engine, [(pts, nan0), (pts, nanj), (pts, anc)])
    assert (g0 == 0).all()
    assert not np.isin(gj, [5, 513]).any()
    assert gp[0] == gp[300] == gp[17] == 0
    assert_nearest(engine, [(pts, nan0), (pts, nanj), (pts, anc)])


def test_nearest_batch_equals_one_by_one(engine):
    r = np.random.default_rng(4)
    jobs = [(r.uniform(-9, 9, (int(r.integers(1, 900)), 3)),
             np.concatenate([r.uniform(-9, 9, (k, 3)), r.normal(size=(k, 3))], 1)) for k in (1, 7, 600, 0, 33)]
    batch = device_nearest(engine, jobs)
    for job, (bi, bq) in zip(jobs, batch):
        (si, sq), = device_nearest(engine, [job])
        assert np.array_equal(bi, si) and same(bq, sq)
    assert (batch[3][0] == -1).all() and np.array_equal(batch[3][1], jobs[3][0])
    assert_nearest(engine, jobs)


@pytest.mark.parametrize("seed,step,n_points", [(11, 0.5, 200), (12, 1.0, 100), (13, 0.37, 50), (14, 2.0, 8)])
def test_discretize_curved_tube_matches_checker(engine, seed, step, n_points):
    xyz, tan, bid, pts = curved_tube(seed)
    got = check_vessel(engine, xyz, tan, bid, pts[0], 0, step, n_points)
    assert len(got) > 5 and all(len(c) == n_points for c in got)


def test_discretize_multi_branch_filters_the_branch(engine):
    xyz, tan, bid, pts = curved_tube(21, branches=3)
    for b in range(3):
        got = check_vessel(engine, xyz, tan, bid, pts[b], b, 0.5, 64)
        assert len(got) > 5
    # points of every branch against one branch's slices: the far ones land in its end slices
    check_vessel(engine, xyz, tan, bid, np.concatenate(pts), 1, 0.5, 64)


def test_discretize_edge_cases(engine):
    xyz, tan, bid, pts = curved_tube(31)
    cl = Centerline.from_arrays(xyz, tan, branch_id=bid)
    assert mm.discretize_vessel(cl, pts[0], 5, 0.5, 50, engine=engine) == []            # absent branch
    assert mm.discretize_vessel(cl, np.zeros((0, 3)), 0, 0.5, 50, engine=engine) == []  # no points
    got = check_vessel(engine, xyz, tan, bid, pts[0], 0, 1000.0, 50)                     # a step longer than the branch
    assert len(got) <= 1
    for step in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            mm.discretize_vessel(cl, pts[0], 0, step, 50, engine=engine)
    with pytest.raises(RuntimeError):
        mm.discretize_vessel(cl, pts[0], 0, 0.5, 1, engine=engine)
    bad = pts[0].copy()
    bad[5] = np.nan                                                # a NaN point: pinned to slice 0, a NaN angle there
    try:
        want = DZ.discretize_vessel(xyz, tan, bid, bad, 0, 0.5, 50)
    except DZ.PanicError:
        with pytest.raises(RuntimeError):
            mm.discretize_vessel(cl, bad, 0, 0.5, 50, engine=engine)
    else:
        got = mm.discretize_vessel(cl, bad, 0, 0.5, 50, engine=engine)
        assert [c.id for c in got] == [w[0] for w in want]


def _tree_cl(xyz, branch_id=None):
    xyz = np.asarray(xyz, dtype=np.float64)
    t = np.gradient(xyz, axis=0)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return Centerline.from_arrays(xyz, t, branch_id=branch_id)


def test_tree_batch_equals_jobs_one_by_one(engine):
    xyz, tan, bid, pts = curved_tube(41, branches=3)
    ao = _tree_cl(curved_tube(42, n_cl=60)[0])
    cor = Centerline.from_arrays(xyz, tan, branch_id=bid)
    ao_pts = curved_tube(42, n_cl=60, radius=6.0)[3][0]
    tree = mm.ccta.discretize_vessel_tree_raw(ao, cor, cor, ao_pts, pts[0], pts[0], [pts[1], pts[2]], [pts[2]],
                                              step_size=0.7, n_points=60, engine=engine)
    one = lambda cl, p, b: mm.discretize_vessel(cl, p, b, 0.7, 60, engine=engine)
    expect = [(tree.discretized_aorta, one(ao, ao_pts, 0)), (tree.discretized_rca_main, one(cor, pts[0], 0)),
              (tree.discretized_lca_main, one(cor, pts[0], 0)), (tree.rca_branches[0], one(cor, pts[1], 1)),
              (tree.rca_branches[1], one(cor, pts[2], 2)), (tree.lca_branches[0], one(cor, pts[2], 1))]
    for got, want in expect:
        assert len(got) == len(want) > 0
        for a, b in zip(got, want):
            assert a.id == b.id and a.centroid == b.centroid and np.array_equal(bits(a.points), bits(b.points))
    assert len(tree.rca_references) >= 1 and tree.spacing == 0.7


@pytest.mark.parametrize("acute", [True, False])
def test_discretize_vessel_tree_end_to_end_on_label_geometry(engine, acute):
    v, f, ca, cr, cl, _ = mm.synth.synthetic_takeoff_mesh(acute_takeoff=acute)
    cla, clr, cll = _tree_cl(ca), _tree_cl(cr), _tree_cl(cl)
    res = mm.label_geometry((v, f), cla, clr, cll, acute_takeoff_rca=acute, control_plot=False, engine=engine)
    rd = dict(res, rca_points_main=res["rca_points"], lca_points_main=res["lca_points"])
    tree = mm.discretize_vessel_tree(cla, clr, cll, rd, step_size=1.0, n_points=100, engine=engine)
    ao_pts = np.concatenate([res["aorta_points"], res["rca_removed_points"]])
    jobs = [(tree.discretized_aorta, cla, ao_pts), (tree.discretized_rca_main, clr, res["rca_points"]),
            (tree.discretized_lca_main, cll, res["lca_points"])]
    for got, c, p in jobs:
        want = DZ.discretize_vessel(c.xyz(), np.stack([c.points["tx"], c.points["ty"], c.points["tz"]], 1),
                                    c.points["branch_id"], p, 0, 1.0, 100)
        assert len(got) == len(want) > 5
        for a, (wid, wcen, wpts) in zip(got, want):
            assert a.id == wid and np.array_equal(bits(a.centroid), bits(wcen)) and np.array_equal(bits(a.points), bits(wpts))
    chk = lambda cs: [(c.id, c.centroid, c.points) for c in cs]
    want = DZ.calculate_ref_pts(chk(tree.discretized_aorta), chk(tree.discretized_rca_main),
                                chk(tree.discretized_lca_main), [], [])
    assert (tree.ao_rca, tree.ao_lca) == want[:2]
    assert [(t.main_ref, t.counter_clock_ref, t.clock_ref) for t in tree.rca_references] == want[2]
    assert [(t.main_ref, t.counter_clock_ref, t.clock_ref) for t in tree.lca_references] == want[3]
    assert tree.rca_branches == [] and tree.lca_branches == [] and len(tree.rca_references) == 1
