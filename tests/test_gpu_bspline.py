"""mm_bspline_fit_closed_batch (csrc/mm_bspline_kernels.hip) on the GPU against the checker of
tests/mm_checkers/bspline.py, bit for bit, and through it against scipy's recorded fits (tests/golden/bspline)."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multimoda_rs_amd as mm  # noqa: E402
from mm_checkers import bspline as B  # noqa: E402
from test_bspline_host import TOL_S, TOL_S0, extent, fixtures  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_against_checker(new, report, want, tag):
    assert report.code == want["status"] and report.status == B.STATUS_NAMES[want["status"]], (tag, report)
    assert same_bits(new, want["points"]), tag
    assert same_bits(report.fp, want["fp"]) and report.n_knots == want["n_knots"], (tag, report, want["fp"])


def test_every_fixture_matches_the_checker_bit_for_bit(engine):
    by_call = {}
    for c in fixtures():
        by_call.setdefault((c["s"], c["k"]), []).append(c)
    assert mm.ccta.bspline_max_points() == B.MAX_POINTS
    n = 0
    for (s, k), cases in sorted(by_call.items()):
        arrays = [c["in"] for c in cases]
        new, reports = mm.fit_bspline_contours(arrays, s, k, engine=engine)
        from multimoda_rs_amd.ccta import _bspline_batch
        _, cen, _ = _bspline_batch([np.ascontiguousarray(a) for a in arrays], s, k, engine)
        for c, a, r, ce in zip(cases, new, reports, cen):
            check_against_checker(a, r, c["res"], c["id"])
            if c["m"]:
                assert same_bits(ce, np.array(c["res"]["centroid"])), c["id"]
                assert same_bits(ce, [np.mean(np.ascontiguousarray(a[:, d])) for d in range(3)]), c["id"]
            if c["ier"] not in (10, 11):
                d = float(np.abs(a - c["out"]).max()) / extent(c["in"])
                assert d <= (TOL_S0 if s == 0.0 else TOL_S), (c["id"], d)
            n += 1
    assert n == len(fixtures())


def _mixed_batch():
    rng = np.random.default_rng(7)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    out = [np.zeros((0, 3)), np.zeros((0, 3)), rng.normal(size=(2, 3)), rng.normal(size=(3, 3))]
    th = lambda m: np.linspace(0, 2 * np.pi, m, endpoint=False)
    for i in range(290):
        m = int(rng.choice([4, 5, 6, 7, 9, 12, 16, 24, 33]))
        r = 2.0 + 0.1 * rng.normal(size=m)
        out.append(np.stack([r * np.cos(th(m)) + i, 1.2 * r * np.sin(th(m)), 0.05 * rng.normal(size=m)], 1))
    m = B.MAX_POINTS
    r = 2.0 + 0.05 * rng.normal(size=m)
    out.append(np.stack([r * np.cos(th(m)), r * np.sin(th(m)), 0.02 * rng.normal(size=m)], 1))
    for i in range(5):                                   # small enough for the constant to satisfy s: collapsed
        out.append(out[20 + i] * 0.01)
    out.append(out[30] * 1e160)                          # finite, but the squared chord overflows: unchanged
    out.append(out[31] * 1e150)                          # the chord is finite, the residuals overflow
    dup = out[10].copy()
    dup[2] = dup[1]
    bad = out[11].copy()
    bad[0, 0] = np.nan
    out += [dup, bad]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def test_one_batch_equals_one_call_per_contour(engine):
    batch = _mixed_batch()
    assert len(batch) >= 295
    s, k = 0.05, 3
    new, reports = mm.fit_bspline_contours(batch, s, k, engine=engine)
    seen = set()
    for i, (a, n1, r) in enumerate(zip(batch, new, reports)):
        seen.add(r.status)
        one, r1 = mm.fit_bspline_contour(a, s, k, engine=engine)
        assert same_bits(one, n1) and r1 == r, i
        check_against_checker(n1, r, B.fit_closed(a, s, k), i)
        if r.status.startswith("unchanged"):
            assert np.array_equal(n1, a, equal_nan=True) and r.n_knots == 0 and r.fp == 0.0
    assert {"fitted", "collapsed", "unchanged_short", "unchanged_zero_chord", "unchanged_nonfinite"} <= seen


def test_too_many_points_and_bad_degree_raise_and_write_nothing(engine):
    N = mm._native
    m = B.MAX_POINTS + 1
    xyz = np.random.default_rng(1).normal(size=(m + 8, 3))
    off = np.array([0, 8, m + 8], dtype=np.int64)
    out = np.full_like(xyz, 7.0)
    cen, st = np.full((2, 3), 7.0), np.full(2, 7, dtype=np.int32)
    fp, nk = np.full(2, 7.0), np.full(2, 7, dtype=np.int32)

    def call(s, k):
        return N.lib().mm_bspline_fit_closed_batch(engine.handle, 2, N._ptr(xyz), N._ptr(off), s, k, N._ptr(out),
                                                   N._ptr(cen), N._ptr(st), N._ptr(fp), N._ptr(nk))
    assert call(0.1, 3) == -2 and "MM_BSPLINE_MAX_POINTS" in N.last_error()
    assert call(0.1, 0) == -2 and call(0.1, 6) == -2 and call(-1.0, 3) == -2 and call(float("nan"), 3) == -2
    assert (out == 7.0).all() and (cen == 7.0).all() and (st == 7).all() and (fp == 7.0).all() and (nk == 7).all()
    with pytest.raises(RuntimeError):
        mm.fit_bspline_contours([xyz[8:]], 0.1, 3, engine=engine)
    for k in (0, 6):
        with pytest.raises(RuntimeError):
            mm.fit_bspline_contour(xyz[:8], 0.1, k, engine=engine)


@pytest.fixture(scope="module")
def tree_inputs():
    from test_gpu_discretize import _tree_cl, curved_tube
    from multimoda_rs_amd.centerline import Centerline
    xyz, tan, bid, pts = curved_tube(41, branches=2)
    ao = _tree_cl(curved_tube(42, n_cl=60)[0])
    cor = Centerline.from_arrays(xyz, tan, branch_id=bid)
    ao_pts = curved_tube(42, n_cl=60, radius=6.0)[3][0]
    results = {"aorta_points": ao_pts[: len(ao_pts) // 2], "rca_removed_points": ao_pts[len(ao_pts) // 2:],
               "rca_points_main": pts[0], "lca_points_main": pts[0], "rca_points_side_1": pts[1],
               "lca_points_side_1": pts[1]}
    return ao, cor, results


def _groups(tree):
    return ([tree.discretized_aorta, tree.discretized_rca_main, tree.discretized_lca_main] + list(tree.rca_branches) +
            list(tree.lca_branches))


def _raw_tree(tree_inputs, engine):
    ao, cor, results = tree_inputs
    pts_ao = np.concatenate([results["aorta_points"], results["rca_removed_points"]])
    return mm.ccta.discretize_vessel_tree_raw(ao, cor, cor, pts_ao, results["rca_points_main"], results["lca_points_main"],
                                              [results["rca_points_side_1"]], [results["lca_points_side_1"]],
                                              step_size=1.5, n_points=16, calculate_ref_pts=False, engine=engine)


def test_tree_replacement(tree_inputs, engine):
    tree = _raw_tree(tree_inputs, engine)
    before = copy.deepcopy(tree)
    assert all(len(g) > 2 for g in _groups(tree)) and len(tree.rca_branches) == 1 and len(tree.lca_branches) == 1
    s, k = 0.04, 3
    back = mm.replace_contours_with_bsplines(tree, s, k, engine=engine)
    assert back is tree
    want_tree = copy.deepcopy(before)
    statuses = set()
    for g_new, g_old, g_want in zip(_groups(tree), _groups(before), _groups(want_tree)):
        assert len(g_new) == len(g_old)
        for q, (cn, co) in enumerate(zip(g_new, g_old)):
            one, rep = mm.fit_bspline_contour(co, s, k, engine=engine)
            statuses.add(rep.status)
            w = B.fit_closed(co.points, s, k)
            assert same_bits(cn.points, one.points) and same_bits(cn.points, w["points"])
            assert cn.points.shape == co.points.shape == (16, 3)
            assert same_bits(np.array(cn.centroid), np.array(w["centroid"]))
            assert (cn.id, cn.original_frame, cn.kind, cn.aortic_thickness, cn.pulmonary_thickness) == \
                   (co.id, co.original_frame, co.kind, co.aortic_thickness, co.pulmonary_thickness)
            g_want[q] = type(co)(co.id, co.original_frame, w["points"], tuple(w["centroid"]), co.aortic_thickness,
                                 co.pulmonary_thickness, co.kind, co.aortic)
    assert "fitted" in statuses
    tree.calculate_ref_pts()
    want_tree.calculate_ref_pts()
    assert tree.ao_rca == want_tree.ao_rca and tree.ao_lca == want_tree.ao_lca
    assert tree.rca_references == want_tree.rca_references and tree.lca_references == want_tree.lca_references
    assert len(tree.rca_references) >= 1


def test_composite_equals_the_steps_by_hand(tree_inputs, engine):
    ao, cor, results = tree_inputs
    got = mm.discretize_vessel_tree_bspline(ao, cor, cor, results, step_size=1.5, n_points=16, bspline_smoothing=0.04,
                                            bspline_degree=3, engine=engine)
    hand = _raw_tree(tree_inputs, engine)
    mm.replace_contours_with_bsplines(hand, 0.04, 3, engine=engine)
    hand.calculate_ref_pts()
    for g1, g2 in zip(_groups(got), _groups(hand)):
        assert len(g1) == len(g2) and len(g1) > 0
        for a, b in zip(g1, g2):
            assert same_bits(a.points, b.points) and a.centroid == b.centroid and a.id == b.id
    assert got.ao_rca == hand.ao_rca and got.ao_lca == hand.ao_lca
    assert got.rca_references == hand.rca_references and got.lca_references == hand.lca_references
    with pytest.raises(NotImplementedError):
        mm.discretize_vessel_tree(ao, cor, cor, results, b_spline=True)
