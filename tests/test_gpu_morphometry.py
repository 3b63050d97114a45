"""Lumen morphometry on the device (csrc/mm_shape_kernels.hip) bit for bit against the checker
(tests/mm_checkers/morphometry.py): every measure and pair index over sizes that straddle the wave, workgroup and LDS
boundaries, engineered ties and near-ties of the farthest pair, inf / NaN coordinates, the 2-D pass with and without a
stored centroid, a mixed batch against its contours one by one, the contour methods and the summaries of a geometry,
a pair and a discretised vessel tree."""
import math
import os

import numpy as np
import pytest

from mm_checkers import morphometry as MC

import multimoda_rs_amd as mm
from multimoda_rs_amd import morphometry as M
from multimoda_rs_amd.frames import Contour

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [3, 4, 5, 63, 64, 65, 255, 256, 257, 501, 1024, 2049, 3001]    # 3001 > the 1024 points staged in LDS
KEYS = ["area", "major", "minor_3d", "minor_2d", "elliptic_ratio"]
PAIRS = ["major_pair", "minor_3d_pair", "minor_2d_pair"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    """Bit for bit, except that a NaN only has to be a NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def assert_matches(contours, got, closest_2d=True):
    for k, c in enumerate(contours):
        p = getattr(c, "points", c)
        want = MC.measures(p, getattr(c, "centroid", None), closest_2d)
        for key in KEYS:
            assert same(getattr(got, key)[k], want[key]), (k, key, getattr(got, key)[k], want[key])
        for key in PAIRS:
            assert tuple(int(v) for v in getattr(got, key)[k]) == tuple(want[key]), (k, key)


def ring(n, seed, centroid=False):
    r = np.random.default_rng(seed)
    t = np.sort(r.uniform(0, 2 * np.pi, n))
    rad = 1.5 + 0.3 * np.sin(3 * t) + r.normal(0, 0.02, n)
    p = np.stack([4.5 + rad * np.cos(t) * 1.4, 4.5 + rad * np.sin(t), np.full(n, 2.0 + 0.01 * seed)], 1)
    return Contour(seed, seed, p, tuple(r.normal(4.5, 0.05, 3)) if centroid else None)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_match_checker(engine, n):
    cs = [ring(n, 1), ring(n, 2, centroid=True)]
    assert_matches(cs, mm.contour_measures(cs, engine=engine))


def _tie_contours():
    out = []
    for n in (8, 64, 96, 300):                                  # regular polygons on exact axes: many equal diameters
        k = np.arange(n)
        q = n // 4
        p = np.zeros((n, 3))
        p[::q, 0] = [1.0, 0.0, -1.0, 0.0][: len(p[::q])]
        p[::q, 1] = [0.0, 1.0, 0.0, -1.0][: len(p[::q])]
        rest = k % q != 0
        t = 2 * np.pi * k[rest] / n
        p[rest, 0], p[rest, 1] = 0.5 * np.cos(t), 0.5 * np.sin(t)
        out.append(p)
    sq = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], dtype=np.float64)
    out.append(np.tile(sq, (70, 1)))                            # duplicated points: equal pairs in many lanes
    out.append(np.ones((300, 3)))                               # all equal: pair (0, 0), distance 0
    out.append(np.ones((3, 3)))
    # near ties: distinct squared distances 1 and 1 + 2^-52 share the sqrt 1.0
    e = 2.0 ** -26
    for layout in range(3):
        c = np.random.default_rng(layout).normal(0.5, 0.004, (300, 3))
        c[:, 2] = 0.0
        if layout == 0:                                         # same row: the larger d2 comes second
            c[5], c[150], c[200] = (0, 0, 0), (1, 0, 0), (1, e, 0)
        elif layout == 1:                                       # different lanes: the later row has the larger d2
            c[5], c[10], c[150] = (0, 0, 0), (0, e, 0), (1, 0, 0)
        else:                                                   # the balanced high rows of one lane
            c[260], c[280], c[299] = (0, 0, 0), (1, 0, 0), (1, e, 0)
            c[40] = (0, e, 0)
        out.append(c)
    return out


def test_engineered_ties_match_checker(engine):
    cs = _tie_contours()
    got = mm.contour_measures(cs, engine=engine)
    assert_matches(cs, got)
    assert tuple(got.major_pair[5]) == (0, 0) and got.major[5] == 0.0
    assert tuple(got.major_pair[7]) == (5, 150) and tuple(got.major_pair[8]) == (5, 150) and got.major[7] == 1.0


def test_inf_and_nan_coordinates(engine):
    cs = []
    for k, bad in enumerate([np.nan, np.inf, -np.inf]):
        for where in (0, 7, 63):
            c = ring(64, 10 + k).points
            c[where, k % 3] = bad
            cs.append(c)
    c = ring(64, 20).points
    c[:] = np.nan
    cs.append(c)
    assert_matches(cs, mm.contour_measures(cs, engine=engine))


def test_two_d_pass_with_and_without_centroid(engine):
    base = ring(257, 30).points
    cs = [Contour(0, 0, base, None), Contour(1, 1, base, (4.4, 4.6, 0.0)), Contour(2, 2, base, tuple(base.mean(0)))]
    got = mm.contour_measures(cs, engine=engine)
    assert_matches(cs, got)
    skip = mm.contour_measures(cs, closest_2d=False, engine=engine)
    assert np.isnan(skip.minor_2d).all() and (skip.minor_2d_pair == -1).all()
    assert same(skip.major, got.major) and same(skip.elliptic_ratio, got.elliptic_ratio)


def test_mixed_batch_equals_one_by_one(engine):
    r = np.random.default_rng(5)
    cs = [ring(int(n), 40 + k, centroid=bool(k % 2)) for k, n in enumerate(r.integers(3, 700, 24))]
    cs += [Contour(99, 99, np.zeros((0, 3))), Contour(98, 98, np.ones((2, 3))), ring(1500, 77), ring(1, 3)]
    batch = mm.contour_measures(cs, engine=engine)
    for k, c in enumerate(cs):
        one = mm.contour_measures([c], engine=engine)
        for key in KEYS:
            assert same(getattr(batch, key)[k], getattr(one, key)[0]), (k, key)
        for key in PAIRS:
            assert np.array_equal(getattr(batch, key)[k], getattr(one, key)[0])
    assert_matches(cs, batch)
    assert np.isnan(batch.major[-4]) and tuple(batch.major_pair[-4]) == (-1, -1) and batch.area[-4] == 0.0


def test_contour_methods_and_known_answers(engine):
    sq = Contour(1, 1, [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 2.0, 0.0), (0.0, 2.0, 0.0)], (1.0, 1.0, 0.0))
    (p1, p2), d = sq.find_farthest_points(engine=engine)
    assert d == math.sqrt(8.0) and (p1, p2) == ((0.0, 0.0, 0.0), (2.0, 2.0, 0.0))
    op = Contour(1, 1, [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, -0.5, 0.0), (-1.0, 0.0, 0.0)], (0.0, 0.125, 0.0))
    (p1, p2), d = op.find_closest_opposite(engine=engine)
    assert abs(d - 1.5) < 1e-6 and {p1, p2} == {(0.0, 1.0, 0.0), (0.0, -0.5, 0.0)}
    rh = Contour(1, 1, [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (1.0, 4.0, 0.0), (2.0, 2.0, 0.0)], (1.0, 2.0, 0.0))
    assert abs(rh.get_elliptic_ratio(engine=engine) - 2.0) < 1e-6 and abs(rh.get_area(engine=engine) - 4.0) < 1e-6
    two = Contour(1, 1, [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)])
    assert two.get_area(engine=engine) == 0.0
    with pytest.raises(RuntimeError):
        Contour(1, 1, np.zeros((0, 3))).find_farthest_points(engine=engine)
    with pytest.raises(RuntimeError):
        two.find_closest_opposite(engine=engine)
    with pytest.raises(RuntimeError):
        two.get_elliptic_ratio(engine=engine)
    g = mm.build_geometry_from_inputdata(None, os.path.join(GOLD, "ivus_rest"), "full", True)
    from multimoda_rs_amd import frames
    lum = frames.to_frames(g)[0].lumen
    assert lum.get_area(engine=engine) == pytest.approx(5.42, abs=0.1)
    assert lum.find_farthest_points(engine=engine)[1] == pytest.approx(5.2, abs=0.1)
    assert lum.find_closest_opposite(engine=engine)[1] == pytest.approx(1.15, abs=0.1)
    assert lum.get_elliptic_ratio(engine=engine) == pytest.approx(4.52, abs=0.1)


def _check_pair_summary(pair, engine, capsys):
    (sa, sb), table = pair.get_summary(engine=engine)
    text = capsys.readouterr().out
    a, b = pair.geom_a, pair.geom_b
    lum = lambda g: [g.frame_lumen(i) for i in range(g.n_frames)]
    assert same(sa, MC.geometry_summary(lum(a), a.centroids)) and same(sb, MC.geometry_summary(lum(b), b.centroids))
    F = a.n_frames
    ma = [MC.measures(p, closest_2d=False) for p in lum(a)]
    mb = [MC.measures(p, closest_2d=False) for p in lum(b)[:F]]
    z = M._lumen_z(a)
    want = np.array([[a.lumen_ids[i], ma[i]["area"], ma[i]["elliptic_ratio"], mb[i]["area"], mb[i]["elliptic_ratio"],
                      z[i]] for i in range(F)]).reshape(F, 6)
    assert same(table, want)
    assert text == MC.deformation_table_text(a.lumen_ids, *[want[:, k] for k in range(1, 6)])
    assert same(a.get_summary(engine=engine), sa)


def test_pair_summary_on_ivus_rest(engine, capsys):
    pair, _ = mm.from_file_singlepair(os.path.join(GOLD, "ivus_rest"), step_rotation_deg=1.0, range_rotation_deg=30.0,
                                      write_obj=False, engine=engine)
    capsys.readouterr()
    _check_pair_summary(pair, engine, capsys)


def test_pair_summary_on_synthetic_case(engine, capsys):
    g = mm.synthetic_case(24)
    _check_pair_summary(mm.GeometryPair(g[0], g[1]), engine, capsys)
    _check_pair_summary(mm.GeometryPair(g[2], mm.synthetic_pullback(30, 501, pullback_id=3)), engine, capsys)


def test_tree_summary_matches_checker(engine):
    from test_gpu_discretize import _tree_cl, curved_tube
    from multimoda_rs_amd.centerline import Centerline
    xyz, tan, bid, pts = curved_tube(41, branches=3)
    ao = _tree_cl(curved_tube(42, n_cl=60)[0])
    cor = Centerline.from_arrays(xyz, tan, branch_id=bid)
    ao_pts = curved_tube(42, n_cl=60, radius=6.0)[3][0]
    tree = mm.ccta.discretize_vessel_tree_raw(ao, cor, cor, ao_pts, pts[0], pts[0], [pts[1], pts[2]], [pts[2]],
                                              step_size=0.7, n_points=60, engine=engine)
    got = tree.get_summary(engine=engine)
    vessels = [("aorta", tree.discretized_aorta), ("rca_main", tree.discretized_rca_main),
               ("lca_main", tree.discretized_lca_main)]
    vessels += [(("rca_branches", k), v) for k, v in enumerate(tree.rca_branches)]
    vessels += [(("lca_branches", k), v) for k, v in enumerate(tree.lca_branches)]
    assert len(got["rca_branches"]) == 2 and len(got["lca_branches"]) == 1
    for key, v in vessels:
        summary, table = got[key] if isinstance(key, str) else got[key[0]][key[1]]
        assert len(v) > 0 and table.shape == (len(v), 6)
        cen = np.array([c.centroid for c in v])
        assert same(summary, MC.geometry_summary([c.points for c in v], cen))
        ms = [MC.measures(c.points, closest_2d=False) for c in v]
        want = np.array([[c.id, m["area"], m["elliptic_ratio"], m["major"], m["minor_3d"], c.centroid[2]]
                         for c, m in zip(v, ms)])
        assert same(table, want)


def test_bad_arguments_are_errors(engine):
    L = mm._native.lib()
    off = np.array([0, 3, 2], dtype=np.int64)
    xyz = np.zeros((3, 3))
    val, idx = np.zeros((2, 5)), np.zeros((2, 6), dtype=np.int64)
    P = mm._native._ptr
    assert L.mm_contour_measures(engine.handle, 2, P(off), P(xyz), None, None, 0, P(val), P(idx)) == -2
    off = np.array([0, 3], dtype=np.int64)
    assert L.mm_contour_measures(engine.handle, 1, P(off), P(xyz), None, None, 4, P(val), P(idx)) == -2
    assert L.mm_contour_measures(engine.handle, 1, P(off), None, None, None, 0, P(val), P(idx)) == -2
    assert L.mm_contour_measures(engine.handle, -1, P(off), P(xyz), None, None, 0, P(val), P(idx)) == -2
    assert L.mm_contour_measures(engine.handle, 0, None, None, None, None, 0, None, None) == 0
