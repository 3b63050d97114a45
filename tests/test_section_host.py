"""Mesh cross-sections on the host (no GPU): the checker (tests/mm_checkers/mesh_sections.py) against known answers,
and the host hooks -- mm_section_plan, mm_section_cut_host (the arithmetic the kernel runs) and mm_section_chain (the code
the product runs on the device's records) -- against the checker bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from mm_checkers import mesh_sections as X
from test_trim_host import octahedron

import multimoda_rs_amd as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = mm.section


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=float)          # index = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return v, f


def tube(n_around, n_rings, radius=1.0, dx=1.0, caps=False, centre=(0.0, 0.0), jitter=0.0, seed=0, snap=None):
    """A tube along x: ring i at x = i dx with radius(i) (a number or a function), 2 n_around (n_rings - 1) side faces and,
    with caps, 2 n_around more on two centre vertices."""
    r = radius if callable(radius) else (lambda i: radius)
    ang = 2.0 * np.pi * np.arange(n_around) / n_around
    v = np.array([[i * dx, centre[0] + r(i) * np.cos(a), centre[1] + r(i) * np.sin(a)] for i in range(n_rings) for a in ang])
    f = []
    for i in range(n_rings - 1):
        for j in range(n_around):
            a, b = i * n_around + j, i * n_around + (j + 1) % n_around
            f += [(a, b, b + n_around), (a, b + n_around, a + n_around)]
    if caps:
        v = np.concatenate([v, [[0.0, centre[0], centre[1]], [(n_rings - 1) * dx, centre[0], centre[1]]]])
        c0, c1, last = len(v) - 2, len(v) - 1, (n_rings - 1) * n_around
        for j in range(n_around):
            f += [(c0, (j + 1) % n_around, j), (c1, last + j, last + (j + 1) % n_around)]
    if jitter:
        v = v + np.random.default_rng(seed).uniform(-jitter, jitter, v.shape)
    if snap:
        v = np.round(v * snap) / snap
    return v, np.array(f, dtype=np.int64)


def join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + base); base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def tilted_planes(n, x_lo, x_hi, seed, tilt=0.4):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(x_lo, x_hi, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], 1)
    nrm = np.stack([np.ones(n), rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n)], 1) * rng.uniform(0.5, 2.0, (n, 1))
    return o, nrm


def x_planes(xs):
    xs = np.asarray(xs, dtype=float)
    return np.stack([xs, 0 * xs, 0 * xs], 1), np.tile([1.0, 0.0, 0.0], (len(xs), 1))


def _cases():
    c = {}
    c["cube_mid"] = (*cube(), [[0.5, 0.5, 0.5], [2.0, 2.0, 0.5]], [[0, 0, 1.0], [0, 0, 1.0]])
    c["octahedron_equator"] = (*octahedron(), [[0.0, 0.0, 0.0]], [[0, 0, 1.0]])
    c["cube_faces"] = (*cube(), [[0.5, 0.5, 0.0], [0.5, 0.5, 1.0], [0.5, 0.5, 1.5]], [[0, 0, 1.0]] * 3)
    c["open_tube_rim"] = (*tube(12, 4), [[0.2, 0.0, 0.0]], [[1.0, 0.0, 1.0]])
    hung = (np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.5], [0.5, 0, 1.0], [3, 3, 3], [4, 3, 3], [3, 4, 3]], dtype=float),
            np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [5, 6, 7]]))
    c["hung_faces"] = (*hung, [[0.5, 0.0, 0.0]], [[1.0, 0.0, 0.0]])
    c["tube_in_tube"] = (*join(tube(16, 5, 2.0), tube(12, 5, 1.0)), [[1.5, 0.1, 0.0], [2.5, 1.5, 0.0]], [[1.0, 0.1, 0.0], [1.0, 0.0, 0.0]])
    c["two_arms"] = (*join(tube(10, 5, 1.0, centre=(-2.0, 0.0)), tube(10, 5, 0.7, centre=(2.0, 0.5))),
                     [[1.5, 2.0, 0.5], [2.5, -2.0, 0.0], [2.5, 0.0, 0.0]], [[1.0, 0.0, 0.0]] * 3)
    v, f = cube()
    c["repeated_index"] = (v, np.concatenate([f, [[0, 0, 7], [3, 5, 3]]]), [[0.5, 0.5, 0.5]], [[0, 0, 1.0]])
    c["jittered_tube"] = (*tube(15, 20, 1.5, 0.5, caps=True, jitter=0.05, seed=3), *tilted_planes(40, -0.5, 10.0, 4))
    vg, fg = tube(15, 20, 1.5, 0.5, caps=True, jitter=0.05, seed=3, snap=8)
    og, ng = tilted_planes(40, 0.0, 9.5, 5)
    c["grid_tube"] = (vg, fg, np.round(og * 8) / 8, np.round(ng * 4) / 4 + [1.0, 0, 0])
    c["faces_257"] = (*tube(8, 18, 1.0, 0.25, jitter=0.02, seed=6)[:1], tube(8, 18)[1][:257], *tilted_planes(6, 0.0, 4.0, 7))
    c["planes_70"] = (*tube(8, 9, 1.0, 1.0), *x_planes(0.05 + np.arange(70) * 0.11))
    c["long_tube"] = (*tube(16, 129, 1.0, 0.25, jitter=0.01, seed=8), *x_planes(0.3 + np.arange(32) * 0.99))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def checked(name):
    return X.scan(*CASES[name])


def same_arrays(got, want):
    for k in X.ARRAYS:
        assert X.same_bits(getattr(got, k), want[k]), k


def host(name):
    """The host hooks on a case: the cut, then the chain, both equal to the checker."""
    v, f, o, n = CASES[name]
    want = checked(name)
    seg = S.section_cut_host((v, f), o, n)
    assert seg.tobytes() == X.to_records(want["segments"]).tobytes()
    got = S.section_chain(seg, o, n)
    same_arrays(got, want)
    for k in ("n_segments", "n_contours", "n_closed", "n_open", "n_branched"):
        assert got.report[k] == want["counts"][k], k
    return got


def test_public_names_and_abi():
    for name in ("mesh_cross_sections", "centerline_cross_sections", "vessel_profile", "MeshCrossSections", "section"):
        assert hasattr(mm, name) and name in mm.__all__
    header = open(os.path.join(ROOT, "include", "mm_ccta.h")).read()
    for sym in ("mm_mesh_sections", "mm_section_plan", "mm_section_cut_host", "mm_section_chain"):
        assert f"int     {sym}(" in header and sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)
    assert C.sizeof(mm._native.MMSectionReport) == 112 and "/* 112 bytes */" in header
    assert [n for n, _t in mm._native.MMSectionReport._fields_] == list(S.SECTION_REPORT_KEYS)
    assert f"#define MM_SECTION_SEGMENT_BYTES {X.SEGMENT_BYTES}" in header and S.SEGMENT_DTYPE == X.SEGMENT_DTYPE
    assert "welds" in mm.mesh_cross_sections.__doc__ and "roadmap" in mm.vessel_profile.__doc__


def test_cube_cut_in_the_middle():
    got = host("cube_mid")
    assert got.contour_off.tolist() == [0, 8, 16] and got.contour_kind.tolist() == [0, 0]
    assert got.contour_area.tolist() == [1.0, 1.0] and got.contour_length.tolist() == [4.0, 4.0]
    assert got.contour_centroid.tolist() == [[0.5, 0.5, 0.5]] * 2
    assert got.selected.tolist() == [0, -1] and got.plane_off.tolist() == [0, 1, 2]
    assert (got.point_face >= 0).all() and len(set(got.point_face[:8].tolist())) == 8
    assert np.array_equal(got.contour(1), got.points[8:16])


def test_octahedron_through_four_vertices_and_four_edges():
    got = host("octahedron_equator")
    assert got.contour_kind.tolist() == [0] and got.contour_area.tolist() == [2.0]
    pts = got.contour(0)
    assert len(pts) == 4 and sorted(map(tuple, pts.tolist())) == sorted(map(tuple, octahedron()[0][:4].tolist()))
    assert set(got.point_face.tolist()) == {4, 5, 6, 7}                   # the upper faces lie on the plane's upper side
    assert got.selected.tolist() == [0]


def test_planes_that_hold_whole_faces():
    got = host("cube_faces")
    assert got.plane_off.tolist() == [0, 0, 1, 1]                         # z = 0: nothing is below it; z = 1: the top face's rim
    assert got.contour_kind.tolist() == [0] and got.contour_area.tolist() == [1.0]
    assert checked("cube_faces")["counts"]["n_open"] == 0 and checked("cube_faces")["counts"]["n_branched"] == 0


def test_open_tube_through_its_rim():
    got = host("open_tube_rim")
    assert got.contour_kind.tolist() == [1] and np.isnan(got.contour_area[0]) and got.contour_length[0] > 0
    first, last = tuple(got.point_edge[0]), tuple(got.point_edge[-1])
    assert first < last and got.point_face[-1] == -1 and (got.point_face[:-1] >= 0).all()
    assert got.selected.tolist() == [-1]


def test_faces_hung_on_an_edge_branch():
    got = host("hung_faces")
    assert got.contour_kind.tolist() == [2] and np.isnan(got.contour_area[0]) and np.isnan(got.contour_centroid[0]).all()
    keys = [tuple(e) for e in got.point_edge.tolist()]
    assert keys == sorted(keys) and len(keys) == 4 and (got.point_face == -1).all()
    assert got.report["n_segments"] == 3 and got.selected.tolist() == [-1]


def test_tube_in_tube_selects_the_inner_loop():
    got = host("tube_in_tube")
    assert got.plane_off.tolist() == [0, 2, 4] and got.contour_kind.tolist() == [0] * 4
    inner = int(got.selected[0])
    assert inner in (0, 1) and got.contour_area[inner] == got.contour_area[:2].min() < 0.5 * got.contour_area[:2].max()
    outer = int(got.selected[1])                                          # an origin between the walls: the outer loop only
    assert outer in (2, 3) and got.contour_area[outer] == got.contour_area[2:].max()


def test_two_arms_select_the_loop_around_the_origin():
    got = host("two_arms")
    assert got.plane_off.tolist() == [0, 2, 4, 6]
    c0, c1 = int(got.selected[0]), int(got.selected[1])
    assert abs(got.contour_centroid[c0][1] - 2.0) < 1e-9 and abs(got.contour_centroid[c1][1] + 2.0) < 1e-9
    assert got.selected[2] == -1


def test_a_repeated_index_is_skipped_and_counted():
    got = host("repeated_index")
    assert checked("repeated_index")["counts"]["n_skipped_faces"] == 2 and got.contour_area.tolist() == [1.0]
    assert S.section_plan(CASES["repeated_index"][:2], *CASES["repeated_index"][2:])["n_skipped_faces"] == 2


@pytest.mark.parametrize("name", ["jittered_tube", "grid_tube", "faces_257", "planes_70", "long_tube"])
def test_hooks_equal_the_checker(name):
    got = host(name)
    assert got.report["n_closed"] > 0
    if name == "grid_tube":                                               # the zero heights are many
        v, _f, o, n = CASES[name]
        zeros = sum(X.height(oo, nn, x) == 0.0 for oo, nn in zip(o.tolist(), n.tolist()) for x in v.tolist())
        assert zeros > 20


def test_a_plane_that_misses():
    v, f = cube()
    got = S.section_chain(S.section_cut_host((v, f), [[0, 0, 5.0]], [[0, 0, 1.0]]), [[0, 0, 5.0]], [[0, 0, 1.0]])
    assert len(got) == 0 and got.plane_off.tolist() == [0, 0] and got.selected.tolist() == [-1]
    assert X.scan(v, f, [[0, 0, 5.0]], [[0, 0, 1.0]])["counts"]["n_contours"] == 0


def test_plan_culls_and_loses_nothing():
    v, f, o, n = CASES["long_tube"]
    plan = S.section_plan((v, f), o, n)
    assert len(f) == 4096 and plan["chunk"] == X.CHUNK and len(plan["boxes"]) == 16 and plan["run"] == X.RUN
    assert sorted(plan["order"].tolist()) == list(range(4096))
    want_pairs, boxes = X.box_pairs(plan["order"].tolist(), v, f, o, n)
    assert np.array_equal(plan["boxes"], np.array([lo + hi for lo, hi in boxes]))
    got_pairs = sorted((int(p), int(c)) for c, first, cnt, _z in plan["items"].tolist() for p in plan["plane_list"][first:first + cnt])
    assert got_pairs == sorted(want_pairs) and plan["pairs"] == len(want_pairs) and plan["pairs_total"] == 16 * 32
    assert set(X.crossed_pairs(plan["order"].tolist(), checked("long_tube")["segments"])) <= set(got_pairs)
    assert 0 < plan["pairs"] <= plan["pairs_total"] // 2
    assert plan["face_tests"] == 256 * plan["pairs"]


def test_plane_runs_are_cut_at_64():
    v, f, o, n = CASES["planes_70"]
    plan = S.section_plan((v, f), o, n)
    assert len(plan["boxes"]) == 1 and plan["pairs"] == 70
    assert plan["items"].tolist() == [[0, 0, 64, 0], [0, 64, 6, 0]] and plan["plane_list"].tolist() == list(range(70))


def test_argument_checks_come_before_the_engine():
    v, f = cube()
    o, n = [[0.5, 0.5, 0.5]], [[0, 0, 1.0]]
    bad_v, bad_f = v.copy(), f.copy()
    bad_v[3, 1], bad_f[2, 2] = np.nan, 8
    for args, match in ((((v, f), o, [[0, 0, 0.0]]), "zero"), (((v, f), o, [[0, np.inf, 1.0]]), "finite"),
                        (((v, f), [[np.nan, 0, 0]], n), "finite"), (((v, f), o, [[0, 0, 1.0]] * 2), r"\(P, 3\)"),
                        (((bad_v, f), o, n), "finite"), (((v, bad_f), o, n), "out of range")):
        with pytest.raises(ValueError, match=match):
            mm.mesh_cross_sections(*args, engine=object())               # never reached
    with pytest.raises(ValueError, match="max_segments"):
        mm.mesh_cross_sections((v, f), o, n, max_segments=-1, engine=object())
    seg = S.section_cut_host((v, f), o, n)
    with pytest.raises(RuntimeError, match="not sorted"):
        S.section_chain(seg[::-1], o, n)
