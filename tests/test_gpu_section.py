"""Mesh cross-sections on the device (csrc/mm_section_kernels.hip, csrc/mm_section.cpp) against the checker
(tests/mm_checkers/mesh_sections.py): every array and every report integer equal, bit for bit; items and items_total
equal mm_section_plan's.  Cases: the known answers, a jittered closed tube under tilted planes, the same on a 1/8 grid
(many zero heights), one face past a chunk, one plane past a run, a long tube (the cull happens and loses nothing),
shuffled faces, a segment buffer below the count, a small call behind a large one, empty inputs, the argument checks,
and the lumen profile of a tube with a dip against the analytic polygon areas."""
import ctypes as C
import math

import numpy as np
import pytest

from mm_checkers import mesh_sections as X
from test_section_host import CASES, checked, cube, same_arrays, tube

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu

N = mm._native
S = mm.section
MM_ERR_INVALID, MM_ERR_TOO_LARGE = -2, -3


def same_as_checker(got, want, mesh, o, n):
    same_arrays(got, want)
    for k, x in want["counts"].items():
        assert got.report[k] == x, (k, got.report[k], x)
    plan = S.section_plan(mesh, o, n)
    assert got.report["items"] == plan["pairs"] and got.report["items_total"] == plan["pairs_total"]
    assert got.report["face_tests"] == plan["face_tests"]
    rep = X.predict_report(len(mesh[1]), len(want["plane_off"]) - 1, plan["pairs"], len(plan["items"]), want["counts"]["n_segments"])
    for k, x in rep.items():
        assert got.report[k] == x, (k, got.report[k], x)
    return got


def case(name, engine, **kw):
    v, f, o, n = CASES[name]
    return same_as_checker(mm.mesh_cross_sections((v, f), o, n, engine=engine, **kw), checked(name), (v, f), o, n)


def test_cube_and_octahedron(engine):
    got = case("cube_mid", engine)
    assert got.contour_area.tolist() == [1.0, 1.0] and got.contour_length.tolist() == [4.0, 4.0]
    assert got.contour_centroid.tolist() == [[0.5, 0.5, 0.5]] * 2 and got.selected.tolist() == [0, -1]
    got = case("octahedron_equator", engine)
    assert got.contour_area.tolist() == [2.0] and len(got.contour(0)) == 4
    got = case("cube_faces", engine)
    assert got.plane_off.tolist() == [0, 0, 1, 1] and got.contour_kind.tolist() == [0]


@pytest.mark.parametrize("name,kinds", [("open_tube_rim", [1]), ("hung_faces", [2]), ("tube_in_tube", [0] * 4),
                                        ("two_arms", [0] * 6), ("repeated_index", [0])])
def test_known_shapes(engine, name, kinds):
    got = case(name, engine)
    assert got.contour_kind.tolist() == kinds
    if name == "repeated_index":
        assert got.report["n_skipped_faces"] == 2


def test_jittered_tube_under_tilted_planes(engine):
    got = case("jittered_tube", engine)
    assert got.report["n_faces"] == 600 and got.report["n_planes"] == 40 and got.report["n_closed"] > 20


def test_grid_tube_with_many_zero_heights(engine):
    got = case("grid_tube", engine)
    assert got.report["n_closed"] > 20


def test_one_face_past_a_chunk_and_one_plane_past_a_run(engine):
    got = case("faces_257", engine)
    assert got.report["items_total"] == 2 * 6
    got = case("planes_70", engine)
    assert got.report["items"] == got.report["items_total"] == 70 and got.report["n_closed"] == 70


def test_long_tube_is_culled_and_loses_nothing(engine):
    got = case("long_tube", engine)
    assert 0 < got.report["items"] <= got.report["items_total"] // 2 and got.report["items_total"] == 16 * 32
    assert got.report["n_closed"] == 32 and (got.selected >= 0).all()


def test_shuffled_faces_give_the_same_contours(engine):
    v, f, o, n = CASES["jittered_tube"]
    want = checked("jittered_tube")
    perm = np.random.default_rng(11).permutation(len(f))
    got = mm.mesh_cross_sections((v, f[perm]), o, n, engine=engine)
    for k in X.ARRAYS:
        if k != "point_face":
            assert X.same_bits(getattr(got, k), want[k]), k
    back = np.where(got.point_face >= 0, perm[np.maximum(got.point_face, 0)], -1)
    assert np.array_equal(back, want["point_face"])


def test_max_segments_below_the_count(engine):
    v, f, o, n = CASES["jittered_tube"]
    full = case("jittered_tube", engine)
    n_seg = full.report["n_segments"]
    assert n_seg > 100 and full.report["attempts"] == 1
    got = mm.mesh_cross_sections((v, f), o, n, max_segments=n_seg // 3, engine=engine)
    assert got.report["attempts"] == 2
    same_arrays(got, checked("jittered_tube"))
    # through the C ABI: MM_ERR_TOO_LARGE with the full count, nothing else written
    out = S._Outputs(n_seg // 3, len(o))
    out.selected[:] = -77
    rep = N.MMSectionReport()
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int64)
    oo, nn = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(n, dtype=np.float64)
    rc = N.lib().mm_mesh_sections(engine.handle, N._ptr(v), len(v), N._ptr(f), len(f), N._ptr(oo), N._ptr(nn), len(oo), n_seg // 3,
                                  *out.pointers(), C.byref(rep))
    assert rc == MM_ERR_TOO_LARGE and rep.n_segments == n_seg and (out.selected == -77).all() and not out.points.any()
    exact = mm.mesh_cross_sections((v, f), o, n, max_segments=n_seg, engine=engine)
    assert exact.report["attempts"] == 1 and exact.report == full.report


def test_a_small_call_behind_a_large_one(engine):
    case("long_tube", engine)                                             # leaves records and a counter behind
    small = case("cube_mid", engine)
    fresh_engine = mm.Engine()
    try:
        v, f, o, n = CASES["cube_mid"]
        fresh = mm.mesh_cross_sections((v, f), o, n, engine=fresh_engine)
    finally:
        fresh_engine.close()
    for k in X.ARRAYS:
        assert X.same_bits(getattr(small, k), getattr(fresh, k)), k
    assert small.report == fresh.report


def test_empty_inputs(engine):
    v, f = cube()
    none_f = np.zeros((0, 3), dtype=np.int64)
    o, n = [[0.5, 0.5, 0.5]], [[0, 0, 1.0]]
    got = same_as_checker(mm.mesh_cross_sections((v, none_f), o, n, engine=engine), X.scan(v, none_f, o, n), (v, none_f), o, n)
    assert len(got) == 0 and got.selected.tolist() == [-1] and got.report["n_launches"] == 0
    got = same_as_checker(mm.mesh_cross_sections((v, f), np.zeros((0, 3)), np.zeros((0, 3)), engine=engine),
                          X.scan(v, f, [], []), (v, f), np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(got) == 0 and got.selected.shape == (0,) and got.plane_off.tolist() == [0] and got.report["bytes_uploaded"] == 0
    far = mm.mesh_cross_sections((v, f), [[0, 0, 9.0]], n, engine=engine)      # faces and a plane, but no item
    assert far.report["items"] == 0 and far.report["items_total"] == 1 and far.report["n_launches"] == 0 and len(far) == 0


def test_invalid_arguments(engine):
    v, f = cube()
    o, n = np.array([[0.5, 0.5, 0.5]]), np.array([[0, 0, 1.0]])
    with pytest.raises(ValueError, match="zero"):
        mm.mesh_cross_sections((v, f), o, [[0, 0, 0.0]], engine=engine)
    with pytest.raises(ValueError, match="out of range"):
        mm.mesh_cross_sections((v, f + 1), o, n, engine=engine)
    out = S._Outputs(64, 1)
    rep = N.MMSectionReport()
    f64 = np.ascontiguousarray(f, dtype=np.int64)
    bad_v, bad_n = v.copy(), np.array([[0.0, 0.0, 0.0]])
    bad_v[1, 1] = np.inf
    for args, err in (((bad_v, f64, o, n), "non-finite vertex coordinate"), ((v, f64 + 1, o, n), "face index out of range"),
                      ((v, f64, o, bad_n), "zero plane normal"), ((v, f64, o * np.nan, n), "non-finite plane origin"),
                      ((v, f64, o, np.array([[0.0, np.inf, 1.0]])), "non-finite plane normal")):
        a = [np.ascontiguousarray(x) for x in args]
        rc = N.lib().mm_mesh_sections(engine.handle, N._ptr(a[0]), 8, N._ptr(a[1]), 12, N._ptr(a[2]), N._ptr(a[3]), 1, 64,
                                      *out.pointers(), C.byref(rep))
        assert rc == MM_ERR_INVALID and N.last_error() == "mm_mesh_sections: " + err, err
    assert N.lib().mm_mesh_sections(engine.handle, N._ptr(v), 8, N._ptr(f64), 12, N._ptr(o), N._ptr(n), 1, -1, *out.pointers(),
                                    C.byref(rep)) == MM_ERR_INVALID


def dip_tube():
    """64 sides, rings 0.5 apart along x, radius 2 with a dip to 1.2 over five stations; the centerline on the axis"""
    dip = {10: 1.8, 11: 1.5, 12: 1.2, 13: 1.5, 14: 1.8}
    radius = lambda i: dip.get(i, 2.0)                                    # noqa: E731
    v, f = tube(64, 25, radius, 0.5)
    stations = np.arange(2, 23)
    xyz = np.stack([stations * 0.5, 0 * stations, 0 * stations], 1).astype(float)
    cl = mm.Centerline.from_arrays(xyz, np.tile([1.0, 0.0, 0.0], (len(stations), 1)), radius=2.0, branch_id=0)
    return (v, f), cl, np.array([radius(int(i)) for i in stations])


def test_lumen_profile_of_a_tube_with_a_dip(engine):
    mesh, cl, radii = dip_tube()
    contours, sec = mm.centerline_cross_sections(mesh, cl, engine=engine)
    assert len(contours) == len(cl) == 21 and all(c is not None and c.kind == "lumen" for c in contours)
    assert [c.id for c in contours] == list(range(21))
    prof = mm.vessel_profile(mesh, cl, engine=engine)
    assert prof.table.shape == (21, 8) and prof.report["n_missing"] == 0 and prof.report["n_stations"] == 21
    want = 32.0 * radii * radii * math.sin(2.0 * math.pi / 64.0)
    rel = np.abs(prof.table[:, 2] - want) / want
    print("largest relative area error:", rel.max())
    assert (rel <= 1e-12).all()
    assert np.array_equal(prof.table[:, 2], sec.contour_area[sec.selected])
    assert np.array_equal(prof.table[:, 3], 2.0 * np.sqrt(prof.table[:, 2] / math.pi))
    assert np.array_equal(prof.table[:, 1], 0.5 * np.arange(21)) and np.array_equal(prof.table[:, 7], sec.contour_length[sec.selected])
    k = int(np.argmin(prof.table[:, 2]))
    assert k == 10 and radii[k] == 1.2 and prof.summary[0] == prof.table[k, 2]          # the MLA row is the dip's station
    m = mm.contour_measures(contours, engine=engine)
    assert np.array_equal(prof.table[:, 4], m.major) and np.array_equal(prof.table[:, 5], m.minor_3d)
    assert np.array_equal(prof.table[:, 6], m.elliptic_ratio)
    # a station outside the mesh: a row of NaN, left out of the summary
    xyz = np.concatenate([cl.xyz(), [[50.0, 0.0, 0.0]]])
    cl2 = mm.Centerline.from_arrays(xyz, np.tile([1.0, 0.0, 0.0], (22, 1)), radius=2.0, branch_id=0)
    prof2 = mm.vessel_profile(mesh, cl2, engine=engine)
    assert prof2.report["n_missing"] == 1 and np.isnan(prof2.table[21, 2:]).all() and prof2.contours[21] is None
    assert prof2.summary == prof.summary and np.array_equal(prof2.table[:21], prof.table)
    # the centerline resampled, one branch of it, a branch it does not have
    coarse = cl.resample(1.0)
    contours, sec = mm.centerline_cross_sections(mesh, cl, branch_id=0, step_mm=1.0, engine=engine)
    assert len(contours) == len(coarse) < len(cl) and all(c is not None for c in contours)
    # a symmetric loop's centroid is on the axis: 128 cancelling terms of size 2 at 2^-53 each, over 3 W = 36
    assert np.abs(sec.contour_centroid[sec.selected][:, 1:]).max() < 1e-12
    none, empty = mm.centerline_cross_sections(mesh, cl, branch_id=3, engine=engine)
    assert none == [] and len(empty) == 0 and empty.report["n_planes"] == 0
