"""Mesh clipping on the device (csrc/mm_clip_kernels.hip, csrc/mm_clip.cpp) against the checker
(tests/mm_checkers/mesh_clip.py): every array bit for bit, every count, and the launches and bytes the checker's
predict_report restates from the sizes and the measured jump rounds.  The cases of tests/test_clip_host.py, with the
project's own manifold report and winding fix on their results, plus the smallest sizes at which a kernel can go wrong:
257 faces (one past a workgroup), 4097 vertices and 8160 faces (one past a scan tile, both scans), a tube 8 around x 600
rings (several pointer-jumping rounds), 3 cuts in one call, shuffled faces, a small call behind a large one on the same
engine (stale scratch), buffers below the counts and the retry, empty inputs."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as CC
from clip_cases import CASES, checked, edge_report, run
from mm_checkers import mesh_clip as Y

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu

MM_ERR_INVALID, MM_ERR_TOO_LARGE = -2, -3


def device(name, engine, **kw):
    """The case on the device with strict off: the checker's arrays and counts, and the predicted report."""
    got = run(name, mm.clip_mesh, engine=engine, strict=False, **kw)
    v, f, o = CASES[name][:3]
    want = Y.predict_report(len(v), len(f), len(o), checked(name), got.report["jump_rounds"])
    for k, x in want.items():
        assert got.report[k] == x, (name, k, got.report[k], x)
    return got


def test_unit_cube_cut_in_half_and_capped(engine):
    got = device("cube_plane_cap", engine)
    assert got.vertices[-1].tolist() == [0.5, 0.5, 0.5] and got.report["jump_rounds"] >= 1
    rep = mm.mesh_manifold_report((got.vertices, got.faces), engine=engine)
    assert rep["n_open_edges"] == 0 and rep["n_nonmanifold_edges"] == 0 and rep["watertight"]
    assert np.array_equal(mm.fix_mesh_winding(got.faces, engine=engine), got.faces)


def test_loop_and_plane_cuts_of_two_arms(engine):
    loop, plane = device("two_arms_loop", engine), device("two_arms_plane", engine)
    assert np.isin(np.arange(50), loop.vertex_origin).all() and not np.isin(np.arange(50), plane.vertex_origin).all()


@pytest.mark.parametrize("name", ["tube_both_ends", "tube_inward"])
def test_closed_tube_opened_extended_and_capped(engine, name):
    got = device(name, engine)
    rep = mm.mesh_manifold_report((got.vertices, got.faces), engine=engine)
    assert rep["watertight"] and edge_report(got.faces) == (0, 0, 0)
    fixed = mm.fix_mesh_winding(got.faces, engine=engine)                  # nothing flips, or (never here: face 0 stays) everything
    assert np.array_equal(fixed, got.faces) or np.array_equal(fixed, got.faces[:, ::-1])
    assert np.bincount(got.face_kind, minlength=4)[2:].tolist() == [6 * got.cut_points.sum(), got.cut_points.sum()]


def test_null_pieces_are_counted(engine):
    assert device("grid_tube", engine).report["n_null_pieces"] == 5


def test_torus_statuses(engine):
    v, f = CASES["torus_one_cut"][:2]
    one = device("torus_one_cut", engine)
    assert one.cut_status.tolist() == [Y.NOT_SEPARATING] and one.vertices.tobytes() == v.tobytes() and one.faces.tobytes() == f.tobytes()
    assert one.report["n_launches"] == 5 + one.report["jump_rounds"]
    with pytest.raises(mm.ClipError) as err:
        mm.clip_mesh((v, f), *CASES["torus_one_cut"][2:4], engine=engine)
    assert err.value.statuses == [Y.NOT_SEPARATING]
    assert device("torus_two_cuts", engine).cut_status.tolist() == [Y.OK, Y.OK]
    assert device("torus_overlap", engine).report["n_launches"] == 0
    assert device("torus_miss", engine).cut_status.tolist() == [Y.OK, Y.NO_LOOP]


@pytest.mark.parametrize("name", ["faces_257", "scan_tiles", "three_cuts", "open_tube_plane"])
def test_sizes_where_a_kernel_takes_another_path(engine, name):
    got = device(name, engine)
    assert got.applied
    if name == "scan_tiles":
        assert len(CASES[name][0]) == 4097 and len(CASES[name][1]) > 4096


def test_a_long_thin_tube_needs_several_jump_rounds(engine):
    got = device("long_thin", engine)
    print("jump_rounds", got.report["jump_rounds"])
    assert got.report["jump_rounds"] >= 2


def test_shuffled_faces(engine):
    v, f, o, n, keep, scope, cap, ext = CASES["tube_both_ends"]
    perm = np.random.default_rng(5).permutation(len(f))
    base = device("tube_both_ends", engine)
    got = mm.clip_mesh((v, f[perm]), o, n, keep=keep, scope=scope, cap=cap, extension=ext, engine=engine)
    assert got.vertices.tobytes() == base.vertices.tobytes() and got.vertex_origin.tobytes() == base.vertex_origin.tobytes()
    origin = np.where(got.face_origin >= 0, perm[np.maximum(got.face_origin, 0)], got.face_origin)
    as_set = lambda faces, org, kind: sorted(zip(map(tuple, faces.tolist()), org.tolist(), kind.tolist()))   # noqa: E731
    assert as_set(got.faces, origin, got.face_kind) == as_set(base.faces, base.face_origin, base.face_kind)


def test_a_small_call_behind_a_large_one(engine):
    device("scan_tiles", engine)
    device("cube_plane_cap", engine)
    device("torus_two_cuts", engine)


def test_buffers_below_the_counts_and_the_retry(engine):
    v, f, o, n = CASES["cube_plane_cap"][:4]
    o, n = np.array(o, dtype=float), np.array(n, dtype=float)
    keep, scope = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32)
    rep = mm._native.MMClipReport()
    P = mm._native._ptr

    def call(vert_cap, face_cap):
        ov, of = np.full((vert_cap, 3), 7.0), np.full((face_cap, 3), 7, dtype=np.int64)
        rest = [np.zeros(vert_cap, dtype=np.int64), np.zeros(face_cap, dtype=np.int64), np.zeros(face_cap, dtype=np.int8),
                np.zeros((1, 4), dtype=np.int64), np.zeros((1, 5)), np.zeros(vert_cap + 1, dtype=np.int64), np.zeros(vert_cap, dtype=np.int64)]
        rc = mm._native.lib().mm_mesh_clip(engine.handle, P(v), 8, P(f), 12, P(o), P(n), P(keep), P(scope), 1, 1, 0.0, 0, vert_cap,
                                           face_cap, P(ov), P(of), *[P(b) for b in rest], C.byref(rep))
        return rc, ov, of
    rc, ov, of = call(13, 21)                                             # one face short
    assert rc == MM_ERR_TOO_LARGE and (rep.n_vertices, rep.n_faces) == (13, 22) and (ov == 7.0).all() and (of == 7).all()
    rc, ov, of = call(12, 22)                                             # one vertex short
    assert rc == MM_ERR_TOO_LARGE and (rep.n_vertices, rep.n_faces) == (13, 22) and (ov == 7.0).all()
    rc, ov, of = call(int(rep.n_vertices), int(rep.n_faces))
    want = checked("cube_plane_cap")
    assert rc == 0 and ov.tobytes() == want["vertices"].tobytes() and of.tobytes() == want["faces"].tobytes()
    # the public call grows its buffers once: a loop of 400 points on 800 faces is longer than its first guess allows for
    from test_section_host import tube
    v, f = tube(200, 3, 1.0, 1.0, jitter=0.01, seed=13)
    o, n = [[1.5, 0.0, 0.0]], [[1.0, 0.01, 0.0]]
    got = mm.clip_mesh((v, f), o, n, cap=True, extension=(1.0, 2), engine=engine)
    CC.same_as_checker(got, CC.check(v, f, o, n, "below", "loop", True, (1.0, 2)))
    assert got.report["attempts"] == 2 and got.cut_points.tolist() == [400]


def test_empty_inputs_and_open_vessel_ends(engine):
    v, f = CASES["cube_plane_cap"][:2]
    none = mm.clip_mesh((v, f), np.zeros((0, 3)), np.zeros((0, 3)), engine=engine)
    assert none.vertices.tobytes() == v.tobytes() and none.faces.tobytes() == f.tobytes() and none.report["n_launches"] == 0
    empty = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    assert mm.clip_mesh(empty, [[0, 0, 0.0]], [[0, 0, 1.0]], strict=False, engine=engine).cut_status.tolist() == [Y.NO_LOOP]
    assert mm.clip_mesh(empty, [[0, 0, 0.0]], [[0, 0, 1.0]], scope="plane", engine=engine).report["n_vertices"] == 0
    with pytest.raises(mm.ClipError):
        mm.clip_mesh(empty, [[0, 0, 0.0]], [[0, 0, 1.0]], engine=engine)
    cloud = mm.clip_mesh((v, np.zeros((0, 3), dtype=np.int64)), [[0.5, 0, 0]], [[1.0, 0, 0]], scope="plane", engine=engine)
    assert cloud.vertex_origin.tolist() == [0, 1, 2, 3] and cloud.report["n_launches"] == 5 + cloud.report["jump_rounds"] + 1 + 8
    from test_section_host import tube
    tv, tf = tube(12, 41, 1.0, 0.25, jitter=0.01, seed=12)
    xs = np.arange(0.0, 10.01, 0.4) + 0.013
    cl = mm.Centerline.from_contour_points(np.stack([xs, 0 * xs, 0 * xs], 1))
    stations, origins, normals, keep = mm.vessel_end_stations(cl, outlet_mm=1.5, inlet_mm=1.0)
    got = mm.open_vessel_ends((tv, tf), cl, outlet_mm=1.5, inlet_mm=1.0, cap=True, extension=(1.0, 2), engine=engine)
    same = mm.clip_mesh((tv, tf), origins, normals, keep=keep, cap=True, extension=(1.0, 2), engine=engine)
    assert got.report["stations"] == stations.tolist()
    for k in ("vertices", "faces", "vertex_origin", "face_origin", "face_kind"):
        assert getattr(got, k).tobytes() == getattr(same, k).tobytes(), k
    CC.same_as_checker(got, CC.check(tv, tf, origins, normals, keep, "loop", True, (1.0, 2)))
