"""Mesh intersections on the device (csrc/mm_intersect_kernels.hip, csrc/mm_intersect.cpp) against the checker
(tests/mm_checkers/mesh_intersections.py): equal face flags, pairs, pair states and counts, and equal report integers
(items before the cull, launches, bytes), bit for bit.  Cases: the known single pairs, two jittered octahedra (with the
exact oracle), a jittered tube as it comes and with a ring pushed through its wall, one face past a chunk, two long tubes
in both forms (culling must happen and lose nothing), shuffled faces, a pair cap below the count, a small call behind a
large one, empty meshes, the argument checks, and stitch(..., check_intersections=True)."""
import ctypes as C

import numpy as np
import pytest

from mm_checkers import mesh_intersections as X
from test_trim_host import octahedron
from test_intersect_host import I, KNOWN, T, checked, known_mesh, oracle
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID = -2
COUNTS = ("n_intersecting_pairs", "n_undecided_pairs", "n_coincident_pairs", "n_degenerate_faces", "narrow_tests")


def same_as_checker(got, want, nfa, nfb, self_form, max_pairs=1 << 20):
    n_pairs = len(want["pairs"])
    if self_form:
        assert got.face_state.dtype == np.uint8 and np.array_equal(got.face_state, want["face_state"])
    else:
        for g, w in zip(got.face_state, want["face_state"]):
            assert g.dtype == np.uint8 and np.array_equal(g, w)
    if n_pairs <= max_pairs:
        assert got.pairs.dtype == np.int64 and got.pairs.shape == (n_pairs, 2) and np.array_equal(got.pairs, want["pairs"])
        assert got.pair_state.dtype == np.int8 and np.array_equal(got.pair_state, want["pair_state"])
    else:
        assert got.pairs is None and got.pair_state is None
    for k in COUNTS:
        assert got.report[k] == want[k], (k, got.report[k], want[k])
    rep = X.predict_report(nfa, nfb, got.report["items"], n_pairs, max_pairs, self_form)
    for k, n in rep.items():
        assert got.report[k] == n, (k, got.report[k], n)
    assert 0 <= got.report["items"] <= got.report["items_total"]
    assert got.report["narrow_tests"] <= got.report["pair_box_tests"]
    return got


def self_case(name, engine, **kw):
    (v, f), want = checked(name)
    return same_as_checker(mm.mesh_self_intersections((v, f), engine=engine, **kw), want, len(f), 0, True, **kw)


def two_case(name, engine, **kw):
    (va, fa, vb, fb), want = checked(name)
    got = mm.mesh_intersections((va, fa), (vb, fb), engine=engine, **kw)
    return same_as_checker(got, want, len(fa), len(fb), False, **kw)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(engine, name):
    v, f = known_mesh(name)
    want = KNOWN[name][3]
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 2, 0, True)
    assert got.face_state.tolist() == [want, want] and got.report["n_coincident_pairs"] == (name == "coincident")
    if KNOWN[name][2] is None:                                            # no shared vertex: the two-mesh form as well
        t1, t2 = KNOWN[name][:2]
        v1, v2, f1 = np.array(t1), np.array(t2), np.array([[0, 1, 2]])
        got = same_as_checker(mm.mesh_intersections((v1, f1), (v2, f1), engine=engine), X.scan_two(v1, f1, v2, f1), 1, 1, False)
        assert got.face_state[0].tolist() == [want] and got.face_state[1].tolist() == [want]


def test_equal_coordinates_and_degenerate_faces(engine):
    t1, t2 = KNOWN["edge_dihedral"][:2]
    v = np.array(t1 + t2)
    v[3, 1] = -0.0
    f = np.array([[0, 1, 2], [3, 4, 5]])
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 2, 0, True)
    assert got.pairs.shape == (0, 2) and got.report["narrow_tests"] == 1  # an unwelded seam reads as adjacent
    v, f = known_mesh("crossing")
    v = np.concatenate([v, [[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]]])
    f = np.concatenate([f, [[6, 7, 8], [0, 1, 1]]])
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 4, 0, True)
    assert got.report["n_degenerate_faces"] == 2 and got.face_state.tolist() == [1, 1, 0, 0]


def test_jittered_octahedra(engine):
    got = two_case("general_octahedra", engine)
    va, fa, vb, fb = checked("general_octahedra")[0]
    assert got.report["n_undecided_pairs"] == 0 and got.report["pair_box_tests"] == 64
    want = sorted((i, j) for i in range(8) for j in range(8) if oracle(T(*va[fa[i]]), T(*vb[fb[j]])))
    assert got.pairs.tolist() == [list(p) for p in want] and len(want) > 0


def test_jittered_tube_as_it_comes_and_pushed_through_its_wall(engine):
    got = self_case("general_tube", engine)
    assert got.report["n_intersecting_pairs"] == 0 and got.report["n_undecided_pairs"] == 0 and not got.face_state.any()
    got = self_case("pushed_tube", engine)
    assert got.report["n_intersecting_pairs"] > 0 and got.report["n_undecided_pairs"] == 0
    assert got.report["items"] == got.report["items_total"] == 3          # 510 faces: chunks I == I, I < J and a tail


def test_one_face_past_a_chunk(engine):
    got = self_case("random_257", engine)
    assert got.report["items_total"] == 3 and got.report["n_intersecting_pairs"] > 0
    assert self_case("random_256", engine).report["items_total"] == 1
    got = self_case("random_1", engine)
    assert got.report["pair_box_tests"] == 0 and got.report["n_launches"] == 2 and got.pairs.shape == (0, 2)


def test_long_tubes_are_culled_and_lose_nothing(engine):
    two = two_case("shifted_long_tubes", engine)
    assert two.report["items"] < two.report["items_total"] == 16 and two.report["n_intersecting_pairs"] > 0
    one = self_case("both_long_tubes", engine)
    assert one.report["items"] < one.report["items_total"] == 36
    nf = len(checked("shifted_long_tubes")[0][1])
    crossing = one.pairs[one.pair_state == I]
    between = crossing[(crossing[:, 0] < nf) & (crossing[:, 1] >= nf)]
    assert np.array_equal(between - [0, nf], two.pairs[two.pair_state == I])


def test_shuffled_faces_give_the_same_pairs(engine):
    (v, f), want = checked("pushed_tube")
    perm = np.random.default_rng(9).permutation(len(f))
    got = mm.mesh_self_intersections((v, f[perm]), engine=engine)
    back = np.sort(perm[got.pairs], axis=1)
    order = np.lexsort((back[:, 1], back[:, 0]))
    assert np.array_equal(back[order], want["pairs"]) and np.array_equal(got.pair_state[order], want["pair_state"])
    assert np.array_equal(got.face_state, want["face_state"][perm])
    for k in COUNTS:
        assert got.report[k] == want[k]


def test_max_pairs_below_the_count(engine):
    full = self_case("pushed_tube", engine)
    n = len(full.pairs)
    assert n > 2
    got = self_case("pushed_tube", engine, max_pairs=n - 1)
    assert got.pairs is None and got.pair_state is None and got.report["pairs_complete"] is False
    assert np.array_equal(got.face_state, full.face_state)
    for k in COUNTS:
        assert got.report[k] == full.report[k]
    exact = self_case("pushed_tube", engine, max_pairs=n)
    assert exact.report["pairs_complete"] is True and np.array_equal(exact.pairs, full.pairs)
    none = self_case("pushed_tube", engine, max_pairs=0)
    assert none.pairs is None and none.report["n_intersecting_pairs"] == full.report["n_intersecting_pairs"]


def test_a_small_call_behind_a_large_one(engine):
    self_case("both_long_tubes", engine)                                  # leaves flags, counters and pairs behind
    small = self_case("general_tube", engine)
    v, f = known_mesh("apart_by_plane")
    after = mm.mesh_self_intersections((v, f), engine=engine)
    fresh_engine = mm.Engine()
    try:
        fresh = mm.mesh_self_intersections((v, f), engine=fresh_engine)
        fresh_tube = mm.mesh_self_intersections(checked("general_tube")[0], engine=fresh_engine)
    finally:
        fresh_engine.close()
    for a, b in ((after, fresh), (small, fresh_tube)):
        assert np.array_equal(a.face_state, b.face_state) and np.array_equal(a.pairs, b.pairs) and a.report == b.report


def test_empty_meshes(engine):
    v, f = octahedron()
    none = np.zeros((0, 3), dtype=np.int64)
    got = same_as_checker(mm.mesh_self_intersections((v, none), engine=engine), X.scan(v, none), 0, 0, True)
    assert got.face_state.shape == (0,) and got.pairs.shape == (0, 2) and got.report["n_launches"] == 0
    got = same_as_checker(mm.mesh_intersections((v, f), (v, none), engine=engine), X.scan_two(v, f, v, none), 8, 0, False)
    assert got.face_state[0].shape == (8,) and got.face_state[1].shape == (0,) and got.report["items"] == 0
    got = same_as_checker(mm.mesh_intersections((np.zeros((0, 3)), none), (v, f), engine=engine),
                          X.scan_two(np.zeros((0, 3)), none, v, f), 0, 8, False)
    assert got.report["n_launches"] == 0 and got.report["bytes_uploaded"] == 0
    far = mm.mesh_intersections((v, f), (v + 10.0, f), engine=engine)     # faces, but no item: nothing launched
    assert far.report["items"] == 0 and far.report["items_total"] == 1 and far.report["n_launches"] == 0
    assert not far.face_state[0].any() and far.pairs.shape == (0, 2)


def _raw(handle, va, fa, vb=None, fb=None, max_pairs=4, **size):
    va, fa = np.ascontiguousarray(va, dtype=np.float64), np.ascontiguousarray(fa, dtype=np.int64)
    two = vb is not None
    if two:
        vb, fb = np.ascontiguousarray(vb, dtype=np.float64), np.ascontiguousarray(fb, dtype=np.int64)
    out = (np.full(max(len(fa), 1), 77, dtype=np.uint8), np.full(max(len(fb), 1) if two else 1, 77, dtype=np.uint8),
           np.full((4, 2), -77, dtype=np.int64), np.full(4, 77, dtype=np.int8))
    rep = (C.c_uint8 * C.sizeof(N.MMIntersectReport))(*([0x5A] * C.sizeof(N.MMIntersectReport)))
    rc = N.lib().mm_mesh_intersections(handle, N._ptr(va), size.get("nva", len(va)), N._ptr(fa), size.get("nfa", len(fa)),
                                       N._ptr(vb) if two else None, size.get("nvb", len(vb) if two else 0),
                                       N._ptr(fb) if two else None, size.get("nfb", len(fb) if two else 0), max_pairs,
                                       *(N._ptr(a) for a in out), C.cast(rep, C.POINTER(N.MMIntersectReport)))
    untouched = all((a == (-77 if a.dtype == np.int64 else 77)).all() for a in out)
    return rc, untouched and (np.frombuffer(rep, dtype=np.uint8) == 0x5A).all()


def test_invalid_arguments(engine):
    v, f = octahedron()
    bad_v, bad_f = v.copy(), f.copy()
    bad_v[5, 1], bad_f[7, 2] = np.inf, 6
    unused = np.concatenate([v, [[np.nan, 0.0, 0.0]]])                    # a vertex no face uses is checked too
    h = engine.handle
    for args, err in (((h, bad_v, f), "non-finite vertex coordinate"), ((h, unused, f), "non-finite vertex coordinate"),
                      ((h, v, bad_f), "face index out of range"), ((h, v, -f), "face index out of range"),
                      ((h, v, f, bad_v, f), "non-finite vertex coordinate"), ((h, v, f, v, bad_f), "face index out of range")):
        rc, untouched = _raw(*args)
        assert rc == MM_ERR_INVALID and N.last_error() == "mm_mesh_intersections: " + err and untouched, err
    for kw in ({"nfa": 2 ** 31}, {"nva": 2 ** 31}, {"nfa": -1}, {"max_pairs": -1}):   # rejected before anything is read
        rc, untouched = _raw(h, v, f, **kw)
        assert rc == MM_ERR_INVALID and untouched, kw
    rc, untouched = _raw(h, v, f, v, f, nfb=2 ** 31)
    assert rc == MM_ERR_INVALID and N.last_error() == "mm_mesh_intersections: nv, nf and nq must stay below 2^31" and untouched
    rc, untouched = _raw(None, v, f)
    assert rc == MM_ERR_INVALID and N.last_error() == "engine == NULL" and untouched
    with pytest.raises(ValueError, match="out of range"):
        mm.mesh_self_intersections((v, bad_f), engine=engine)
    with pytest.raises(RuntimeError, match="mm_mesh_intersections: non-finite vertex coordinate"):
        mm.mesh_intersections((v, f), (bad_v, f), engine=engine)
    rep = N.MMIntersectReport()                                           # the pair outputs are nullable: counts only
    state = np.zeros(8, dtype=np.uint8)
    assert N.lib().mm_mesh_intersections(h, N._ptr(v), 6, N._ptr(f), 8, None, 0, None, 0, 100, N._ptr(state), None, None,
                                         None, C.byref(rep)) == 0
    assert rep.n_intersecting_pairs == 0 and rep.n_undecided_pairs == 0 and rep.pairs_complete == 1


def test_stitch_reports_the_self_check_of_its_result(engine):
    res, geom, frames = takeoff_case(engine)
    plain = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    out = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, check_intersections=True)
    assert "intersection_report" not in plain and set(out) == set(plain) | {"intersection_report"}
    for a, b in zip(mm.ccta._mesh_parts(plain["mesh"]), mm.ccta._mesh_parts(out["mesh"])):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert plain["stitch_report"] == out["stitch_report"] and plain["fill_report"] == out["fill_report"]
    check = mm.mesh_self_intersections(out["mesh"], engine=engine)
    assert out["intersection_report"] == check.report and check.report["narrow_tests"] > 0
    print("stitched take-off:", check.report)
