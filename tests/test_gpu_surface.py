"""Surface distance on the device (csrc/mm_tri_kernels.hip, csrc/mm_surface.cpp) against the checker
(tests/mm_checkers/surface_distance.py): bit-identical squared distances and closest points, equal faces and regions,
equal integer report fields (items, launches, bytes).  Cases: the seven regions, the small solids, the ties, the
degenerate faces, one face past a chunk and one query past a block, a long tube whose pass B must skip items, an equal
distance in a chunk that pass B skips, shuffled faces, random meshes, empty inputs, the argument checks; then surface_distance, and the line label -> remove ->
stitch(fill_holes=True, refine=True, smooth=True) measured against its unrefined, unsmoothed self."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import surface_distance as S
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, jitter, wound_tube
from test_surface_host import (ACCURACY_TOL, REGION_QUERIES, REGIONS, TRIANGLE, degenerate_faces,
                               far_face_touching_the_first_chunk, long_tube, must_skip, two_coplanar)
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import surface

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID = -2
QPB, CHUNK = 512, 256


def same_as_checker(points, v, f, engine):
    got = mm.point_mesh_distance(points, (v, f), engine=engine)
    sq, face, closest, region = S.scan(points, v, f)
    assert same_bits(got.sq_distance, sq) and same_bits(got.distance, np.sqrt(sq))
    assert got.face.dtype == np.int64 and np.array_equal(got.face, face)
    assert same_bits(got.closest, closest)
    assert got.region.dtype == np.int32 and np.array_equal(got.region, region)
    want = S.predict_report(len(np.reshape(points, (-1, 3))), len(f), QPB, CHUNK)
    for k, n in want.items():
        assert got.report[k] == n, (k, got.report[k], n)
    assert 0 <= got.report["items_skipped"] <= got.report["items_pass_b"]
    return got


def test_the_seven_regions(engine):
    got = same_as_checker(REGION_QUERIES, *TRIANGLE, engine)
    assert got.region.tolist() == REGIONS and got.report["n_launches"] == 4 and got.report["items_pass_a"] == 1


@pytest.mark.parametrize("solid", [tetrahedron, octahedron])
def test_small_solids(engine, solid):
    v, f = solid()
    rng = np.random.default_rng(11)
    p = np.concatenate([rng.uniform(-3.5, 3.5, (300, 3)), v, mm.sample_mesh_surface((v, f), 3)[0]])
    same_as_checker(p, v, f, engine)
    same_as_checker(p, jitter(v, 1), f, engine)


def test_ties_and_degenerate_faces(engine):
    v, f = two_coplanar()
    q = np.array([[1.0, 1.0, 3.0], [0.5, 1.5, 1.0], [1.5, 0.5, -2.0]])
    assert (same_as_checker(q, v, f, engine).face == 0).all() and (same_as_checker(q, v, f[::-1], engine).face == 0).all()
    v, f = octahedron()
    q = np.array([[-0.4, -0.3, 0.9]])
    assert same_as_checker(q, v, f, engine).face.tolist() == [2]
    assert same_as_checker(q, v, np.concatenate([f[[2]], f, f[[2]]]), engine).face.tolist() == [0]
    v, f, q = degenerate_faces()
    got = same_as_checker(q, v, f, engine)
    assert got.face.tolist() == [0, 0, 2, 2, 0, 2] and np.isfinite(got.sq_distance).all()
    for k in range(4):
        got = same_as_checker(q, v, f[[k]], engine)
        assert np.isfinite(got.closest).all() and set(got.region.tolist()) <= {4, 5, 6}


def test_one_face_past_a_chunk_and_one_query_past_a_block(engine):
    rng = np.random.default_rng(257)
    v = rng.uniform(-3.0, 3.0, (90, 3))
    f = rng.integers(0, 90, (CHUNK + 1, 3))
    p = rng.uniform(-3.5, 3.5, (QPB + 1, 3))
    got = same_as_checker(p, v, f, engine)
    assert got.report["items_pass_a"] == 2 and got.report["items_pass_b"] == 2 and got.report["n_launches"] == 5
    for nf, nq in ((CHUNK, QPB), (CHUNK + 1, QPB), (CHUNK, QPB + 1), (1, 1)):
        same_as_checker(p[:nq], v, f[:nf], engine)


def test_long_tube_skips_what_the_plan_says_it_must(engine):
    v, f, moved = long_tube()
    fine = mm.refine_mesh((moved, f), 0.6, engine=engine)[0][0]
    plan = surface.tri_plan(fine, (v, f))
    assert len(f) > 3 * CHUNK and len(fine) > 2 * QPB
    n = must_skip(plan, fine, v, f)
    got = same_as_checker(fine, v, f, engine)                             # the checker's scan is unpruned
    print(f"long tube: pass B {got.report['items_pass_b']} items, skipped {got.report['items_skipped']}, must_skip {n}")
    assert got.report["items_skipped"] >= n > 0


def test_an_equal_distance_in_a_chunk_pass_b_skips_still_wins_on_face_index(engine):
    """Every minimum of the one query block is 0 after pass A, so pass B skips both its items (lb2 >= 0), the far chunk
    with bound 0.0 among them; the who pass must still run that chunk (lb2 > 0 is false): face 0, staged there, touches
    the first query and has the lowest index.  The layout is checked on the host in tests/test_surface_host.py."""
    v, f, q = far_face_touching_the_first_chunk()
    got = same_as_checker(q, v, f, engine)
    assert got.face.tolist() == [0, 6, 101] and (got.sq_distance == 0.0).all()
    assert got.report["items_pass_a"] == 1 and got.report["items_pass_b"] == 2 and got.report["items_skipped"] == 2


def test_shuffled_faces(engine):
    rng = np.random.default_rng(9)
    v, f = wound_tube(15, 17)
    v = jitter(v, 17)
    p = rng.uniform(v.min(axis=0), v.max(axis=0), (600, 3))
    base = same_as_checker(p, v, f, engine)
    perm = rng.permutation(len(f))
    other = same_as_checker(p, v, f[perm], engine)
    assert same_bits(base.sq_distance, other.sq_distance)
    unique = (S.pair_sq(p, v, f) == base.sq_distance[None, :]).sum(axis=0) == 1
    assert unique.sum() > 300 and np.array_equal(perm[other.face[unique]], base.face[unique])
    assert same_bits(base.closest[unique], other.closest[unique])


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), nv=st.integers(1, 40), nf=st.integers(0, 50), nq=st.integers(0, 60),
       lattice=st.booleans())
def test_random_small_meshes(engine, seed, nv, nf, nq, lattice):
    r = np.random.default_rng(seed)
    # lattice coordinates make exact ties, collinear corners and coincident vertices common
    v = r.integers(-2, 3, (nv, 3)).astype(np.float64) if lattice else r.uniform(-3, 3, (nv, 3))
    p = r.integers(-3, 4, (nq, 3)) * 0.5 if lattice else r.uniform(-4, 4, (nq, 3))
    same_as_checker(p, v, r.integers(0, nv, (nf, 3)), engine)


def test_empty_inputs(engine):
    v, f = octahedron()
    none = np.zeros((0, 3), dtype=np.int64)
    got = same_as_checker(REGION_QUERIES, v, none, engine)
    assert (got.sq_distance == np.inf).all() and (got.face == -1).all() and np.isnan(got.closest).all()
    assert (got.region == -1).all() and got.report["n_launches"] == 0 and got.report["bytes_uploaded"] == 0
    got = same_as_checker(np.zeros((0, 3)), v, f, engine)
    assert got.sq_distance.shape == (0,) and got.closest.shape == (0, 3) and got.report["n_launches"] == 0
    rep = mm.surface_distance((v, f), (v, none), engine=engine)
    assert rep.a_to_b.max == np.inf and rep.b_to_a.n == 0 and np.isnan(rep.b_to_a.max) and rep.hausdorff == np.inf


def _raw(handle, v, f, q, nv=None, nf=None, nq=None):
    v, f, q = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64), np.ascontiguousarray(q)
    n = max(len(q), 1)
    out = (np.full(n, 7.5), np.full(n, -77, dtype=np.int64), np.full((n, 3), 7.5), np.full(n, -77, dtype=np.int32))
    rep = (C.c_uint8 * C.sizeof(N.MMSurfaceReport))(*([0x5A] * C.sizeof(N.MMSurfaceReport)))
    rc = N.lib().mm_point_mesh_distance(handle, N._ptr(v), len(v) if nv is None else nv, N._ptr(f), len(f) if nf is None else nf,
                                        N._ptr(q), len(q) if nq is None else nq, *(N._ptr(a) for a in out),
                                        C.cast(rep, C.POINTER(N.MMSurfaceReport)))
    untouched = (out[0] == 7.5).all() and (out[1] == -77).all() and (out[2] == 7.5).all() and (out[3] == -77).all()
    return rc, untouched and (np.frombuffer(rep, dtype=np.uint8) == 0x5A).all()


def test_invalid_arguments(engine):
    v, f = octahedron()
    q = REGION_QUERIES
    bad_v, bad_q, bad_f = v.copy(), q.copy(), f.copy()
    bad_v[5, 1], bad_q[6, 2], bad_f[7, 2] = np.inf, np.nan, 6
    unused = np.concatenate([v, [[np.nan, 0.0, 0.0]]])                    # a vertex no face uses is checked too
    h = engine.handle
    for args, err in (((h, bad_v, f, q), "non-finite vertex coordinate"), ((h, unused, f, q), "non-finite vertex coordinate"),
                      ((h, v, f, bad_q), "non-finite query coordinate"), ((h, v, bad_f, q), "face index out of range"),
                      ((h, v, -f, q), "face index out of range")):
        rc, untouched = _raw(*args)
        assert rc == MM_ERR_INVALID and N.last_error() == "mm_point_mesh_distance: " + err and untouched
    for kw in ({"nq": 2 ** 31}, {"nf": 2 ** 31}, {"nv": 2 ** 31}, {"nq": -1}):   # rejected before anything is read
        rc, untouched = _raw(h, v, f, q, **kw)
        assert rc == MM_ERR_INVALID and untouched, kw
    rc, untouched = _raw(None, v, f, q)
    assert rc == MM_ERR_INVALID and N.last_error() == "engine == NULL" and untouched
    rep = N.MMSurfaceReport()
    sq = np.zeros(len(q))
    assert N.lib().mm_point_mesh_distance(h, N._ptr(v), 6, N._ptr(f), 8, N._ptr(q), len(q), N._ptr(sq), None, None, None,
                                          C.byref(rep)) == 0                 # the other outputs are nullable
    assert same_bits(sq, S.scan(q, v, f)[0])
    assert N.lib().mm_point_mesh_distance(h, N._ptr(v), 6, N._ptr(f), 8, N._ptr(q), len(q), None, None, None, None,
                                          C.byref(rep)) == MM_ERR_INVALID


# ---- surface_distance ----------------------------------------------------------------------------------------------------

def diagonal(*meshes):
    pts = np.concatenate([m[0] for m in meshes])
    return float(np.sqrt(((pts.max(axis=0) - pts.min(axis=0)) ** 2).sum()))


def test_a_mesh_against_itself_and_against_its_refinement(engine):
    v, f = wound_tube(15, 17)
    v = jitter(v, 17)
    rep = mm.surface_distance((v, f), (v, f), engine=engine)
    assert rep.hausdorff == 0.0 and rep.a_to_b.mean == 0.0 and rep.b_to_a.rms == 0.0 and rep.a_to_b.argmax == 0
    fine, _, _ = mm.refine_mesh((v, f), 0.4, engine=engine)
    assert len(fine[0]) > len(v)
    rep = mm.surface_distance((v, f), fine, engine=engine)
    assert rep.a_to_b.max == 0.0                                          # old vertices keep their bits
    assert 0.0 <= rep.b_to_a.max <= ACCURACY_TOL * diagonal((v, f))       # midpoints lie on the old faces
    assert rep.hausdorff == rep.b_to_a.max
    rep3 = mm.surface_distance((v, f), fine, samples=3, engine=engine)
    assert rep3.a_to_b.n == 10 * len(f) and rep3.b_to_a.n == 10 * len(fine[1]) and rep3.hausdorff < 1e-12


def test_translated_octahedron(engine):
    v, f = octahedron()
    moved = v + [0.5, 0.0, 0.0]
    rep = mm.surface_distance((v, f), (moved, f), engine=engine)
    tol = ACCURACY_TOL * diagonal((v, f), (moved, f))
    # the vertex (-1, 0, 0) is 0.5 from the moved vertex (-0.5, 0, 0); the moved vertex (1.5, 0, 0) 0.5 from (1, 0, 0)
    assert abs(rep.a_to_b.max - 0.5) <= tol and abs(rep.b_to_a.max - 0.5) <= tol and abs(rep.hausdorff - 0.5) <= tol
    pa, oa = mm.sample_mesh_surface((v, f))
    assert pa[rep.a_to_b.argmax].tolist() == [-1.0, 0.0, 0.0] and np.abs(rep.a_to_b.closest - [-0.5, 0.0, 0.0]).max() <= tol
    assert oa[rep.a_to_b.argmax] == rep.a_to_b.sample_face
    # the vertex (0, 1, 0) is nearest to the moved edge (0.5, 1, 0) - (-0.5, 0, 0) in its own plane z = 0: the distance
    # from (-0.5, 1) to the line y - x = 1 of the unmoved frame, 0.5 / sqrt(2)
    d = mm.point_mesh_distance([[0.0, 1.0, 0.0]], (moved, f), engine=engine)
    assert abs(d.distance[0] - 0.5 / np.sqrt(2.0)) <= tol and d.region[0] in (4, 5, 6)
    assert rep.n_launches == rep.a_to_b.report["n_launches"] + rep.b_to_a.report["n_launches"] == 8


def test_both_directions_are_two_point_mesh_distance_calls(engine):
    v, f = wound_tube(15, 17)
    a = (jitter(v, 3), f)
    b = mm.refine_mesh((jitter(v, 4), f), 0.5, engine=engine)[0]
    rep = mm.surface_distance(a, b, samples=2, engine=engine)
    for d, (src, dst) in ((rep.a_to_b, (a, b)), (rep.b_to_a, (b, a))):
        p, owner = mm.sample_mesh_surface(src, 2)
        r = mm.point_mesh_distance(p, dst, engine=engine)
        k = int(np.argmax(r.sq_distance))
        assert d.n == len(p) and d.argmax == k and d.face == r.face[k] and d.sample_face == owner[k]
        assert same_bits(d.max, r.distance[k]) and same_bits(d.closest, r.closest[k])
        total, total_sq = 0.0, 0.0
        for x, y in zip(r.distance.tolist(), r.sq_distance.tolist()):     # in index order
            total, total_sq = total + x, total_sq + y
        assert same_bits(d.mean, total / len(p)) and same_bits(d.rms, np.sqrt(total_sq / len(p)))
        assert d.report == r.report
    assert rep.hausdorff == max(rep.a_to_b.max, rep.b_to_a.max) > 0.0
    assert rep.bytes_uploaded == rep.a_to_b.report["bytes_uploaded"] + rep.b_to_a.report["bytes_uploaded"]
    assert rep.bytes_downloaded == rep.a_to_b.report["bytes_downloaded"] + rep.b_to_a.report["bytes_downloaded"]


# ---- the line label -> remove -> stitch ---------------------------------------------------------------------------------

def test_stitched_mesh_against_its_refined_and_smoothed_self(engine):
    res, geom, frames = takeoff_case(engine)
    before = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    after = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=True,
                      smooth=True)
    rep = mm.surface_distance(before, after, engine=engine)
    for d in (rep.a_to_b, rep.b_to_a):
        assert np.isfinite([d.max, d.mean, d.rms]).all() and np.isfinite(d.closest).all() and d.face >= 0
        assert 0.0 <= d.mean <= d.rms <= d.max
    assert rep.hausdorff == max(rep.a_to_b.max, rep.b_to_a.max) > 0.0
    # every vertex of `after` is a vertex of the refined mesh, which lies on `before` (old vertices, and midpoints of its
    # edges), moved by the smoothing by at most its largest displacement
    moved = float(np.sqrt(after["smooth_report"]["max_displacement_sq"]))
    assert rep.b_to_a.max <= moved + ACCURACY_TOL * diagonal(before["mesh"], after["mesh"])
