"""GPU tests of the winding number (csrc/mm_winding_kernels.hip): the device's (turns, p, rho, touch) equal the checker
(tests/mm_checkers/winding_number.py) bit for bit, and w, err and inside are equal, on closed solids, a sphere of 8 192
faces (32 chunks, 16 groups of 2) cut at every size where the grouping changes, an open tube, adversarial queries,
degenerate faces and a shuffled face list; a query's bits do not depend on the other queries of the call nor on what the
engine ran before; and the functions built on it -- signed distance, containment, the intramural course -- on small
nested shapes.  Every shape is small; the checker's results are shared through tests/winding_cases.py."""
import ctypes as C

import numpy as np
import pytest

import multimoda_rs_amd as mm
import winding_cases as wc
from mm_checkers import winding_number as chk

pytestmark = pytest.mark.gpu

RAW = ("turns", "p", "rho", "touch")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_equals(got, want, sel=slice(None)):
    for k in RAW:
        assert _same_bits(getattr(got, k), want[k][sel]), k
    assert _same_bits(got.w, want["w"][sel]) and _same_bits(got.err, want["err"][sel])
    assert _same_bits(got.inside, want["inside"][sel])


@pytest.mark.parametrize("name", wc.BIT_CASES)
def test_device_equals_checker_bit_for_bit(engine, name):
    q, v, f = wc.get(name)
    want = wc.expected(name)
    got = mm.mesh_winding_number(q, (v, f), engine=engine)
    _assert_equals(got, want)
    pl = wc.plan(want["n_staged"])
    r = got.report
    assert r["n_staged_faces"] == want["n_staged"] and r["n_degenerate_faces"] == f.shape[0] - want["n_staged"]
    assert (r["chunk_faces"], r["chunks_per_group"], r["groups"]) == (pl["chunk"], pl["chunks_per_group"], pl["groups"])
    if want["n_staged"]:
        assert r["n_launches"] == 2 and r["items"] == -(-q.shape[0] // 512) * pl["groups"]
        assert r["bytes_scratch"] >= q.shape[0] * pl["groups"] * 32


def test_closed_solids_give_whole_numbers(engine):
    """As tests/test_winding_host.py::test_closed_solids_give_whole_numbers, on the device: exactly 1 inside, exactly -1
    in an inward-oriented solid, exactly 0 outside where the arithmetic is exact (integer distances), within err of 0 at
    a generic outside point."""
    q, v, f = wc.get("octahedron")
    r = mm.mesh_winding_number(q, (v, f), engine=engine)
    assert r.w[[0, 2]].tolist() == [1.0, 1.0] and r.w[[1, 4]].tolist() == [0.0, 0.0]
    assert (r.turns[:5] % 4 == 0).all() and abs(r.w[3]) <= r.err[3] < 1e-13
    assert r.inside.tolist() == [1, 0, 1, 0, 0, -1] and r.touch.tolist() == [False] * 5 + [True]
    q, v, f = wc.get("octahedron_inward")
    r = mm.mesh_winding_number(q, (v, f), engine=engine)
    assert r.w.tolist() == [-1.0, 0.0, -1.0] and r.turns.tolist() == [-4, 0, -4] and r.inside.tolist() == [0, 0, 0]
    assert mm.points_in_mesh(q, (v, f), two_sided=True, engine=engine).tolist() == [1, 0, 1]
    q, v, f = wc.get("tetrahedron")
    r = mm.mesh_winding_number(q, (v, f), engine=engine)
    assert r.w.tolist() == [0.0, 1.0, 0.0] and (r.turns % 4 == 0).all()
    q, v, f = wc.get("tetrahedron_about_origin")
    assert mm.mesh_winding_number(q, (v, f), engine=engine).w.tolist() == [1.0, 0.0, 1.0]


@pytest.mark.parametrize("name", ["sphere8192", "q513cut511"])
@pytest.mark.parametrize("nq", [1, 512, 513])
def test_query_counts_around_a_block(engine, name, nq):
    q, v, f = wc.get(name)
    got = mm.mesh_winding_number(q[:nq], (v, f), engine=engine)
    _assert_equals(got, wc.expected(name), slice(0, nq))
    assert got.report["items"] == (2 if nq == 513 else 1) * got.report["groups"]


def test_open_tube_gives_fractions_within_err_of_the_reference(engine):
    q, v, f = wc.get("tube")
    r = mm.mesh_winding_number(q, (v, f), engine=engine)
    ref = wc.expected_reference("tube")
    assert np.isfinite(r.err).all() and (np.abs(r.w - ref).astype(np.float64) <= r.err).all()
    assert (r.turns % 4 != 0).any()
    assert ((r.w > 1e-3) & (r.w < 1 - 1e-3)).any() and 0.5 < r.w[-4] < r.w[-5] < 1.0 and 0.0 < r.w[-2] < r.w[-3] < 0.5 + 1e-12


@pytest.mark.parametrize("name,mesh,stride", [("adversarial_sphere", "sphere512", 16), ("adversarial_tube", "tube", 18)])
def test_adversarial_queries(engine, name, mesh, stride):
    v, f = getattr(wc, mesh)()
    pts, kind, h = wc.adversarial(v, f, stride)
    r = mm.mesh_winding_number(pts, (v, f), engine=engine)
    ref = wc.expected_reference(name)
    assert r.touch[(kind == 0) & (h == 0.0)].all() and not r.touch[np.abs(h) >= 1e-12].any()
    assert (r.rho[(kind == 2) & (h == 0.0)] == 0.0).all() and not r.touch[kind == 3].any()
    fin = np.isfinite(r.err)
    assert fin[np.abs(h) >= 1e-12].all() and not fin[(kind <= 2) & (h == 0.0)].any()
    gap = np.abs(r.w - ref).astype(np.float64)
    print(name, "largest |w - ref| where err is finite", gap[fin].max(), "largest finite err", r.err[fin].max())
    assert (gap[fin] <= r.err[fin]).all()
    assert (ref[r.inside == 1] > 0.5).all() and (ref[r.inside == 0] < 0.5).all()
    far = mm.point_mesh_distance(pts, (v, f), engine=engine).distance >= 1e-3
    assert far.sum() >= 100
    print(name, "queries 1e-3 or more from every face", int(far.sum()), "largest err", r.err[far].max())
    assert (r.err[far] <= 1e-6).all()


def test_degenerate_faces_do_not_change_a_bit(engine):
    q, v2, f2 = wc.get("degenerate")
    with_them = mm.mesh_winding_number(q, (v2, f2), engine=engine)
    without = mm.mesh_winding_number(q, wc.sphere512(), engine=engine)
    assert with_them.report["n_degenerate_faces"] == 8 and without.report["n_degenerate_faces"] == 0
    for k in RAW + ("w", "err", "inside"):
        assert _same_bits(getattr(with_them, k), getattr(without, k)), k


def test_face_order_moves_w_within_err(engine):
    q = wc.queries513()[:200]
    v, f = wc.sphere512()
    a = mm.mesh_winding_number(q, (v, f), engine=engine)
    b = mm.mesh_winding_number(q, (v, f[np.random.default_rng(3).permutation(f.shape[0])]), engine=engine)
    assert (np.abs(a.w - b.w) <= a.err + b.err).all()
    both = (a.inside >= 0) & (b.inside >= 0)
    assert both.sum() >= 190 and (a.inside[both] == b.inside[both]).all()


def test_a_querys_bits_do_not_depend_on_the_other_queries(engine):
    q, v, f = wc.get("sphere8192")
    want = wc.expected("sphere8192")
    q = q[:300]
    rev = mm.mesh_winding_number(q[::-1].copy(), (v, f), engine=engine)
    _assert_equals(rev, want, slice(299, None, -1))
    for part in (slice(0, 7), slice(7, 300)):
        _assert_equals(mm.mesh_winding_number(q[part], (v, f), engine=engine), want, part)
    twice = mm.mesh_winding_number(np.vstack([q[:20], q[:20]]), (v, f), engine=engine)
    for k in RAW:
        assert _same_bits(getattr(twice, k)[:20], want[k][:20]) and _same_bits(getattr(twice, k)[20:], want[k][:20]), k


def test_stale_partials_never_reach_a_result(engine):
    """a large call (513 queries x 16 groups of partial records), then a small one on the same engine: equal to the
    small one on a fresh engine"""
    q, v, f = wc.get("sphere8192")
    mm.mesh_winding_number(q, (v, f), engine=engine)
    sq, sv, sf = wc.get("cut257")
    after = mm.mesh_winding_number(sq, (sv, sf), engine=engine)
    with mm.Engine() as fresh:
        alone = mm.mesh_winding_number(sq, (sv, sf), engine=fresh)
    for k in RAW + ("w", "err", "inside"):
        assert _same_bits(getattr(after, k), getattr(alone, k)), k
    _assert_equals(after, wc.expected("cut257"))


def test_empty_and_invalid_inputs(engine):
    v, f = wc.box((0, 0, 0), (1, 1, 1))
    q = np.array([[0.5, 0.5, 0.5], [2.0, 0.5, 0.5]])
    none = mm.mesh_winding_number(q, (v, np.zeros((0, 3), dtype=np.int64)), engine=engine)
    flat = mm.mesh_winding_number(q, (v, np.array([[0, 0, 1], [2, 2, 2]])), engine=engine)
    for r in (none, flat):
        assert r.w.tolist() == [0.0, 0.0] and r.err.tolist() == [0.0, 0.0] and r.inside.tolist() == [0, 0]
        assert r.turns.tolist() == [0, 0] and r.report["n_launches"] == 0 and r.report["n_staged_faces"] == 0
    empty = mm.mesh_winding_number(np.zeros((0, 3)), (v, f), engine=engine)
    assert empty.w.shape == (0,) and empty.inside.shape == (0,) and empty.p.shape == (0, 2) and empty.report["n_launches"] == 0
    assert mm.mesh_winding_number(q, (v, f), engine=engine).inside.tolist() == [1, 0]
    bad = f.copy()
    bad[5, 0] = 8
    for call in (lambda: mm.mesh_winding_number(q, (v, bad), engine=engine),
                 lambda: mm.mesh_winding_number(q * np.nan, (v, f), engine=engine),
                 lambda: mm.mesh_winding_number(q, (v * 2.0 ** 301, f), engine=engine),
                 lambda: mm.signed_point_mesh_distance(q * np.inf, (v, f), engine=engine)):
        with pytest.raises(ValueError):
            call()
    # the C entry point refuses the same before any launch and writes nothing
    N = mm._native
    n, p, rho, touch = (np.full(2, -7, dtype=np.int32), np.full((2, 2), 7.5), np.full(2, 7.5), np.full(2, 0xA5, dtype=np.uint8))
    rep = N.MMWindingReport()
    big = v * 2.0 ** 301
    for vv, ff, msg in ((v, bad, "face index out of range"), (big, f, "vertex coordinate above 2^300")):
        rc = N.lib().mm_mesh_winding(engine.handle, N._ptr(vv), 8, N._ptr(ff), 12, N._ptr(q), 2, N._ptr(n), N._ptr(p),
                                     N._ptr(rho), N._ptr(touch), C.byref(rep))
        assert rc == -2 and N.last_error() == "mm_mesh_winding: " + msg
        assert (n == -7).all() and (p == 7.5).all() and (rho == 7.5).all() and (touch == 0xA5).all()


def test_signed_distance_on_the_sphere(engine):
    q, v, f = wc.get("sphere8192")
    r = np.sqrt((q * q).sum(axis=1))
    clear = np.abs(r - 1.0) > 0.01                       # the inscribed mesh lies within 0.002 of the unit sphere
    s = mm.signed_point_mesh_distance(q, (v, f), engine=engine)
    d = mm.point_mesh_distance(q, (v, f), engine=engine)
    assert clear.sum() > 450 and (s.sign[clear] == np.sign(r[clear] - 1.0)).all()
    assert _same_bits(s.distance, d.distance) and _same_bits(s.face, d.face) and _same_bits(s.closest, d.closest)
    assert (s.sign != 0).all() and _same_bits(np.abs(s.signed_distance), d.distance)
    assert _same_bits(s.winding.inside, wc.expected("sphere8192")["inside"])


def test_mesh_containment(engine):
    v, f = wc.sphere512()
    inner = mm.mesh_containment((0.5 * v, f), (v, f), engine=engine)
    assert inner.contained and inner.n_inside == inner.n_samples == 3 * f.shape[0] and inner.worst_outside.sample == -1
    assert 0.4 < inner.deepest_inside.distance < 0.5 + 1e-12
    shifted = (0.5 * v + np.array([0.8, 0.0, 0.0]), f)
    r = mm.mesh_containment(shifted, (v, f), samples=2, engine=engine)
    assert r.n_inside > 0 and r.n_outside > 0 and not r.contained and r.n_inside + r.n_outside + r.n_undecided == r.n_samples
    pts, owner = mm.sample_mesh_surface(shifted, 2)
    d = mm.point_mesh_distance(pts, (v, f), engine=engine)
    out = np.flatnonzero(r.inside == 0)
    k = int(out[np.argmax(d.sq_distance[out])])
    w = r.worst_outside
    assert (w.sample, w.sample_face, w.face) == (k, int(owner[k]), int(d.face[k]))
    assert w.distance == d.distance[k] and _same_bits(w.closest, d.closest[k]) and 0.29 < w.distance < 0.35
    # an open tube inside a wider open tube: every sample away from the ends is inside
    thin, wide = wc.tube(radius=0.3), wc.tube(radius=0.5)
    r = mm.mesh_containment(thin, wide, engine=engine)
    pts, _ = mm.sample_mesh_surface(thin, 1)
    assert (r.inside[np.abs(pts[:, 2]) <= 0.5] == 1).all() and r.n_inside < r.n_samples


def test_intramural_course(engine):
    lumen, wall = wc.box((-1, -1, -1), (1, 1, 1)), wc.box((-2, -2, -2), (2, 2, 2))
    line = np.array([[-3.1 + 0.25 * k, 0.1, 0.2] for k in range(14)])          # from outside through the wall into the lumen
    r = mm.intramural_course(line, lumen, wall, engine=engine)
    in_wall = chk.winding(line, *wall, wc.plan)["inside"] == 1
    in_lumen = chk.winding(line, *lumen, wc.plan)["inside"] == 0
    want = chk.first_run(in_wall & in_lumen, line)
    assert r.intramural.tolist() == [(-2 < x < -1) for x in line[:, 0]] and r.intramural.sum() == 4
    assert (r.start, r.end, r.length) == want and r.start == 5 and r.end == 8 and abs(r.length - 0.75) < 1e-12
    assert not r.points.undecided.any()
    never = mm.intramural_course(line + np.array([0.0, 5.0, 0.0]), lumen, wall, engine=engine)
    assert (never.start, never.end, never.length) == (-1, -1, 0.0) and not never.intramural.any()
