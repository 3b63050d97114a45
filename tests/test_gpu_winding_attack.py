"""GPU tests of the winding number on worst cases (tests/winding_attack_cases.py): the device equals the checker bit for bit
on ulp ladders through face planes, on queries where the f64 sign of num is wrong, on lattices with exact contact, on
covers with |w| > 1, on the boundaries of `cone` and at coordinates scaled by 2^-299 ... 2^298 -- the first runs of
k_wind_partial's sqrt, division, frexp and ldexp at these exponents and with subnormal intermediate products; the
proofs hold on the device's own output; and the functions built on it answer "undecided" at exact contact.  Every call
is at most 512 faces and 75 000 queries; the checker's results are shared through the case module."""
import numpy as np
import pytest

import multimoda_rs_amd as mm
import winding_attack_cases as ac
import winding_cases as wc

pytestmark = pytest.mark.gpu

ARRAYS = ("turns", "p", "rho", "touch", "w", "err", "inside")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _run(engine, name):
    q, v, f = ac.get(name)
    return mm.mesh_winding_number(q, (v, f), engine=engine)


def _as_dict(r):
    return {k: getattr(r, k) for k in ARRAYS}


def _assert_equals(got, want):
    for k in ARRAYS:
        assert _same_bits(getattr(got, k), want[k]), k


@pytest.mark.parametrize("name", ac.DEVICE_CASES)
def test_device_equals_checker_bit_for_bit(engine, name):
    q, v, f = ac.get(name)
    want = ac.expected(name)
    got = _run(engine, name)
    _assert_equals(got, want)
    pl = wc.plan(want["n_staged"])
    r = got.report
    assert r["n_staged_faces"] == want["n_staged"] and r["n_degenerate_faces"] == f.shape[0] - want["n_staged"]
    assert (r["chunk_faces"], r["chunks_per_group"], r["groups"]) == (pl["chunk"], pl["chunks_per_group"], pl["groups"])
    assert r["n_launches"] == 2 and r["items"] == -(-q.shape[0] // 512) * pl["groups"]
    assert r["bytes_scratch"] >= q.shape[0] * pl["groups"] * 32


def test_single_faces_of_the_wrong_sign_grid_and_the_cone_ties(engine):
    """In the merged grid every query is within a few ulp of all 24 planes and `touch` is the OR over them; against its
    own face alone a query's touch bit is that face's, which is where a touch constant too small on the device would
    show.  The cone ties likewise: merged, the quarter turns of one face cancel against the next."""
    g = ac.wrong_sign_grid()
    n = 0
    for i in range(ac.GRID_FACES):
        name = f"wrong_sign_{i}"
        got = _run(engine, name)
        _assert_equals(got, ac.expected(name))
        n += ac.check_no_wrong_sign_is_decided(got.err, np.flatnonzero(g["owner"] == i))
    assert n == int((g["wrong"] & g["over"]).sum()) >= 1000
    for name in ac.TIE_CASES:
        _assert_equals(_run(engine, name), ac.expected(name))


def test_the_proofs_hold_on_device_output(engine):
    got = _run(engine, "wrong_sign_merged")
    assert ac.check_no_wrong_sign_is_decided(got.err) >= 1000
    for name in ("lattice_box", "lattice_box_inward"):
        r = _as_dict(_run(engine, name))
        assert ac.check_nothing_on_a_face_is_decided(name, r) == 266
        tight = ac.check_err_and_decisions(name, r)
        print(name, "on the device: largest |w - exact| / err", tight)
        assert tight <= 1.0
        m = ac.meta(name)
        assert (r["inside"][~m["on"]] >= 0).all()                     # 175 + 2 934: none hides behind err = inf
    r = _as_dict(_run(engine, "lattice_box_inward"))
    ac.check_err_and_decisions("lattice_box_inward", r, two_sided=True)
    for name in ("ladder_sphere", "ladder_needle"):
        r = _as_dict(_run(engine, name))
        ac.check_nothing_on_a_face_is_decided(name, r)
        assert ac.check_err_and_decisions(name, r) <= 1.0


def test_scale_invariance_on_the_device(engine):
    base = _run(engine, "ladder_sphere")
    for k in ac.SCALES_IDENTICAL:
        got = _run(engine, f"scaled_{k}")
        for key in ARRAYS:
            assert _same_bits(getattr(got, key), getattr(base, key)), (k, key)
    for k in (-180, -200, -299):
        got = _run(engine, f"scaled_{k}")
        fin = np.isfinite(got.err)
        assert _same_bits(got.err[fin], base.err[fin]) and _same_bits(got.inside[fin], base.inside[fin])
        assert np.isinf(got.err[got.rho == 0.0]).all() and (got.inside[got.rho == 0.0] == -1).all()
        assert fin.any() == (k == -180)
    assert (got.rho == 0.0).all() and not got.turns.any() and (got.p[:, 1] == 0.0).all()      # 2^-299: nothing folded


def test_compositions_at_exact_contact(engine):
    q, v, f = ac.get("lattice_box")
    m = ac.meta("lattice_box")
    inside = mm.points_in_mesh(q, (v, f), engine=engine)
    assert m["on"].sum() == 266 and (inside[m["on"]] == -1).all()
    assert (inside[m["exact"] == 1.0] == 1).all() and (inside[m["exact"] == 0.0] == 0).all()
    s = mm.signed_point_mesh_distance(q, (v, f), engine=engine)
    assert ((s.sign == 0) == (s.winding.inside == -1)).all() and _same_bits(s.winding.inside, inside)
    decided = s.sign != 0
    assert _same_bits(np.abs(s.signed_distance[decided]), s.distance[decided]) and np.isnan(s.signed_distance[~decided]).all()
    assert (s.distance[m["on"]] < 1e-9).all() and (s.distance[~m["on"]] >= 0.5).all()    # the grid's step
    assert (s.sign[m["exact"] == 1.0] == -1).all() and (s.sign[m["exact"] == 0.0] == 1).all()
    # the shell between two boxes with integer corners, on the half-integer grid
    lumen, wall = wc.box((-1, -1, -1), (1, 1, 1)), wc.box((-2, -2, -2), (2, 2, 2))
    g = ac.get("lattice_box")[0]
    in_lumen, in_wall = ac.box_side(g, (-1, -1, -1), (1, 1, 1)), ac.box_side(g, (-2, -2, -2), (2, 2, 2))
    r = mm.intramural_points(g, lumen, wall, engine=engine)
    on_either = (in_lumen == -1) | (in_wall == -1)
    assert on_either.sum() > 300 and r.undecided[on_either].all() and not r.mask[on_either].any()
    assert not r.undecided[~on_either].any()
    shell = (in_wall == 1) & (in_lumen == 0)
    assert shell.sum() > 200 and (r.mask == shell).all()
