"""The winding number's promises on worst cases, without a GPU (tests/winding_attack_cases.py): `touch` catches every query
whose face may sit on the wrong side of its jump, `err` bounds the distance from the exact value, no decided query is
wrong, and none of it depends on the scale of the coordinates.  Every family goes through the checker
(tests/mm_checkers/winding_number.py) and through mm.winding.winding_fold_host plus winding_result, the C++ text the
kernel compiles; the two must agree bit for bit, and the proofs are tested on the checker's output.

What a value is compared with: on lattices and covers the exact winding number, known from coordinate comparisons; on the
ladders chk.reference (80-bit), only where it is trusted (winding_attack_cases: every owner face has an exact
|num| / L >= 2^-58, or the query lies exactly in its plane outside the closed triangle).  A query exactly on a closed face
has no value; err = inf is the only acceptable answer there.

Floors on what must be decided are the checker's own counts on the committed families (CPU, f64): they keep a rule that
answers err = inf everywhere from passing.  The printed figures are recorded in DESIGN section 4.29."""
import functools

import numpy as np
import pytest

import multimoda_rs_amd as mm
import winding_attack_cases as ac
from mm_checkers import winding_number as chk

ARRAYS = ("turns", "p", "rho", "touch", "w", "err", "inside")
H0 = ac.ULP_STEPS.index(0)

# finite err among the queries through face interiors / among all queries: the checker's counts on the committed ladders
# (printed by test_floors_on_what_is_decided; CPU).  Every interior query of the translated ladder is finite: one ulp of
# a coordinate of 1e4 is 2^-39 of a face there.
FINITE_INTERIOR = {"ladder_sphere": 3223, "ladder_tube": 3104, "ladder_translated": 4896}
FINITE = {"ladder_sphere": 6220, "ladder_tube": 6096, "ladder_translated": 8220}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _host(name):
    q, v, f = ac.get(name)
    r = mm.winding.winding_fold_host(q, (v, f))
    r["w"], r["err"] = mm.winding.winding_result(r["turns"], r["p"], r["rho"], r["touch"], r["n_staged"])
    r["inside"] = mm.winding.classify(r["w"], r["err"])
    return r


@pytest.mark.parametrize("name", ac.HOST_CASES)
def test_host_hook_equals_checker_bit_for_bit(name):
    want, got = ac.expected(name), _host(name)
    assert got["n_staged"] == want["n_staged"]
    for k in ARRAYS:
        assert _same_bits(got[k], want[k]), k


def test_the_oracle_on_known_positions():
    A, B, C = np.array([0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]), np.array([0.0, 4.0, 0.0])
    assert ac.exact_num((1.0, 1.0, -0.5), A, B, C) == 8 and ac.exact_num((1.0, 1.0, 2.0 ** -1074), A, B, C) < 0
    tiny = ac.exact_num((1.0, 1.0, 2.0 ** -1074), A, B, C)
    assert tiny == -16 * ac.Fraction(2) ** -1074                      # no double holds 1 - 2^-1074; the oracle does
    for p, over in (((1, 1, 5), True), ((2, 2, -1), True), ((0, 0, 3), True), ((4, 0, 0), True), ((2.5, 2, 0), False),
                    ((-2.0 ** -1074, 1, 0), False), ((1, -1, 7), False)):
        assert ac.over_face(np.array(p, dtype=np.float64), A, B, C) is over, p
    q = np.array([[1, 1, 0], [2, 2, 0], [4, 0, 0], [3, 3, 0], [1, 1, 2.0 ** -60], [1, 1, 2.0 ** -50]], dtype=np.float64)
    c = ac.owner_classes(q, np.array([A, B, C]), np.array([[0, 1, 2]]), [[0]] * 6)
    assert c["cls"].tolist() == [ac.ON, ac.ON, ac.ON, ac.PLANE_OUT, ac.OFF, ac.OFF]
    assert c["trusted"].tolist() == [False, False, False, True, False, True] and c["sign"].tolist() == [0, 0, 0, 0, -1, -1]
    for name in ac.LATTICE_CASES:                                     # coordinate comparison and oracle agree on "on a face"
        assert (ac.exact_surface_by_oracle(name) == ac.meta(name)["on"]).all(), name
    assert int(ac.meta("lattice_box")["on"].sum()) == 266


@pytest.mark.parametrize("name", ac.LADDER_CASES + ac.LATTICE_CASES + ("scaled_-150", "scaled_298"))
def test_nothing_on_a_face_is_decided(name):
    n = ac.check_nothing_on_a_face_is_decided(name, ac.expected(name))
    print(name, "queries exactly on a closed face of an owner:", n)


def test_which_ladder_queries_at_offset_zero_are_exactly_on_their_face():
    """The rung 0 of a ladder is the double nearest its face's plane, not a point of the plane: of the queries through
    face interiors the oracle finds 1 of 96 exactly on the face on the sphere, 4 on the tube; the others are a fraction of
    an ulp off, their exact num is not 0, and whether they are decided is the touch bound's business, not exactness."""
    for name, n_on in (("ladder_sphere", 1), ("ladder_tube", 4)):
        m, e = ac.meta(name), ac.expected(name)
        zero = (m["rung"] == H0) & (m["kind"] == 0)
        assert zero.sum() == 96 and int((zero & m["on"]).sum()) == n_on
        assert (m["sign"][zero & ~m["on"]] != 0).all() and (m["log2_ratio"][zero & ~m["on"]] < -47.0).all()
        assert np.isinf(e["err"][zero & m["on"]]).all()


def test_no_wrong_sign_is_decided():
    """Every query of the grid whose f64 num has the wrong sign (or is zero where the exact num is not) and that lies over
    its face: err = inf, against its face alone and in the merged mesh.  The margin: the largest f64 |num| / L among
    them, which a touch constant has to exceed to catch them all."""
    g = ac.wrong_sign_grid()
    n = 0
    for i in range(ac.GRID_FACES):
        sel = np.flatnonzero(g["owner"] == i)
        n += ac.check_no_wrong_sign_is_decided(ac.expected(f"wrong_sign_{i}")["err"], sel)
    assert n == ac.check_no_wrong_sign_is_decided(ac.expected("wrong_sign_merged")["err"]) >= 1000
    attacked = g["wrong"] & g["over"]
    margin = float(np.log2((np.abs(g["num"][attacked]) / g["L"][attacked]).max()))
    print("wrong-sign grid: queries", g["points"].shape[0], "wrong or zero f64 sign of num", int(g["wrong"].sum()),
          "of them f64 zero", int((g["num"][g["wrong"]] == 0.0).sum()), "over their face", n,
          f"largest f64 |num| / L among them 2^{margin:.2f}", f"largest exact 2^{g['log2_ratio'][attacked].max():.2f}")
    assert margin < np.log2(chk.TOUCH)
    # the sign the rule would act on is wrong only where den <= 0, the side of the jump: the attack is on that side
    assert (g["den"][attacked] < 0.0).all()


@pytest.mark.parametrize("name", ac.LADDER_CASES + ac.LATTICE_CASES + ac.COVER_CASES)
def test_err_holds_and_no_decided_query_is_wrong(name):
    e = ac.expected(name)
    tight = ac.check_err_and_decisions(name, e)
    assert tight is not None and tight <= 1.0
    if name == "lattice_box_inward":
        ac.check_err_and_decisions(name, e, two_sided=True)
        assert (chk.classify(e["w"], e["err"], two_sided=True) == ac.expected("lattice_box")["inside"]).all()
        assert not (e["inside"] == 1).any()


def test_floors_on_what_is_decided():
    m, e = ac.meta("lattice_box"), ac.expected("lattice_box")
    assert int(((m["exact"] == 1.0) & (e["inside"] == 1)).sum()) == 175 == int((m["exact"] == 1.0).sum())
    assert int(((m["exact"] == 0.0) & (e["inside"] == 0)).sum()) == 2934 == int((m["exact"] == 0.0).sum())
    m, e = ac.meta("lattice_octahedron"), ac.expected("lattice_octahedron")
    assert (e["inside"][~m["on"]] == m["exact"][~m["on"]]).all() and (~m["on"]).sum() == 4913 - 146
    for name in ac.LADDER_CASES:
        m, e = ac.meta(name), ac.expected(name)
        fin = np.isfinite(e["err"])
        far = np.abs(m["h"]) >= 1e-12 * m["size"]
        print(name, "queries", fin.size, "exactly on a face", int(m["on"].sum()), "finite err", int(fin.sum()), "interiors",
              int((fin & (m["kind"] == 0)).sum()), "of", int((m["kind"] == 0).sum()), "decided", int((e["inside"] >= 0).sum()),
              "1e-12 of the face or more off its plane", int(far.sum()), "finite there", int((far & fin).sum()))
        if name in FINITE:
            assert int((fin & (m["kind"] == 0)).sum()) >= FINITE_INTERIOR[name] and int(fin.sum()) >= FINITE[name]
            assert far.sum() >= 1536 and fin[far].all()
            assert not e["touch"][far].any()
    for name in ac.COVER_CASES:
        assert (ac.expected(name)["inside"] >= 0).all()


@pytest.mark.parametrize("k", ac.SCALES)
def test_scale(k):
    base, e = ac.expected("ladder_sphere"), ac.expected(f"scaled_{k}")
    fin = np.isfinite(e["err"])
    print("scale 2^%d: finite err" % k, int(fin.sum()), "of", fin.size, "unscaled", int(np.isfinite(base["err"]).sum()),
          "queries with a zero face", int((e["rho"] == 0.0).sum()), "unscaled", int((base["rho"] == 0.0).sum()))
    if k in ac.SCALES_IDENTICAL:
        for key in ARRAYS:
            assert _same_bits(e[key], base[key]), key
    else:
        assert _same_bits(e["err"][fin], base["err"][fin]) and _same_bits(e["inside"][fin], base["inside"][fin])
        assert (e["rho"] == 0.0).sum() > (base["rho"] == 0.0).sum()
        assert np.isinf(e["err"][e["rho"] == 0.0]).all() and (e["inside"][e["rho"] == 0.0] == -1).all()
    if k == -180:
        assert _same_bits(e["err"], base["err"]) and fin.any()        # only queries that were undecided anyway cross over
    if k == -299:
        assert (e["rho"] == 0.0).all() and not fin.any() and (e["inside"] == -1).all() and not e["turns"].any()


def test_the_coordinate_limit_is_2_to_the_300():
    q, v, f = ac.get("limit_box")
    e = ac.expected("limit_box")                                      # inside, inside, a corner, on two faces, inside
    assert e["w"][[0, 1, 5]].tolist() == [1.0, 1.0, 1.0] and e["inside"].tolist() == [1, 1, -1, -1, -1, 1]
    assert np.isfinite(e["p"]).all() and e["rho"][2] == 0.0
    over = np.nextafter(2.0 ** 300, np.inf)
    for sign in (1.0, -1.0):
        vv, qq = v.copy(), q.copy()
        vv[3, 1], qq[0, 2] = sign * over, sign * over
        with pytest.raises(ValueError, match="mesh vertices must not exceed 2\\^300 in magnitude"):
            mm.winding.winding_fold_host(q, (vv, f))
        with pytest.raises(ValueError, match="points must not exceed 2\\^300 in magnitude"):
            mm.winding.winding_fold_host(qq, (v, f))
        N = mm._native
        n, p, rho, touch = mm.winding._raw_arrays(q.shape[0])
        staged = np.zeros(1, dtype=np.int64)
        rc = N.lib().mm_winding_fold_host(N._ptr(vv), 8, N._ptr(f), 12, N._ptr(q), q.shape[0], N._ptr(n), N._ptr(p), N._ptr(rho),
                                          N._ptr(touch), N._ptr(staged))
        assert rc == -2 and N.last_error() == "mm_winding_fold_host: vertex coordinate above 2^300"


def test_ties_on_the_boundaries_of_cone_take_the_first_case_that_holds():
    """den and num of each face are the integers listed, exactly on a boundary between two cases of `cone` (rule 3).
    Either neighbouring case would give the same angle -- 135 degrees is one quarter turn plus 45 or two minus 45 -- so no
    proof depends on the choice; the bits do, and the device, the host hook and the checker must make the same one."""
    for i, (tri, num, den, (turns, side)) in enumerate(ac.CONE_TIES):
        q, v, f = ac.get(f"cone_tie_{i}")
        n, d, L = ac.rule_terms(q[:1], v[None, 0], v[None, 1], v[None, 2])
        assert (n[0], d[0]) == (num, den) and ac.exact_num(q[0], *v) == num
        e = ac.expected(f"cone_tie_{i}")
        assert e["turns"][0] == turns and e["p"][0, 1] == side * e["p"][0, 0] and 0.5 <= e["p"][0, 0] < 1.0
        assert abs(e["w"][0] - np.arctan2(num, den) / (2 * np.pi)) <= e["err"][0] < 1e-12
        ref = chk.reference(q, v, f).astype(np.float64)
        assert (np.abs(e["w"] - ref) <= e["err"]).all()
    e, ref = ac.expected("cone_ties"), chk.reference(*ac.get("cone_ties")).astype(np.float64)
    assert np.isfinite(e["err"]).all() and (np.abs(e["w"] - ref) <= e["err"]).all()


def test_covers():
    """|w| > 1, cancellation and nesting.  The whole part of w is carried by `turns` and is exact: 0 or 20 quarter turns
    for five copies of the sphere, 0 for the cancelling pair, 0, 4 or 8 for the nested boxes.  w itself is `turns / 4`
    plus the remainder's rounding residue over 2 pi ("Whole numbers"): within err of the whole number, and
    equal to it only where the residue is absorbed by the addition -- measured on the checker (CPU): 5.0 +- one ulp, 1.0 and
    2.0 up to three ulp off, and outside the residue itself, about 1e-16, not 0.0."""
    m, e = ac.meta("cover_five"), ac.expected("cover_five")
    inner, outer = m["exact"] == 5.0, m["exact"] == 0.0
    assert inner.sum() >= 20 and outer.sum() >= 100
    assert set(e["turns"].tolist()) == {0, 20} and (e["turns"][inner] == 20).all() and (e["turns"][outer] == 0).all()
    assert (np.abs(e["w"] - e["turns"] / 4.0) <= e["err"]).all() and e["err"].max() < 1e-9
    assert (e["inside"] == (e["turns"] == 20)).all()
    e = ac.expected("cover_cancel")
    assert not e["turns"].any() and (np.abs(e["w"]) <= e["err"]).all()
    assert e["err"].max() < 1e-9 and not e["inside"].any()
    m, e = ac.meta("cover_nested"), ac.expected("cover_nested")
    assert set(m["exact"].tolist()) == {0.0, 1.0, 2.0} and (e["turns"] == 4 * m["exact"]).all()
    assert (np.abs(e["w"] - m["exact"]) <= e["err"]).all() and e["err"].max() < 1e-12
    assert (e["inside"] == (m["exact"] >= 1.0)).all()
