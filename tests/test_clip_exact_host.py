"""Mesh clipping against an exact oracle, on the host (no GPU): the host hook mm_mesh_clip_host and the checker
(tests/mm_checkers/mesh_clip.py), equal bit for bit, judged by tests/clip_exact.py (X1-X9: rationals on the f64 inputs and
on the stored coordinates, no clipped mesh of its own) on the cases of tests/clip_exact_cases.py: lattice solids whose
heights are exact, in both orientations, capped and with 1, 2 and 5 extension layers; a plane through rows of vertices;
every case with its complement; K = 2 with one failing cut in either order; ten cuts; a mesh whose every face is cut; cut
faces and kept / dropped vertices on the boundaries of the scans and the waves; heights that round to zero and diagonals
closer than one rounding; and C2's orphan rule, a cut whose kept side another cut drops (KEPT_SIDE_DROPPED).  The oracle
is first tested on itself: hand-made wrong results must fail the matching property.

Figures of these cases (printed by the tests): X7 worst ratio 0.72 of eps max(|p|, ext_length) against
C7 = 4.5; X8 volume worst ratio 0.0025 of the bound (icosahedron), exactly zero where the loop points are exact; 8 exact
ties on the prism, 40 on the torus rows; 32 heights that round to zero, 16 of them negative; 24 near-tied diagonals, 7 of
which a contracted sum decides the other way."""
import types

import numpy as np
import pytest

import clip_cases as CC
import clip_exact as E
import clip_exact_cases as XC
from clip_exact_cases import CASES, judge
from mm_checkers import mesh_clip as Y

import multimoda_rs_amd as mm

HOST = mm.clip.clip_mesh_host


def result(name, impl, flip=False):
    case = CASES[name] if isinstance(name, str) else name
    return XC.run(case, HOST, flip) if impl == "hook" else XC.checked_of(case, flip)


def clone(res):
    return types.SimpleNamespace(vertices=res.vertices.copy(), faces=res.faces.copy(), vertex_origin=res.vertex_origin.copy(),
                                 face_origin=res.face_origin.copy(), face_kind=res.face_kind.copy(), rims=[[r.copy() for r in k] for k in res.rims],
                                 cut_status=res.cut_status.copy(), cut_points=res.cut_points.copy(), cut_loops=res.cut_loops.copy(),
                                 cut_faces=res.cut_faces.copy(), applied=res.applied, report=dict(res.report))


# ---- the oracle on itself ----------------------------------------------------------------------------------------------------

def test_the_oracle_fails_hand_made_wrong_results():
    name = "tie_prism_out_L0"
    case, p = CASES[name], CASES[name].problem()
    good, other = result(name, "hook"), result(name, "hook", flip=True)
    w, w2 = E.View(good), E.View(other)
    cuts = E.cut_sets(w, w2)
    assert not E.x6_caps(p, w, 1)["bad"] and not E.x3_diagonals(p, w, w2, cuts)["bad"] and not E.x1_sides(p, w, cuts)["bad"]
    assert not E.x5_rims(p, w)["bad"] and not E.x4_whole(w)["bad"] and not E.x8_complement(p, w, w2, cuts, closed=True)["bad"]

    # a cap face reversed
    wrong = clone(good)
    at = int(np.nonzero(wrong.face_kind == Y.CAP)[0][0])
    wrong.faces[at] = wrong.faces[at][[1, 0, 2]]
    assert any(b[0] == "the cap does not sum to its polygon" for b in E.x6_caps(p, E.View(wrong), 1)["bad"])
    assert E.x4_whole(E.View(wrong))["bad"]

    # at an exact tie, the quad of one face cut by m_ab - c where C4 says b - m_ca
    quads = other if max(len(x) for x in w2.pieces.values()) == 2 else good
    wrong = clone(quads)
    parent = int(wrong.face_origin[wrong.face_kind == Y.PIECE][0])
    i, j = np.nonzero(wrong.face_origin == parent)[0].tolist()
    (m_ab, b, m_ca), (b2, c, m_ca2) = wrong.faces[i].tolist(), wrong.faces[j].tolist()
    assert b == b2 and m_ca == m_ca2
    wrong.faces[i], wrong.faces[j] = [m_ab, b, c], [m_ab, c, m_ca]
    pair = (E.View(good), E.View(wrong)) if quads is other else (E.View(wrong), E.View(other))
    found = E.x3_diagonals(p, *pair, cuts)
    assert found["n_ties"] == 8 and [b[:2] for b in found["bad"]] == [("the other diagonal", parent)]
    assert not E.x2_pieces(p, *pair, cuts, planar=True)["bad"]             # it still tiles its parent: only X3 knows

    # a dropped vertex resurrected
    wrong = clone(good)
    dead = min(set(range(len(case.v))) - set(good.vertex_origin.tolist()))
    at = int(np.searchsorted(good.vertex_origin[good.vertex_origin >= 0], dead))
    wrong.vertices = np.insert(good.vertices, at, case.v[dead], axis=0)
    wrong.vertex_origin = np.insert(good.vertex_origin, at, dead)
    wrong.faces = good.faces + (good.faces >= at)
    wrong.rims = [[r + (r >= at) for r in k] for k in good.rims]
    assert ("kept though it hangs on a drop side", dead) in E.x1_sides(p, E.View(wrong), cuts)["bad"]
    assert not E.x9_order(p, E.View(wrong))["bad"]                          # in its place, so only X1 (and X4) object

    # a loose cap disc: the pieces of the cut gone, its rim and cap left
    wrong = clone(good)
    keep = wrong.face_kind != Y.PIECE
    wrong.faces, wrong.face_origin, wrong.face_kind = wrong.faces[keep], wrong.face_origin[keep], wrong.face_kind[keep]
    found = E.x5_rims(p, E.View(wrong))
    assert len(found["bad"]) == int(good.cut_points[0]) and all(b[0] == "ring 0 / piece" and b[-1] == 0 for b in found["bad"])

    # the complement of a run is not the run itself
    assert E.x8_complement(p, w, w, cuts)["bad"]


@pytest.mark.parametrize("name", ["torus2_out_L0", "icosa_out_L0", "tie_prism_out_L0", "torus_rows"])
def test_lattice_inputs_have_exact_heights(name):
    """the precondition of X1 and X3, on the inputs alone: rule 1's unfused f64 height is the exact height of every
    (plane, vertex), so the oracle's sides are the rule's; closed and outward"""
    case = CASES[name]
    p = case.problem()
    assert E.heights_are_exact(p)
    assert not E.x4_manifold(p.vF, p.f)["bad"] and E.signed_volume6(p.vF, p.f) > 0


# ---- X1-X9 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", ["hook", "checker"])
@pytest.mark.parametrize("name", XC.PAIRS)
def test_exact_properties_of_a_run_and_its_complement(name, impl):
    case = CASES[name]
    res, other = result(name, impl), result(name, impl, flip=True)
    out = judge(name, res, other)
    judge_flipped = E.x5_rims(case.problem(flip=True), E.View(other))
    assert not judge_flipped["bad"]
    assert set(out) >= {"x2", "x5", "x8", "x9"} and (not case.lattice or {"x1", "x3"} <= set(out))
    if case.ext:
        assert case.ext[1] in (1, 2, 3, 5) and out["x7"]["n_components"] == 3 * case.ext[1] * int(res.cut_points.sum())
    if name.startswith("tie_prism"):
        assert out["x3"]["n_ties"] == 8 and out["x3"]["n_quads"] == 8      # every side face of the prism ties
        if not case.ext:
            assert out["x8"]["asserted_exact"]
    if name == "torus_rows":
        assert out["x3"]["n_ties"] > 0 and out["x8"]["asserted_exact"]
    if name == "tube_capped":
        assert 0.0 <= out["x8"]["volume_ratio"] <= 1.0


def test_a_plane_through_rows_of_vertices_leaves_two_null_pieces_in_one_face():
    case = CASES["torus_rows"]
    res = result("torus_rows", "hook")
    w = E.View(res)
    null = lambda q: len({w.point[n] for n in q}) < 3                      # noqa: E731
    per_face = {parent: sum(null(q) for q in pieces) for parent, pieces in w.pieces.items()}
    assert max(per_face.values()) == 2 and res.report["n_null_pieces"] == sum(per_face.values())
    # an apex on the plane: m_ab = m_ca = a, the apex piece is a point
    p = case.problem()
    on_plane = [parent for parent, pieces in w.pieces.items() if any(len({w.point[n] for n in q}) == 1 for q in pieces)]
    assert on_plane and all(p.h[0][E.apex_frame(p, parent, 0)[0]] == 0 for parent in on_plane)
    print("faces with two null pieces", sum(x == 2 for x in per_face.values()), "apexes on the plane", len(on_plane))


@pytest.mark.parametrize("name, status", [("k2_fail_first", [Y.NOT_SEPARATING, Y.OK]), ("k2_fail_second", [Y.OK, Y.NOT_SEPARATING])])
def test_one_failing_cut_of_two_names_itself_and_nothing_is_cut(name, status):
    case = CASES[name]
    got = result(name, "hook")
    assert got.cut_status.tolist() == status and not got.applied and got.report["n_applied"] == 0
    assert got.vertices.tobytes() == case.v.tobytes() and got.faces.tobytes() == case.f.tobytes() and got.rims == [[], []]


def test_ten_cuts():
    case = CASES["ten_cuts"]
    got = result("ten_cuts", "hook")
    assert got.cut_status.tolist() == [Y.OK] * 10 and got.cut_faces[8:].tolist() == [0, 0] and (got.cut_faces[:8] == 16).all()
    w = E.View(got)                                                       # no status is OVERLAP: no face in two cut sets
    judge("ten_cuts", got)
    pieces = XC.closed_pieces(got)
    assert len(pieces) == 4 and all(not x["bad"] and x["n_faces"] > 0 for x in pieces)
    assert len(w.kept) < len(case.v) - 2 * 20        # both small tubes are gone, and S0, S2, ...
    assert not np.isin(np.arange(len(case.v) - 40, len(case.v)), got.vertex_origin).any()


def test_every_face_cut():
    case = CASES["every_face_cut"]
    got, other = result("every_face_cut", "hook"), result("every_face_cut", "hook", flip=True)
    assert got.cut_faces.tolist() == [len(case.f)] and (got.face_kind != Y.UNTOUCHED).all() and (other.face_kind != Y.UNTOUCHED).all()
    assert got.report["n_pieces"] + other.report["n_pieces"] == 3 * len(case.f)
    judge("every_face_cut", got, other)


# ---- C2's orphan rule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(XC.ORPHAN_STATUS))
def test_a_cut_whose_kept_side_is_dropped(name):
    case = CASES[name]
    for impl in ("hook", "checker"):
        got = result(name, impl)
        assert got.cut_status.tolist() == XC.ORPHAN_STATUS[name] and not got.applied
        assert got.vertices.tobytes() == case.v.tobytes() and got.faces.tobytes() == case.f.tobytes() and got.rims == [[], []]
        assert got.vertex_origin.tolist() == list(range(len(case.v))) and got.face_origin.tolist() == list(range(len(case.f)))
        assert (got.face_kind == Y.UNTOUCHED).all() and got.report["n_applied"] == 0
    err = mm.ClipError(XC.ORPHAN_STATUS[name])
    assert err.statuses == XC.ORPHAN_STATUS[name] and "kept_side_dropped" in str(err)


def test_either_cut_alone_is_applied_and_its_rim_holds():
    """the cuts of the orphan cases one at a time: nothing is wrong with either, and X5 holds"""
    case = CASES["orphan_below_below"]
    for k in range(2):
        one = XC.Case(case.v, case.f, case.o[k:k + 1], case.n[k:k + 1], "below", "loop", True, None, closed=False, outward=1)
        got = XC.run(one, HOST)
        assert got.applied
        judge(one, got, XC.run(one, HOST, flip=True))


STATUS_BEFORE = {"torus_one_cut": [Y.NOT_SEPARATING], "torus_overlap": [Y.OVERLAP, Y.OVERLAP], "torus_miss": [Y.OK, Y.NO_LOOP]}


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_the_earlier_cases_keep_their_statuses_and_have_no_loose_rim(name):
    v, f, o, n, keep, scope, cap, ext = CC.CASES[name]
    got = CC.run(name, HOST)
    assert got.cut_status.tolist() == STATUS_BEFORE.get(name, [Y.OK] * len(o))
    if got.applied:
        case = XC.Case(v, f, o, n, keep, scope, cap, ext)
        found = E.x5_rims(case.problem(), E.View(got))
        assert not found["bad"] and (found["n_edges"] > 0 or got.report["n_closed_loops"] == 0), found["bad"][:3]
        assert not E.x9_order(case.problem(), E.View(got))["bad"]


# ---- the boundaries of the scans and the waves --------------------------------------------------------------------------------

@pytest.mark.parametrize("first_kind", [1, 2])
def test_cut_faces_on_scan_and_wave_boundaries(first_kind):
    base_case, _left = XC.boundary_base()
    case, perm = XC.boundary_faces(first_kind)
    base, got = XC.run(base_case, HOST), XC.run(case, HOST)
    assert got.applied and XC.as_sets(got, face_map=perm) == XC.as_sets(base)
    assert got.vertices.tobytes() == base.vertices.tobytes()


def test_kept_and_dropped_vertices_across_a_scan_boundary():
    base_case, _left = XC.boundary_base()
    case, perm = XC.boundary_vertices()
    base, got = XC.run(base_case, HOST), XC.run(case, HOST)
    assert got.applied and XC.as_sets(got, vertex_map=perm, decimals=9) == XC.as_sets(base, decimals=9)


# ---- rounding worst cases: the hook against the checker, bit for bit -------------------------------------------------------------

def test_heights_that_round_to_zero():
    case, ring = XC.zero_heights()
    zero, neg, pos = XC.zero_height_facts(case, ring)
    print("heights that round to zero", zero, "exact height negative", neg, "positive", pos)
    assert zero == len(ring) == 32 and neg >= 8 and pos >= 8
    got = XC.run(case, HOST)
    # every vertex of the ring is above, so it stays, and no face of the band behind it loses a corner
    assert got.applied and np.isin(ring, got.vertex_origin).all()
    assert (got.face_kind == Y.UNTOUCHED).sum() == 64 and got.report["n_null_pieces"] > 0
    XC.run(case, HOST, flip=True)


def test_near_tied_diagonals():
    case, n_near, n_flip = XC.near_ties()
    print("near-tied diagonals", n_near, "decided the other way by a contracted sum", n_flip)
    assert n_near == 24 and n_flip >= 6
    got = XC.run(case, HOST)
    assert got.applied and got.report["n_pieces"] == 2 * n_near
    # the loop points are the midpoints the search assumed
    new = got.vertices[got.vertex_origin < 0]
    mids = {(0.5 * (case.v[3 * i] + case.v[3 * i + j])).tobytes() for i in range(n_near) for j in (1, 2)}
    assert {x.tobytes() for x in new} == mids
    XC.run(case, HOST, flip=True)
