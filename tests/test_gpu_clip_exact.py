"""Mesh clipping on the device (csrc/mm_clip_kernels.hip, csrc/mm_clip.cpp) against the exact oracle: the case table of
tests/clip_exact_cases.py, each result equal to the checker bit for bit (the report's launches and bytes included) and
then judged by X1-X9 of tests/clip_exact.py, as tests/test_clip_exact_host.py does for the hook.  What only the device
can get wrong is here too: cut faces of either kind at the boundaries of a lane's 16 scan items, of a wave, of a
workgroup, of a scan tile and alone in a tail tile; kept and dropped vertices alternating across a scan tile of the keep
flags; a status word other than the first on a failing call, followed by an applied call on the same engine; heights that
round to zero and diagonals closer than one rounding, where a contracted multiply-add would decide otherwise; and C2's
orphan rule (k_clip_orphan)."""
import numpy as np
import pytest

import clip_cases as CC
import clip_exact as E
import clip_exact_cases as XC
from clip_exact_cases import CASES, judge
from mm_checkers import mesh_clip as Y

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu


def device(case, engine, flip=False):
    """the case on the device with strict off: the checker's arrays and counts, and the predicted report"""
    case = CASES[case] if isinstance(case, str) else case
    got = XC.run(case, mm.clip_mesh, flip, engine=engine, strict=False)
    want = Y.predict_report(len(case.v), len(case.f), len(case.o), XC.checked_dict(case, flip), got.report["jump_rounds"])
    for k, x in want.items():
        assert got.report[k] == x, (k, got.report[k], x)
    return got


@pytest.mark.parametrize("name", XC.PAIRS)
def test_exact_properties_of_a_run_and_its_complement(engine, name):
    case = CASES[name]
    res, other = device(name, engine), device(name, engine, flip=True)
    out = judge(name, res, other)
    assert not E.x5_rims(case.problem(flip=True), E.View(other))["bad"]
    if name.startswith("tie_prism"):
        assert out["x3"]["n_ties"] == 8
    if name == "torus_rows":
        w = E.View(res)
        assert out["x3"]["n_ties"] > 0 and max(sum(len({w.point[n] for n in q}) < 3 for q in ps) for ps in w.pieces.values()) == 2


@pytest.mark.parametrize("name, status", [("k2_fail_first", [Y.NOT_SEPARATING, Y.OK]), ("k2_fail_second", [Y.OK, Y.NOT_SEPARATING])])
def test_one_failing_cut_of_two_then_an_applied_call(engine, name, status):
    case = CASES[name]
    got = device(name, engine)
    assert got.cut_status.tolist() == status and not got.applied
    assert got.vertices.tobytes() == case.v.tobytes() and got.faces.tobytes() == case.f.tobytes()
    assert got.report["n_launches"] == 5 + got.report["jump_rounds"]       # the verdict said no: the orphan check is not run
    small = device("tie_prism_out_L0", engine)
    assert small.applied and small.report["n_launches"] == 5 + small.report["jump_rounds"] + 1 + 11


def test_ten_cuts_and_every_face_cut(engine):
    got = device("ten_cuts", engine)
    assert got.cut_status.tolist() == [Y.OK] * 10
    judge("ten_cuts", got)
    pieces = XC.closed_pieces(got)
    assert len(pieces) == 4 and all(not x["bad"] for x in pieces)
    every, other = device("every_face_cut", engine), device("every_face_cut", engine, flip=True)
    assert (every.face_kind != Y.UNTOUCHED).all() and every.cut_faces.tolist() == [len(CASES["every_face_cut"].f)]
    judge("every_face_cut", every, other)


@pytest.mark.parametrize("name", sorted(XC.ORPHAN_STATUS))
def test_a_cut_whose_kept_side_is_dropped(engine, name):
    case = CASES[name]
    got = device(name, engine)
    assert got.cut_status.tolist() == XC.ORPHAN_STATUS[name] and not got.applied
    assert got.vertices.tobytes() == case.v.tobytes() and got.faces.tobytes() == case.f.tobytes() and got.rims == [[], []]
    assert got.report["n_launches"] == 5 + got.report["jump_rounds"] + 1
    with pytest.raises(mm.ClipError) as err:
        v, f, o, n, keep, scope, cap, ext = case.args()
        mm.clip_mesh((v, f), o, n, keep=keep, scope=scope, cap=cap, extension=ext, engine=engine)
    assert err.value.statuses == XC.ORPHAN_STATUS[name] and "kept_side_dropped" in str(err.value)


@pytest.mark.parametrize("name", [n for n in sorted(CC.CASES) if n not in ("scan_tiles", "long_thin")])
def test_the_earlier_cases_have_no_loose_rim(engine, name):
    v, f, o, n, keep, scope, cap, ext = CC.CASES[name]
    got = CC.run(name, mm.clip_mesh, engine=engine, strict=False)
    if got.applied:
        case = XC.Case(v, f, o, n, keep, scope, cap, ext)
        assert not E.x5_rims(case.problem(), E.View(got))["bad"] and not E.x9_order(case.problem(), E.View(got))["bad"]


@pytest.mark.parametrize("first_kind", [1, 2])
def test_cut_faces_on_scan_and_wave_boundaries(engine, first_kind):
    base_case, _left = XC.boundary_base()
    case, perm = XC.boundary_faces(first_kind)
    base, got = device(base_case, engine), device(case, engine)
    assert got.applied and XC.as_sets(got, face_map=perm) == XC.as_sets(base)
    assert got.vertices.tobytes() == base.vertices.tobytes()
    assert not E.x5_rims(case.problem(), E.View(got))["bad"]


def test_kept_and_dropped_vertices_across_a_scan_boundary(engine):
    base_case, _left = XC.boundary_base()
    case, perm = XC.boundary_vertices()
    base, got = device(base_case, engine), device(case, engine)
    assert got.applied and XC.as_sets(got, vertex_map=perm, decimals=9) == XC.as_sets(base, decimals=9)


def test_heights_that_round_to_zero(engine):
    case, ring = XC.zero_heights()
    zero, neg, pos = XC.zero_height_facts(case, ring)
    assert zero == len(ring) and neg >= 8
    got = device(case, engine)                                             # sides, cut set, pieces and counts: the checker's
    assert got.applied and np.isin(ring, got.vertex_origin).all() and (got.face_kind == Y.UNTOUCHED).sum() == 64
    device(case, engine, flip=True)


def test_near_tied_diagonals(engine):
    case, n_near, n_flip = XC.near_ties()
    assert n_near == 24 and n_flip >= 6
    got = device(case, engine)
    assert got.applied and got.report["n_pieces"] == 2 * n_near
    device(case, engine, flip=True)
