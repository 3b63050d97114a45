"""The winding number without a GPU: the checker (tests/mm_checkers/winding_number.py) against an independent long-double
reference, the host hooks mm_winding_plan and mm_winding_fold_host (the arithmetic the kernels run) against the checker bit
for bit, the claims about touch, err and the classification on adversarial queries, and the Python argument checks."""
import os

import numpy as np
import pytest

import multimoda_rs_amd as mm
import winding_attack_cases as ac
import winding_cases as wc
from mm_checkers import winding_number as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nf,chunks_per_group,groups", [(0, 0, 0), (1, 1, 1), (256, 1, 1), (257, 1, 2), (16 * 256, 1, 16),
                                                        (16 * 256 + 1, 2, 9), (8192, 2, 16), (511, 1, 2), (513, 1, 3)])
def test_plan_is_the_rules_grouping(nf, chunks_per_group, groups):
    pl = mm.winding.winding_plan(nf)
    chunks = -(-nf // 256)
    assert pl == {"chunk": 256, "chunks_per_group": chunks_per_group, "groups": groups, "n_staged": nf}
    assert pl["chunks_per_group"] == -(-chunks // 16) and pl["groups"] <= 16
    if nf:
        assert (pl["groups"] - 1) * pl["chunks_per_group"] < chunks <= pl["groups"] * pl["chunks_per_group"]   # no empty group


@pytest.mark.parametrize("name", wc.BIT_CASES)
def test_fold_host_equals_checker_bit_for_bit(name):
    q, v, f = wc.get(name)
    want = wc.expected(name)
    got = mm.winding.winding_fold_host(q, (v, f))
    assert got["n_staged"] == want["n_staged"]
    for k in ("turns", "p", "rho", "touch"):
        assert _same_bits(got[k], want[k]), k
    w, err = mm.winding.winding_result(got["turns"], got["p"], got["rho"], got["touch"], got["n_staged"])
    assert _same_bits(w, want["w"]) and _same_bits(err, want["err"])
    assert _same_bits(mm.winding.classify(w, err), want["inside"])


@pytest.mark.parametrize("name", wc.BIT_CASES)
def test_checker_agrees_with_long_double_reference_within_err(name):
    want, ref = wc.expected(name), wc.expected_reference(name)
    fin = np.isfinite(want["err"])
    gap = np.abs(want["w"] - ref).astype(np.float64)
    print(name, "finite", int(fin.sum()), "of", fin.size, "largest |w - ref|", gap[fin].max() if fin.any() else None)
    assert (gap[fin] <= want["err"][fin]).all()
    decided_in, decided_out = want["inside"] == 1, want["inside"] == 0
    assert (ref[decided_in] > 0.5).all() and (ref[decided_out] < 0.5).all()


def test_closed_solids_give_whole_numbers():
    """Inside is exactly 1, an inward-oriented solid gives exactly -1: the remainder's angle is below half an ulp of
    2 pi and is absorbed.  Outside is exactly 0 where the arithmetic is exact -- the queries at integer distances from
    every corner (winding_cases.octahedron, tetrahedron) -- and within err of 0 elsewhere: the remainder's imaginary part
    is then a rounding residue of order 1e-17, and w is that over 2 pi, not 0."""
    e = wc.expected("octahedron")                       # (0,0,0) (4,0,0) (1,.5,.25) (5,5,5) (-4,0,0) (1,1,1) on a face
    assert e["w"][[0, 2]].tolist() == [1.0, 1.0] and e["w"][[1, 4]].tolist() == [0.0, 0.0]
    assert (e["turns"][:5] % 4 == 0).all() and e["turns"][[0, 2]].tolist() == [4, 4]
    assert abs(e["w"][3]) <= e["err"][3] < 1e-13
    assert e["inside"][:5].tolist() == [1, 0, 1, 0, 0]
    assert e["touch"].tolist() == [False] * 5 + [True] and e["err"][5] == np.inf and e["inside"][5] == -1
    e = wc.expected("octahedron_inward")
    assert e["w"].tolist() == [-1.0, 0.0, -1.0] and e["turns"].tolist() == [-4, 0, -4]
    assert e["inside"].tolist() == [0, 0, 0]
    assert chk.classify(e["w"], e["err"], two_sided=True).tolist() == [1, 0, 1]
    e = wc.expected("tetrahedron")                      # the origin (outside), the centroid, (10, 10, 10)
    assert e["w"].tolist() == [0.0, 1.0, 0.0] and (e["turns"] % 4 == 0).all()
    e = wc.expected("tetrahedron_about_origin")         # the origin (inside), (2, 2, 2), (.1, .1, .1)
    assert e["w"].tolist() == [1.0, 0.0, 1.0] and e["turns"].tolist() == [4, 0, 4]


def test_open_tube_gives_fractions():
    e = wc.expected("tube")
    inner = e["w"][-5:]                                 # on the axis: middle, near the end, in the opening, beyond, the other end
    assert 0.5 < inner[1] < inner[0] < 1.0 and 0.0 < inner[3] < inner[2] < 0.5 + 1e-12
    assert (e["turns"] % 4 != 0).any()
    assert np.isfinite(e["err"]).all()


@pytest.mark.parametrize("name,mesh,stride", [("adversarial_sphere", "sphere512", 16), ("adversarial_tube", "tube", 18)])
def test_adversarial_queries(name, mesh, stride):
    v, f = getattr(wc, mesh)()
    pts, kind, h = wc.adversarial(v, f, stride)
    e, ref = wc.expected(name), wc.expected_reference(name)
    # touch: every query placed on a face's interior, none that is 1e-12 or more off its face; a query placed on an edge
    # or a vertex is caught by touch or by rho, whichever way its own rounding moved it.  Where the rounding of an h = 0
    # query left it, by the exact oracle of tests/winding_attack_cases.py: of the 32 placed on a face's interior 1 is
    # exactly on its face on the sphere and none on the tube, the others are off the plane by less than an ulp of a
    # coordinate; of the 96 on edge midpoints 15 and 39 are exactly on the edge; all 96 on corners are the corner; and of
    # the 32 placed in the plane outside the triangle 1 (sphere) and 0 (tube) are exactly in the plane.
    zero = np.flatnonzero(h == 0.0)
    owner = (zero // (pts.shape[0] // len(range(0, f.shape[0], stride)))) * stride
    cls = ac.owner_classes(pts[zero], v, f, [[int(o)] for o in owner])["cls"]
    on = [int(((cls == ac.ON) & (kind[zero] == k)).sum()) for k in range(4)]
    assert on == {"sphere512": [1, 15, 96, 0], "tube": [0, 39, 96, 0]}[mesh]
    assert int(((cls == ac.PLANE_OUT) & (kind[zero] == 3)).sum()) == {"sphere512": 1, "tube": 0}[mesh]
    assert np.isinf(e["err"][zero][cls == ac.ON]).all() and (e["inside"][zero][cls == ac.ON] == -1).all()
    assert e["touch"][(kind == 0) & (h == 0.0)].all()
    assert not e["touch"][np.abs(h) >= 1e-12].any()
    assert (e["rho"][(kind == 2) & (h == 0.0)] == 0.0).all()          # a query on a vertex
    assert not e["touch"][kind == 3].any()                            # in the plane, outside the triangle
    fin = np.isfinite(e["err"])
    assert fin[np.abs(h) >= 1e-12].all() and not fin[(kind <= 2) & (h == 0.0)].any()
    gap = np.abs(e["w"] - ref).astype(np.float64)
    print(name, "largest |w - ref| where err is finite", gap[fin].max(), "largest finite err", e["err"][fin].max())
    assert (gap[fin] <= e["err"][fin]).all()
    assert (ref[e["inside"] == 1] > 0.5).all() and (ref[e["inside"] == 0] < 0.5).all()
    far = wc.point_triangle_distance(pts, v, f) >= 1e-3
    assert far.sum() >= 100
    print(name, "queries 1e-3 or more from every face", int(far.sum()), "largest err", e["err"][far].max())
    assert (e["err"][far] <= 1e-6).all()


def test_degenerate_faces_do_not_change_a_bit():
    q, v2, f2 = wc.get("degenerate")
    v, f = wc.sphere512()
    plain = chk.winding(q, v, f, wc.plan)
    assert wc.expected("degenerate")["n_staged"] == f.shape[0] < f2.shape[0]
    for k in ("turns", "p", "rho", "touch", "w", "err", "inside"):
        assert _same_bits(wc.expected("degenerate")[k], plain[k]), k
    e = wc.expected("degenerate_only")
    assert e["n_staged"] == 0 and not e["w"].any() and not e["err"].any() and not e["inside"].any()


def test_face_order_moves_w_within_err():
    q, v, f = wc.get("degenerate")[0], *wc.sphere512()
    a = chk.winding(q, v, f, wc.plan)
    b = chk.winding(q, v, f[np.random.default_rng(3).permutation(f.shape[0])], wc.plan)
    assert (np.abs(a["w"] - b["w"]) <= a["err"] + b["err"]).all()
    both = (a["inside"] >= 0) & (b["inside"] >= 0)
    assert both.all() and (a["inside"] == b["inside"]).all()


def test_exports_and_argument_checks_need_no_engine():
    header = open(os.path.join(ROOT, "include", "mm_ccta.h")).read()
    for sym in ("mm_mesh_winding", "mm_winding_result", "mm_winding_plan", "mm_winding_fold_host"):
        assert f"int     {sym}(" in header and sym in mm._native.EXPORTS_CCTA and hasattr(mm._native.lib(), sym)
    for name in ("mesh_winding_number", "points_in_mesh", "signed_point_mesh_distance", "mesh_containment", "intramural_points",
                 "intramural_course", "WindingNumber", "ContainmentReport"):
        assert hasattr(mm, name) and name in mm.__all__
    assert "winding number" in header
    v, f = wc.box((0, 0, 0), (1, 1, 1))
    ok = np.zeros((2, 3))
    bad_f = f.copy()
    bad_f[3, 1] = 8
    for bad_v in (np.nan, np.inf, 2.0 ** 301, -2.0 ** 301):
        w = v.copy()
        w[2, 1] = bad_v
        p = ok.copy()
        p[1, 2] = bad_v
        for call in (lambda: mm.mesh_winding_number(ok, (w, f)), lambda: mm.mesh_winding_number(p, (v, f)),
                     lambda: mm.points_in_mesh(p, (v, f)), lambda: mm.signed_point_mesh_distance(ok, (w, f)),
                     lambda: mm.mesh_containment((w, f), (v, f)), lambda: mm.mesh_containment((v, f), (w, f)),
                     lambda: mm.intramural_points(p, (v, f), (v, f)), lambda: mm.intramural_course(ok, (v, f), (w, f)),
                     lambda: mm.winding.winding_fold_host(p, (v, f))):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: mm.mesh_winding_number(ok, (v, bad_f)), lambda: mm.intramural_points(ok, (v, f), (v, bad_f)),
                 lambda: mm.mesh_winding_number(ok, (v, f), threshold=np.nan)):
        with pytest.raises(ValueError):
            call()
    # the C entry points say the same
    n, p, rho, touch = mm.winding._raw_arrays(2)
    staged = np.zeros(1, dtype=np.int64)
    N = mm._native
    big = v.copy()
    big[0, 0] = 2.0 ** 301
    for vv, ff, msg in ((big, f, "vertex coordinate above 2^300"), (v, bad_f, "face index out of range")):
        rc = N.lib().mm_winding_fold_host(N._ptr(vv), 8, N._ptr(ff), 12, N._ptr(ok), 2, N._ptr(n), N._ptr(p), N._ptr(rho),
                                          N._ptr(touch), N._ptr(staged))
        assert rc == -2 and N.last_error() == "mm_winding_fold_host: " + msg
    assert mm.winding.first_run(np.array([False, True, True, False, True]), np.arange(15.0).reshape(5, 3))[:2] == (1, 2)
    assert mm.winding.first_run(np.zeros(4, dtype=bool), np.zeros((4, 3))) == (-1, -1, 0.0)
