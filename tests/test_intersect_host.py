"""Mesh intersections without a device: the public names; the checker (tests/mm_checkers/mesh_intersections.py) against
an oracle in exact rational arithmetic -- known answers on single pairs, soundness of every proved state on pairs pushed
off a plane or an edge line by a few ulp, nothing undecided on the general-position fixtures; the host plan
(mm_isect_plan): the items are the chunk pairs with overlapping boxes, and every pair the unculled scan does not call
disjoint lies inside one; the kernels' resources from the compiler's remarks."""
import functools
import math
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

from mm_checkers import mesh_intersections as X
from test_trim_host import octahedron
from test_refine_host import jitter, wound_tube
from test_surface_host import long_tube
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm
from multimoda_rs_amd import intersect

D, I, U = X.DISJOINT, X.INTERSECTING, X.UNDECIDED


# ---- the exact oracle --------------------------------------------------------------------------------------------------

def _fr(p):
    return tuple(Fraction(float(x)) for x in p)


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _at(p, q, t):
    return tuple(p[k] + (q[k] - p[k]) * t for k in range(3))


def segment_in_triangle(p, q, tri):
    """The parameters [t0, t1] of the part of the segment p q inside the closed triangle, or None; exact."""
    a, b, c = tri
    n = _cross(_sub(b, a), _sub(c, a))
    dp, dq = _dot(n, _sub(p, a)), _dot(n, _sub(q, a))
    if dp == 0 and dq == 0:                                               # coplanar: clip against the three edges
        t0, t1 = Fraction(0), Fraction(1)
        for u, w in ((a, b), (b, c), (c, a)):
            side = lambda x: _dot(_cross(_sub(w, u), _sub(x, u)), n)      # noqa: E731  >= 0 inside
            f0, f1 = side(p), side(q)
            if f0 < 0 and f1 < 0:
                return None
            if f0 < 0:
                t0 = max(t0, f0 / (f0 - f1))
            elif f1 < 0:
                t1 = min(t1, f0 / (f0 - f1))
        return (t0, t1) if t0 <= t1 else None
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return None
    t = dp / (dp - dq)
    x = _at(p, q, t)
    for u, w in ((a, b), (b, c), (c, a)):
        if _dot(_cross(_sub(w, u), _sub(x, u)), n) < 0:
            return None
    return (t, t)


def _in_hull(x, shared):
    if len(shared) == 1:
        return x == shared[0]
    a, b = shared
    e, d = _sub(b, a), _sub(x, a)
    return _cross(e, d) == (0, 0, 0) and 0 <= _dot(e, d) <= _dot(e, e)


def oracle(t1, t2, id1=(0, 1, 2), id2=(3, 4, 5)):
    """True iff the closed triangles meet in a point outside the hull of their shared vertices; three shared: True."""
    a, b = tuple(_fr(p) for p in t1), tuple(_fr(p) for p in t2)
    shared = [a[k] for k in range(3) if id1[k] in id2]
    if len(shared) == 3:
        return True
    for s, t in ((a, b), (b, a)):
        for k in range(3):
            p, q = s[k], s[(k + 1) % 3]
            hit = segment_in_triangle(p, q, t)
            if hit is None:
                continue
            if not shared or not (_in_hull(_at(p, q, hit[0]), shared) and _in_hull(_at(p, q, hit[1]), shared)):
                return True
    return False


def sound(t1, t2, id1=(0, 1, 2), id2=(3, 4, 5)):
    """The checker's state, asserted against the oracle where it is a proof."""
    state, _ = X.pair_state(t1, t2, id1, id2)
    if state != U:
        assert (state == I) == oracle(t1, t2, id1, id2), (t1, t2, id1, id2, state)
    return state


def T(*rows):
    return tuple(tuple(float(x) for x in r) for r in rows)


# ---- known answers -----------------------------------------------------------------------------------------------------

BASE = T((0, 0, 0), (4, 0, 0), (0, 4, 0))
KNOWN = {
    "crossing": (BASE, T((1, 1, -1), (1, 1, 1), (2, 1.5, 1)), None, I),
    "apart_by_plane": (BASE, T((1, 1, 1), (2, 1, 2), (1, 2, 3)), None, D),
    "apart_along_the_line": (BASE, T((5, 5, -1), (5, 5, 1), (7, 6, 1)), None, D),
    "coplanar_apart": (BASE, T((5, 5, 0), (7, 5, 0), (5, 7, 0)), None, D),
    "coplanar_overlapping": (BASE, T((1, 1, 0), (7, 1, 0), (1, 7, 0)), None, U),
    "one_shared_no_crossing": (BASE, T((0, 0, 0), (-1, -2, 3), (-2, -1, -3)), ((0, 1, 2), (0, 3, 4)), D),
    "one_shared_crossing": (BASE, T((0, 0, 0), (3, 3, 2), (3, 3, -2)), ((0, 1, 2), (0, 3, 4)), I),
    "one_shared_flat": (BASE, T((0, 0, 0), (-1, -3, 0), (-3, -1, 0)), ((0, 1, 2), (0, 3, 4)), D),
    "one_shared_flat_collinear_edges": (BASE, T((0, 0, 0), (-2, 0, 0), (-1, -3, 0)), ((0, 1, 2), (0, 3, 4)), D),
    "one_shared_flat_overlapping": (BASE, T((0, 0, 0), (3, 1, 0), (1, 3, 0)), ((0, 1, 2), (0, 3, 4)), U),
    "edge_flat": (BASE, T((4, 0, 0), (0, 0, 0), (1, -3, 0)), ((0, 1, 2), (1, 0, 3)), D),
    "edge_dihedral": (BASE, T((4, 0, 0), (0, 0, 0), (1, 1, 3)), ((0, 1, 2), (1, 0, 3)), D),
    "edge_folded": (BASE, T((4, 0, 0), (0, 0, 0), (1, 2, 0)), ((0, 1, 2), (1, 0, 3)), U),
    "coincident": (BASE, T((4, 0, 0), (0, 4, 0), (0, 0, 0)), ((0, 1, 2), (1, 2, 0)), I),
}
ORACLE = {"crossing": True, "apart_by_plane": False, "apart_along_the_line": False, "coplanar_apart": False,
          "coplanar_overlapping": True, "one_shared_no_crossing": False, "one_shared_crossing": True, "one_shared_flat": False,
          "one_shared_flat_collinear_edges": False, "one_shared_flat_overlapping": True, "edge_flat": False,
          "edge_dihedral": False, "edge_folded": True, "coincident": True}


def known_mesh(name):
    """The pair as a mesh of two faces: (vertices, faces); shared ids become shared indices."""
    t1, t2, ids, _ = KNOWN[name]
    id1, id2 = ids or ((0, 1, 2), (3, 4, 5))
    n = max(id1 + id2) + 1
    v = np.zeros((n, 3))
    for t, i in ((t1, id1), (t2, id2)):
        for p, k in zip(t, i):
            v[k] = p
    return v, np.array([id1, id2])


def test_public_names():
    for name in ("mesh_self_intersections", "mesh_intersections", "MeshIntersections", "intersect"):
        assert hasattr(mm, name) and name in mm.__all__
    assert "mm_mesh_intersections" in mm._native.EXPORTS_CCTA and "mm_isect_plan" in mm._native.EXPORTS_CCTA
    with pytest.raises(ValueError, match="max_pairs"):
        mm.mesh_self_intersections(octahedron(), max_pairs=-1)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    t1, t2, ids, want = KNOWN[name]
    ids = ids or ((0, 1, 2), (3, 4, 5))
    assert oracle(t1, t2, *ids) == ORACLE[name]
    state, coincident = X.pair_state(t1, t2, *ids)
    assert state == want and coincident == (name == "coincident")
    assert sound(t2, t1, ids[1], ids[0]) == want                          # the other order proves no less here
    got = X.scan(*known_mesh(name))
    assert got["pairs"].tolist() == ([] if want == D else [[0, 1]]) and got["pair_state"].tolist() == ([] if want == D else [want])
    assert got["face_state"].tolist() == [want, want]


def test_equal_coordinates_under_other_indices_read_as_adjacent():
    t1, t2, ids, _ = KNOWN["edge_dihedral"]
    v = np.array(t1 + t2)                                                 # six vertices, two pairs of them equal
    v[3, 1] = -0.0                                                        # (4, -0, 0) equals (4, 0, 0)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    assert X.canonical_ids(v).tolist() == [0, 1, 2, 1, 0, 5]
    got = X.scan(v, f)
    assert got["pairs"].shape == (0, 2) and got["narrow_tests"] == 1
    two = X.scan_two(v, f[:1], v, f[1:])                                  # without identities the faces touch
    assert two["pair_state"].tolist() == [U]


def test_a_degenerate_face_is_counted_and_tested_against_nothing():
    v, f = known_mesh("crossing")
    v = np.concatenate([v, [[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]]])
    f = np.concatenate([f, [[6, 7, 8], [0, 1, 1]]])
    got = X.scan(v, f)
    assert got["n_degenerate_faces"] == 2 and got["pairs"].tolist() == [[0, 1]] and got["face_state"].tolist() == [1, 1, 0, 0]
    assert got["narrow_tests"] == 1


# ---- soundness under attack ----------------------------------------------------------------------------------------------

def _steps(x, size):
    """x moved by 0, +-1, +-2, ... ulp and by +- size * 2^-k, k = 30 .. 52."""
    out = [x]
    up = down = x
    for _ in range(6):
        up, down = math.nextafter(up, math.inf), math.nextafter(down, -math.inf)
        out += [up, down]
    for k in range(30, 53):
        out += [x + size * 2.0 ** -k, x - size * 2.0 ** -k]
    return out


def test_every_proved_state_is_true_near_a_plane_and_near_an_edge_line():
    rng = np.random.default_rng(23)
    seen = {D: 0, I: 0, U: 0}
    for trial in range(4):
        a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
        wa, wb = rng.uniform(0.1, 0.45, 2)
        on_plane = a + wa * (b - a) + wb * (c - a)                        # inside the face, up to rounding
        on_edge = a + wa * (b - a)                                        # on the line of edge ab
        t1 = T(a, b, c)
        far1, far2 = on_plane + rng.uniform(-1.0, 1.0, 3), on_plane + rng.uniform(-1.0, 1.0, 3)
        n = np.cross(b - a, c - a)
        ax = int(np.argmax(np.abs(n)))
        for base in (on_plane, on_edge):
            for x in _steps(float(base[ax]), 4.0):
                p = base.copy()
                p[ax] = x
                # no shared vertex; one shared vertex (a); the shared edge a b with the moved corner opposite
                seen[sound(t1, T(p, far1, far2))] += 1
                seen[sound(T(p, far1, far2), t1)] += 1
                seen[sound(t1, T(a, p, far1), (0, 1, 2), (0, 3, 4))] += 1
                seen[sound(t1, T(a, far1, p), (0, 1, 2), (0, 3, 4))] += 1
                seen[sound(t1, T(b, a, p), (0, 1, 2), (1, 0, 3))] += 1
                # a coplanar partner: all three corners in the plane up to rounding
                q1 = a + 0.3 * (b - a) + 1.5 * (c - a)
                q2 = a + 1.5 * (b - a) + 1.6 * (c - a)
                seen[sound(t1, T(p, q1, q2))] += 1
                # coplanar partners that share the corner a: one in the opposite wedge, one beside the edge a b
                w1, w2 = a - 0.7 * (b - a) - 0.2 * (c - a), a - 0.1 * (b - a) - 0.9 * (c - a)
                for other in (T(a, w1, w2), T(a, p, w2), T(a, w1, p)):
                    seen[sound(t1, other, (0, 1, 2), (0, 3, 4))] += 1
    print("soundness: states seen", seen)
    assert min(seen.values()) > 50                                        # the attack reaches all three states


def test_lattice_pairs_with_exact_contact_are_never_proved_wrong():
    rng = np.random.default_rng(31)
    seen = {D: 0, I: 0, U: 0}
    for _ in range(1500):
        v = rng.integers(-2, 3, (6, 3)).astype(np.float64)
        if X.is_degenerate(v[:3], (0, 1, 2)) or X.is_degenerate(v[3:], (3, 4, 5)):
            continue
        ids = X.canonical_ids(v)
        seen[sound(T(*v[:3]), T(*v[3:]), tuple(ids[:3]), tuple(ids[3:]))] += 1
    print("lattice: states seen", seen)
    assert min(seen.values()) > 20


# ---- condition -------------------------------------------------------------------------------------------------------------

def general_octahedra():
    v, f = octahedron()
    v = jitter(v, 1)
    return v, f, v + [0.3, 0.2, 0.1], f


def general_tube():
    v, f = wound_tube(15, 17)
    return jitter(v, 17), f


def pushed_tube():
    """general_tube with one ring pushed through the opposite wall."""
    v, f = general_tube()
    v = v.copy()
    ring = np.arange(15 * 8, 15 * 9)
    far = ring[v[ring, 0] < -0.5]                                         # the side of the ring opposite the wall x = 1
    v[far, 0] += 2.6
    return v, f


def random_faces(nf):
    """nf random faces over 90 vertices: most boxes overlap, many faces share a vertex or an edge."""
    rng = np.random.default_rng(257)
    v = rng.uniform(-3.0, 3.0, (90, 3))
    return v, rng.integers(0, 90, (X.CHUNK + 1, 3))[:nf]


def shifted_long_tubes():
    v, f, _ = long_tube()
    return v, f, v + [0.5, 0.0, 0.0], f


def both_long_tubes():
    va, fa, vb, fb = shifted_long_tubes()
    return np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])


SELF_CASES = {"general_tube": general_tube, "pushed_tube": pushed_tube, "both_long_tubes": both_long_tubes,
              "random_257": lambda: random_faces(X.CHUNK + 1), "random_256": lambda: random_faces(X.CHUNK),
              "random_1": lambda: random_faces(1)}
TWO_CASES = {"general_octahedra": general_octahedra, "shifted_long_tubes": shifted_long_tubes}


@functools.lru_cache(maxsize=None)
def checked(name):
    """(mesh arrays, the checker's unculled scan) of a named case, computed once a process."""
    if name in SELF_CASES:
        mesh = SELF_CASES[name]()
        return mesh, X.scan(*mesh)
    mesh = TWO_CASES[name]()
    return mesh, X.scan_two(*mesh)


def test_general_position_leaves_nothing_undecided():
    va, fa, vb, fb = general_octahedra()
    two = checked("general_octahedra")[1]
    assert two["n_undecided_pairs"] == 0 and two["n_intersecting_pairs"] > 0
    want = sorted((i, j) for i in range(8) for j in range(8) if oracle(T(*va[fa[i]]), T(*vb[fb[j]])))
    assert two["pairs"].tolist() == [list(p) for p in want]
    tube = checked("general_tube")[1]
    assert tube["n_undecided_pairs"] == 0 and tube["n_intersecting_pairs"] == 0 and tube["narrow_tests"] > 510
    pushed = checked("pushed_tube")[1]
    assert pushed["n_undecided_pairs"] == 0 and pushed["n_intersecting_pairs"] > 0


# ---- the host plan ---------------------------------------------------------------------------------------------------------

def boxes_overlap(a, b):
    return bool((a[:3] <= b[3:]).all() and (b[:3] <= a[3:]).all())


def check_plan(plan, va, fa, vb, fb, found):
    ch = plan["chunk"]
    assert ch == X.CHUNK
    self_form = vb is None
    oa = plan["order_a"]
    ob = oa if self_form else plan["order_b"]
    vb, fb = (va, fa) if self_form else (vb, fb)
    assert np.array_equal(np.sort(oa), np.arange(len(fa))) and np.array_equal(np.sort(ob), np.arange(len(fb)))
    ba, bb = plan["boxes_a"], plan["boxes_a"] if self_form else plan["boxes_b"]
    for boxes, v, f, order in ((ba, va, fa, oa), (bb, vb, fb, ob)):
        assert len(boxes) == -(-len(f) // ch)
        for c in range(len(boxes)):
            pts = v[f[order[c * ch:(c + 1) * ch]]].reshape(-1, 3)
            assert np.array_equal(boxes[c], np.concatenate([pts.min(axis=0), pts.max(axis=0)]))
    want = [(i, j) for i in range(len(ba)) for j in range(i if self_form else 0, len(bb)) if boxes_overlap(ba[i], bb[j])]
    assert sorted(map(tuple, plan["items"].tolist())) == want
    assert plan["items_total"] == (len(ba) * (len(ba) + 1) // 2 if self_form else len(ba) * len(bb))
    items = set(want)
    wa, wb = np.argsort(oa), np.argsort(ob)                               # face -> staged position
    for i, j in found:
        ci, cj = int(wa[i]) // ch, int(wb[j]) // ch
        assert ((min(ci, cj), max(ci, cj)) if self_form else (ci, cj)) in items


def test_plan_items_are_the_overlapping_chunk_pairs_and_hold_every_pair_found():
    (v, f, moved, _), two = checked("shifted_long_tubes")
    plan = intersect.isect_plan((v, f), (moved, f))
    check_plan(plan, v, f, moved, f, two["pairs"])
    assert len(two["pairs"]) > 0 and len(plan["items"]) < plan["items_total"] == 16
    both, one = checked("both_long_tubes")
    plan = intersect.isect_plan(both)
    check_plan(plan, both[0], both[1], None, None, one["pairs"])
    assert len(plan["items"]) < plan["items_total"] == 36
    # the crossings between the two tubes are the same in both forms (a flat cap's own fan is undecided by rule 6)
    crossing = lambda r: r["pairs"][r["pair_state"] == I]                 # noqa: E731
    between = crossing(one)[(crossing(one)[:, 0] < len(f)) & (crossing(one)[:, 1] >= len(f))]
    assert np.array_equal(between - [0, len(f)], crossing(two)) and len(between) > 0
    (v, f), pushed = checked("pushed_tube")
    check_plan(intersect.isect_plan((v, f)), v, f, None, None, pushed["pairs"])


def test_plan_argument_checks_and_empty_meshes():
    v, f = octahedron()
    with pytest.raises(RuntimeError, match="mm_isect_plan: non-finite vertex"):
        intersect.isect_plan((np.where(v > 0, np.inf, v), f))
    with pytest.raises(RuntimeError, match="mm_isect_plan: non-finite vertex"):
        intersect.isect_plan((v, f), (np.where(v > 0, np.nan, v), f))
    none = np.zeros((0, 3), dtype=np.int64)
    plan = intersect.isect_plan((v, none))
    assert len(plan["items"]) == 0 and plan["items_total"] == 0 and len(plan["order_a"]) == 0
    plan = intersect.isect_plan((v, f), (v, none))
    assert len(plan["items"]) == 0 and len(plan["order_b"]) == 0 and len(plan["order_a"]) == 8
    plan = intersect.isect_plan((v, f))
    assert plan["items"].tolist() == [[0, 0]] and plan["items_total"] == 1


# ---- the kernels' resources ----------------------------------------------------------------------------------------------

# name -> (VGPRs, waves per SIMD) as the compiler reports them
RESOURCES = {"k_isect_clear": (5, 8), "k_isect_pairsILb1E": (172, 2), "k_isect_pairsILb0E": (126, 4)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_intersect_kernels_spill_nothing(tmp_path):
    b = _flags()
    assert "mm_intersect_kernels.hip" in b.SOURCES and "mm_intersect.cpp" in b.SOURCES and "mm_isect_device.h" in b.HEADERS
    assert "-ffp-contract=off" in b.FLAGS
    remarks, text = _compile(b, os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_intersect_kernels.hip"), tmp_path / "k.s")
    seen = {}
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))   # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        key = [k for k in RESOURCES if k in name]
        assert len(key) == 1, name
        seen[key[0]] = (get("VGPRs"), get(r"Occupancy \[waves/SIMD\]"))
        if "k_isect_pairs" in name:
            assert 24576 <= get(r"LDS Size \[bytes/block\]") <= 24576 + 64, name
    print("intersect kernels:", seen)
    assert seen == RESOURCES
    body = text[text.index("k_isect_pairsILb1E"):]
    assert "v_add_f64" in body and "v_mul_f64" in body and not re.search(r"\bv_fmac?_f64\b", body)
