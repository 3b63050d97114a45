"""Surface distance without a device: the public names and their argument checks; the checker
(tests/mm_checkers/surface_distance.py) against the properties the rule must have -- the seven regions, exact zeros on a
lattice-aligned triangle, never above the nearest corner, invariance under a shuffle of the faces, the ties, the degenerate
faces, the empty mesh -- and against an independent oracle in exact rational arithmetic; the host plan (mm_tri_plan): every
query and face once, every lower bound a true one, and items that pass B must skip on a long tube; the kernels' resources
from the compiler's remarks.

Accuracy of the rule (test_rule_against_the_exact_oracle), measured here on the CPU: the largest
|sqrt(d2) - sqrt(d2_exact)| / D over the octahedron, wound_tube(15, 17) and its jittered copy, with D the bounding-box
diagonal, was 9.61e-17 (the jittered tube; 3.2e-17 on the octahedron, 6.9e-18 on the tube); ACCURACY_TOL is four times
that, rounded up: 3.9e-16.  Sliver triangles are not part of that measurement: tests/test_surface_sliver_host.py holds
theirs (the thin rule, its bounds against the same oracle and its own rounding allowance)."""
import math
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

from mm_checkers import refine_mesh as R
from mm_checkers import surface_distance as S
from test_trim_host import octahedron, capped_tube
from test_refine_host import same_bits, jitter, wound_tube
from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

import multimoda_rs_amd as mm
from multimoda_rs_amd import surface

ACCURACY_TOL = 3.9e-16          # of the bounding-box diagonal; see the module docstring

# one triangle, lattice-aligned, and a query in each region: 0 interior, 1 2 3 corner a b c, 4 5 6 edge ab bc ca
TRIANGLE = (np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]), np.array([[0, 1, 2]]))
REGION_QUERIES = np.array([[1.0, 1.0, 0.5], [-1.0, -1.0, 0.25], [6.0, -1.0, 0.0], [-1.0, 6.0, -0.5], [2.0, -1.0, 1.0],
                           [3.0, 3.0, 0.0], [-2.0, 2.0, 0.0]])
REGIONS = [0, 1, 2, 3, 4, 5, 6]


def two_coplanar():
    """Two triangles of one square; the diagonal (1 - 2) is their shared edge."""
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 2.0, 0.0]])
    return v, np.array([[0, 1, 2], [3, 2, 1]])


def degenerate_faces():
    """(a, a, b), (a, b, a), three collinear corners, three equal corners (by value), one proper face far away."""
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0],
                  [9.0, 9.0, 9.0], [9.0, 8.0, 9.0], [8.0, 9.0, 9.0]])
    f = np.array([[0, 0, 1], [0, 1, 0], [0, 2, 3], [0, 4, 5], [6, 7, 8]])
    q = np.array([[1.0, 1.0, 0.0], [-1.0, 0.5, 0.0], [3.0, 0.0, 2.0], [7.0, 1.0, 1.0], [0.0, 0.0, 0.0], [2.5, -1.0, 0.5]])
    return v, f, q


def long_tube():
    """A capped tube of 41 rings (984 faces: 4 chunks of 256) and the vertices of its jittered, refined copy (at least 2
    query blocks of 512)."""
    v, f = wound_tube(12, 41)
    return v, f, jitter(v, 41)


def far_face_touching_the_first_chunk():
    """513 faces (three chunks): 512 small ones in a row along x, and face 0, a long triangle whose corner sum stages it
    last -- alone in the third chunk -- while its corner (0, 0, 0) is also a corner of the first small face.  The three
    queries are that shared vertex and two more vertices of small faces of the first chunk: every minimum is exactly 0."""
    v = [[0.0, 0.0, 0.0], [2000.0, 1.0, 0.0], [2000.0, -1.0, 0.0]]
    f = [[0, 1, 2]]
    for i in range(512):
        a = 0 if i == 0 else len(v)
        if i:
            v.append([float(i), 0.25, 0.5])
        v += [[i + 0.5, 0.25, 0.5], [float(i), 0.75, 0.5]]
        f.append([a, len(v) - 2, len(v) - 1])
    v, f = np.array(v), np.array(f)
    return v, f, np.array([v[0], v[f[6, 0]], v[f[101, 0]]])


def must_skip(plan, points, v, f):
    """Items of pass B whose lower bound is not below the largest minimum pass A leaves in their block: whatever the
    order in which the device runs pass B, it skips at least these."""
    p = np.asarray(points)[plan["query_perm"]]
    sf = np.asarray(f)[plan["face_order"]]
    top = {}
    for q0, c0 in plan["a"]:
        sq = S.scan(p[q0:q0 + plan["qpb"]], v, sf[c0:c0 + plan["chunk"]])[0]
        top[int(q0)] = sq.max()
    return int(sum(lb2 >= top[int(q0)] for (q0, _), lb2 in zip(plan["b"], plan["b_lb2"])))


# ---- public names ----------------------------------------------------------------------------------------------------

def test_public_names_and_argument_checks():
    for name in ("point_mesh_distance", "sample_mesh_surface", "surface_distance", "PointMeshDistance",
                 "SurfaceDistanceReport", "surface"):
        assert hasattr(mm, name) and name in mm.__all__
    v, f = octahedron()
    with pytest.raises(ValueError, match="out of range"):
        mm.point_mesh_distance(np.zeros((1, 3)), (v, [[0, 1, 6]]))
    with pytest.raises(ValueError, match="finite"):
        mm.point_mesh_distance([[0.0, np.nan, 0.0]], (v, f))
    with pytest.raises(ValueError, match="finite"):
        mm.point_mesh_distance(np.zeros((1, 3)), (np.where(v > 0, np.inf, v), f))
    with pytest.raises(ValueError, match="finite"):
        mm.surface_distance((v, f), (np.where(v > 0, np.inf, v), f))
    with pytest.raises(ValueError, match="at least 1"):
        mm.sample_mesh_surface((v, f), 0)
    with pytest.raises(ValueError, match='"mesh"'):
        mm.sample_mesh_surface({"vertices": v})
    with pytest.raises(ValueError):
        mm.point_mesh_distance(np.zeros((2, 2)), (v, f))


def test_sample_mesh_surface():
    v, f = octahedron()
    p, owner = mm.sample_mesh_surface((v, f))
    assert same_bits(p, v[f[:, ::-1]].reshape(-1, 3) + 0.0) and np.array_equal(owner, np.repeat(np.arange(8), 3))
    p, owner = mm.sample_mesh_surface({"mesh": (v, f)}, 4)
    assert p.shape == (8 * 15, 3) and np.array_equal(owner, np.repeat(np.arange(8), 15))
    a, b, c = v[f[3]]
    k = 0
    for i in range(5):
        for j in range(5 - i):
            assert same_bits(p[3 * 15 + k], ((a * i + b * j) + c * (4 - i - j)) / 4.0)
            k += 1
    assert (np.abs(np.abs(p).sum(axis=1) - 1.0) < 1e-15).all()           # on the octahedron |x| + |y| + |z| = 1


# ---- the checker -----------------------------------------------------------------------------------------------------

def test_the_seven_regions():
    v, f = TRIANGLE
    sq, face, closest, region = S.scan(REGION_QUERIES, v, f)
    assert region.tolist() == REGIONS and (face == 0).all()
    assert closest.tolist() == [[1, 1, 0], [0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]]
    assert sq.tolist() == [0.25, 2.0625, 5.0, 5.25, 2.0, 2.0, 4.0]


def test_points_on_a_lattice_aligned_triangle_are_at_zero():
    v, f = TRIANGLE
    p, _ = mm.sample_mesh_surface((v, f), 8)                             # multiples of 0.5: every operation exact
    sq, face, closest, _ = S.scan(p, v, f)
    assert (sq == 0.0).all() and (face == 0).all() and same_bits(closest, p + 0.0)


def test_never_above_the_nearest_corner():
    rng = np.random.default_rng(5)
    v, f = wound_tube(15, 17)
    v = jitter(v, 17)
    p = rng.uniform(v.min(axis=0) - 1.0, v.max(axis=0) + 1.0, (300, 3))
    sq = S.scan(p, v, f)[0]
    for k in range(len(p)):
        d = p[k] - v[np.unique(f)]
        assert sq[k] <= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min()


def test_shuffled_faces_give_the_same_bits():
    rng = np.random.default_rng(9)
    v, f = wound_tube(15, 17)
    v = jitter(v, 17)
    p = rng.uniform(v.min(axis=0), v.max(axis=0), (200, 3))
    sq, face, closest, region = S.scan(p, v, f)
    perm = rng.permutation(len(f))
    sq2, face2, closest2, _ = S.scan(p, v, f[perm])
    assert same_bits(sq, sq2)
    unique = (S.pair_sq(p, v, f) == sq[None, :]).sum(axis=0) == 1
    assert unique.sum() > 100 and np.array_equal(perm[face2[unique]], face[unique])
    assert same_bits(closest[unique], closest2[unique])


def test_ties_take_the_lower_face():
    v, f = two_coplanar()
    q = np.array([[1.0, 1.0, 3.0], [0.5, 1.5, 1.0], [1.5, 0.5, -2.0]])    # above the shared edge
    sq, face, closest, region = S.scan(q, v, f)
    assert (face == 0).all() and sq.tolist() == [9.0, 1.0, 4.0] and (region == 5).all()
    assert (S.scan(q, v, f[::-1])[1] == 0).all()                          # whichever of the two comes first
    v, f = octahedron()
    twice = np.concatenate([f[[2]], f, f[[2]]])
    q = np.array([[-0.4, -0.3, 0.9]])                                     # nearest to face 2 of the octahedron
    assert S.scan(q, v, f)[1].tolist() == [2] and S.scan(q, v, twice)[1].tolist() == [0]


def test_degenerate_faces_follow_the_segment_rule():
    v, f, q = degenerate_faces()
    assert [S.is_degenerate(v, t) for t in f] == [True, True, True, True, False]
    for k in range(4):
        sq, face, closest, region = S.scan(q, v, f[[k]])
        assert np.isfinite(sq).all() and np.isfinite(closest).all() and set(region.tolist()) <= {4, 5, 6}
        a, b, c = v[f[k]]
        for i, p in enumerate(q):                                         # the nearest of the three segments, sampled
            t = np.linspace(0.0, 1.0, 1001)[:, None]
            pts = np.concatenate([a + (b - a) * t, b + (c - b) * t, c + (a - c) * t])
            assert abs(math.sqrt(sq[i]) - np.sqrt(((pts - p) ** 2).sum(axis=1)).min()) < 1e-3
    sq, face, closest, region = S.scan(q, v, f[[3]])                      # three equal corners: the point itself
    assert (closest == 0.0).all() and (region == 4).all() and same_bits(sq, (q * q).sum(axis=1))
    assert S.scan(q, v, f)[1].tolist() == [0, 0, 2, 2, 0, 2]


def test_an_empty_face_list():
    sq, face, closest, region = S.scan(REGION_QUERIES, TRIANGLE[0], np.zeros((0, 3), dtype=np.int64))
    assert (sq == np.inf).all() and (face == -1).all() and np.isnan(closest).all() and (region == -1).all()


# ---- the exact oracle --------------------------------------------------------------------------------------------------

def _fr(p):
    return tuple(Fraction(float(x)) for x in p)


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def exact_sq(p, a, b, c):
    """The squared distance from p to the triangle in rational arithmetic: the smallest of the plane projection, where
    it falls inside, and the three segments."""
    best = None
    for u, w in ((a, b), (b, c), (c, a)):
        e, pu = _sub(w, u), _sub(p, u)
        l = _dot(e, e)
        t = min(max(_dot(pu, e) / l, 0), 1) if l else 0
        d = _sub(pu, tuple(x * t for x in e))
        d = _dot(d, d)
        best = d if best is None or d < best else best
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    if nn:
        h = _dot(ap, n)
        foot = _sub(ap, tuple(x * h / nn for x in n))                    # the projection, relative to a
        wc, wb = _dot(_cross(ab, foot), n), _dot(_cross(foot, ac), n)
        if wc >= 0 and wb >= 0 and nn - wb - wc >= 0:
            best = min(best, h * h / nn)
    return best


def exact_nearest(p, v, f):
    """(exact squared distance, the faces that reach it) of one point; faces that a bounding sphere rules out (with a
    margin far above rounding) are not evaluated."""
    tri = v[f]
    cen = tri.mean(axis=1)
    rad = np.sqrt(((tri - cen[:, None, :]) ** 2).sum(axis=2)).max(axis=1)
    dc = np.sqrt(((cen - p) ** 2).sum(axis=1))
    corner = np.sqrt(((tri - p) ** 2).sum(axis=2)).min()                 # no face is farther than its nearest corner
    near = np.flatnonzero(dc - rad <= corner * (1.0 + 1e-9) + 1e-9)
    fp = _fr(p)
    d = [exact_sq(fp, _fr(tri[k, 0]), _fr(tri[k, 1]), _fr(tri[k, 2])) for k in near]
    best = min(d)
    return best, [int(near[i]) for i, x in enumerate(d) if x == best]


def accuracy_cases():
    tube = wound_tube(15, 17)
    return {"octahedron": octahedron(), "tube": tube, "jittered_tube": (jitter(tube[0], 17), tube[1])}


def measure_accuracy(v, f, distance, seed=3):
    """The largest |sqrt(d2) - sqrt(d2_exact)| / D of `distance(points) -> (sq, face)` over the samples of two displaced
    copies (by 0.05 and 0.5) and 200 random points of the bounding box; asserts the face where the exact minimum is
    unique."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0), v.max(axis=0)
    D = float(np.sqrt(((hi - lo) ** 2).sum()))
    pts = [rng.uniform(lo, hi, (200, 3))]
    for shift in (np.array([0.03, -0.04, 0.0]), np.array([0.3, 0.0, 0.4])):
        s = mm.sample_mesh_surface((v + shift, f), 2)[0]
        pts.append(s[rng.choice(len(s), min(len(s), 100), replace=False)])
    p = np.concatenate(pts)
    sq, face = distance(p)
    worst, unique = 0.0, 0
    for k in range(len(p)):
        want, faces = exact_nearest(p[k], v, f)
        err = abs(Fraction(math.sqrt(sq[k])) - Fraction(math.sqrt(want))) if want else Fraction(math.sqrt(sq[k]))
        worst = max(worst, float(err) / D)                                # sqrt of the exact value: one more rounding
        if len(faces) == 1:
            unique += 1
            assert face[k] == faces[0], (k, face[k], faces)
    assert unique > len(p) // 2
    return worst


@pytest.mark.parametrize("name", sorted(accuracy_cases()))
def test_rule_against_the_exact_oracle(name):
    v, f = accuracy_cases()[name]
    worst = measure_accuracy(v, f, lambda p: S.scan(p, v, f)[:2])
    print(f"{name}: largest |sqrt(d2) - sqrt(d2_exact)| / D = {worst:.3e}")
    assert worst <= ACCURACY_TOL


# ---- the host plan -----------------------------------------------------------------------------------------------------

def test_plan_holds_every_query_and_face_once_and_true_bounds():
    v, f = wound_tube(15, 17)                                             # 510 faces: 2 chunks
    v = jitter(v, 17)
    p = mm.sample_mesh_surface((v + [0.1, 0.0, 0.2], f))[0]               # 1530 queries: 3 blocks
    plan = surface.tri_plan(p, (v, f))
    qpb, ch = plan["qpb"], plan["chunk"]
    assert qpb == 512 and ch == 256
    assert np.array_equal(np.sort(plan["face_order"]), np.arange(len(f)))
    assert np.array_equal(np.sort(plan["query_perm"]), np.arange(len(p)))
    items = np.concatenate([plan["a"], plan["b"]])
    assert len(plan["a"]) == 3 and len(plan["b"]) == 3
    assert sorted(map(tuple, items.tolist())) == [(q0, c0) for q0 in (0, 512, 1024) for c0 in (0, 256)]
    want = S.predict_report(len(p), len(f), qpb, ch)
    assert want["items_pass_a"] == 3 and want["items_pass_b"] == 3 and want["n_launches"] == 5
    pairs = S.pair_sq(p[plan["query_perm"]], v, f[plan["face_order"]])    # (staged face, staged query)
    for (q0, c0), lb2 in zip(items, np.concatenate([plan["a_lb2"], plan["b_lb2"]])):
        assert lb2 <= pairs[c0:c0 + ch, q0:q0 + qpb].min()
    for (q0, c0), lb2, (_, c1), lb1 in zip(plan["a"], plan["a_lb2"], plan["b"], plan["b_lb2"]):
        assert lb2 <= lb1                                                 # pass A takes the smaller bound
    # slabs: staged faces (by the sum of their corners) and queries ascend along the longest axis (z), up to one cell of
    # the 20-bit quantisation of their range
    for key in (v[f[plan["face_order"]]][:, :, 2].sum(axis=1), p[plan["query_perm"], 2]):
        assert (np.diff(key) >= -(key.max() - key.min()) / 1048575.0 * (1.0 + 1e-9)).all()


def test_plan_of_the_long_tube_has_items_pass_b_must_skip():
    v, f, moved = long_tube()
    fine = R.refine(moved, f, 0.6)[0]
    assert len(f) == 984 and len(fine) > 1024
    plan = surface.tri_plan(fine, (v, f))
    assert len(plan["a"]) == -(-len(fine) // 512) >= 3 and len(plan["b"]) == 3 * len(plan["a"])
    n = must_skip(plan, fine, v, f)
    print(f"long tube: {len(plan['b'])} items in pass B, must_skip = {n}")
    assert n > 0


def test_plan_of_the_far_face_touching_the_first_chunk():
    """The layout tests/test_gpu_surface.py relies on for the who pass's `lb2 > top`: face 0 is staged in another chunk
    than the small face it touches, and the item of its chunk carries the bound 0.0."""
    v, f, q = far_face_touching_the_first_chunk()
    assert len(f) == 513 and f[0, 0] == f[1, 0] and same_bits(q[0], v[f[0, 0]])
    plan = surface.tri_plan(q, (v, f))
    where = np.argsort(plan["face_order"])                                 # face -> staged position
    assert where[0] // plan["chunk"] == 2 and where[1] // plan["chunk"] == 0
    assert (where[[6, 101]] // plan["chunk"] == 0).all()                  # pass A alone brings every minimum to 0
    assert plan["a"].tolist() == [[0, 0]] and sorted(plan["b"][:, 1].tolist()) == [256, 512]
    far = plan["b_lb2"][plan["b"][:, 1] == 512]
    assert len(far) == 1 and same_bits(far, np.array([0.0]))
    assert S.scan(q, v, f)[1].tolist() == [0, 6, 101] and (S.scan(q, v, f)[0] == 0.0).all()


def test_plan_argument_checks():
    v, f = octahedron()
    q = np.zeros((3, 3))
    with pytest.raises(RuntimeError, match="non-finite query"):
        surface.tri_plan(np.full((1, 3), np.nan), (v, f))
    with pytest.raises(RuntimeError, match="non-finite vertex"):
        surface.tri_plan(q, (np.where(v > 0, np.inf, v), f))
    plan = surface.tri_plan(q, (v, np.zeros((0, 3), dtype=np.int64)))
    assert len(plan["a"]) == 0 and len(plan["b"]) == 0 and len(plan["face_order"]) == 0
    plan = surface.tri_plan(np.zeros((0, 3)), (v, f))
    assert len(plan["a"]) == 0 and len(plan["query_perm"]) == 0 and np.array_equal(np.sort(plan["face_order"]), np.arange(8))


# ---- the kernels' resources ----------------------------------------------------------------------------------------------

# name -> (VGPRs, waves per SIMD) as the compiler reports them
RESOURCES = {"k_tri_fill": (8, 8), "k_tri_closest": (72, 7), "k_tri_minILi2ELb0ELb0E": (106, 4),
             "k_tri_minILi2ELb1ELb0E": (108, 4), "k_tri_minILi2ELb0ELb1E": (110, 4)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_tri_kernels_spill_nothing(tmp_path):
    b = _flags()
    assert "mm_tri_kernels.hip" in b.SOURCES and "mm_surface.cpp" in b.SOURCES and "-ffp-contract=off" in b.FLAGS
    remarks, text = _compile(b, os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_tri_kernels.hip"), tmp_path / "k.s")
    seen = {}
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))   # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        key = [k for k in RESOURCES if k in name]
        assert len(key) == 1, name
        seen[key[0]] = (get("VGPRs"), get(r"Occupancy \[waves/SIMD\]"))
        if "k_tri_min" in name:
            assert 24576 <= get(r"LDS Size \[bytes/block\]") <= 24576 + 64, name
    assert seen == RESOURCES
    body = text[text.index("k_tri_minILi2ELb0ELb0E"):]
    assert "v_div_fixup_f64" in body and "v_add_f64" in body and "v_mul_f64" in body
