"""The closest point of a triangle on sliver faces, without a device: the checker (tests/mm_checkers/surface_distance.py,
the line-for-line twin of csrc/mm_tri_device.h) against exact rational arithmetic on the faces of
tests/tri_sliver_cases.py, the host plan's bounds on meshes that hold slivers, and the fold over such meshes.

What is asserted for every (query, face) pair of the per-face families, with d = sqrt(d2) of the checker, d_exact the
exact distance, alt the face's exact smallest altitude (2 area / longest edge) rounded up, and R = R_TOL * max(D, M) -- D
the diagonal of the box of the face and its queries, M their largest |coordinate|:

* d >= d_exact - R: the computed point is a point of the closed triangle up to rounding, so the distance is never too
  small and a lower bound of the exact distance is one of the computed distance (the pruning proof).
* d <= d_exact + alt + R.  Derived, not measured: every point of a triangle lies within its inradius (<= alt / 2) of an
  edge, so a rule that returns the nearest of candidates that include the three segments overshoots by no more.
* the closest point lies in the face's box widened by the plan's slack (tri_slack: 64 ulp of the largest coordinate);
* it agrees with the region: a corner's bits for 1, 2, 3; within R of the edge's line for 4, 5, 6.

R_TOL.  Measured here on the CPU over all the families (test_rule_on_slivers prints the figure of each): the largest
shortfall (d_exact - d) / max(D, M) was R_MEASURED (below); R_TOL is four times that, rounded up.
ACCURACY_TOL of tests/test_surface_host.py (3.9e-16 of D, well-shaped faces) stays what it was.

The rule before the thin branch (every non-degenerate face through Ericson's tests) misses the upper bound from the ratio
2^-20 on; DESIGN 4.19 has the table of both."""
import math
from fractions import Fraction

import numpy as np
import pytest

from mm_checkers import surface_distance as S
from test_refine_host import same_bits
from test_surface_host import _cross, _dot, _fr, _sub, exact_sq, must_skip
import tri_sliver_cases as C

import multimoda_rs_amd as mm
from multimoda_rs_amd import surface

R_MEASURED = 1.52e-16           # the largest shortfall (needle_random, 2^-24); see the module docstring
R_TOL = 6.1e-16                 # of max(D, largest |coordinate|)
EPS = 2.0 ** -52


def up(x):
    return math.nextafter(x * (1.0 + 4.0 * EPS), math.inf)


def exact_altitude(a, b, c):
    """The smallest altitude of the face, 2 area / longest edge, from exact rationals, rounded up."""
    fa, fb, fc = _fr(a), _fr(b), _fr(c)
    n = _cross(_sub(fb, fa), _sub(fc, fa))
    longest = max(_dot(e, e) for e in (_sub(fb, fa), _sub(fc, fb), _sub(fa, fc)))
    return up(math.sqrt(_dot(n, n) / longest)) if longest else 0.0


def line_distance(q, u, w):
    """The distance of q from the line through u and w (from u where they coincide), exact up to the last root."""
    fq, fu, fw = _fr(q), _fr(u), _fr(w)
    e, d = _sub(fw, fu), _sub(fq, fu)
    x = _cross(d, e)
    return math.sqrt(_dot(x, x) / _dot(e, e)) if _dot(e, e) else math.sqrt(_dot(d, d))


def check_face(tri, queries, kind, r_tol=R_TOL):
    """Asserts the four properties for one face against its queries; returns the largest shortfall and the largest
    overshoot in units of max(D, M), and the largest overshoot in altitudes."""
    a, b, c = tri
    both = np.concatenate([tri, queries])
    scale = max(float(np.linalg.norm(both.max(axis=0) - both.min(axis=0))), float(np.abs(both).max()))
    alt = exact_altitude(a, b, c)
    q, region = S.closest_on_face(queries, a, b, c, kind)
    d = np.sqrt(S.dist_sq(queries, q))
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    fa, fb, fc = _fr(a), _fr(b), _fr(c)
    short = over = over_alt = 0.0
    for k, p in enumerate(queries):
        want = math.sqrt(exact_sq(_fr(p), fa, fb, fc))
        err = float(Fraction(float(d[k])) - Fraction(want))
        short, over = max(short, -err / scale), max(over, err / scale)
        over_alt = max(over_alt, err / alt) if alt else over_alt
        assert d[k] >= want - r_tol * scale, ("too small", k, d[k], want, scale)
        assert d[k] <= want + alt + r_tol * scale, ("too large", k, d[k], want, alt, scale)
        slack = 64.0 * EPS * max(float(np.abs(tri).max()), float(np.abs(p).max()))
        assert (q[k] >= lo - slack).all() and (q[k] <= hi + slack).all(), ("outside the box", k, q[k], lo, hi)
        r = int(region[k])
        if r in (1, 2, 3):
            assert same_bits(q[k], tri[r - 1] + 0.0), ("corner", k, r)
        elif r in (4, 5, 6):
            u, w = ((a, b), (b, c), (c, a))[r - 4]
            assert line_distance(q[k], u, w) <= r_tol * scale, ("off the edge", k, r)
        else:
            assert r == 0 and kind != S.DEGENERATE
    return short, over, over_alt


@pytest.fixture(scope="module")
def families():
    return C.families()


def test_the_case_module_holds_what_it_says(families):
    assert sorted(families) == ["cap_axis", "cap_random", "collinear", "needle_axis", "needle_random"]
    kinds = {}
    for name, (v, f, q) in families.items():
        assert len(f) <= 48 and q.shape == (len(f), 48, 3) and np.isfinite(v).all() and np.isfinite(q).all()
        kinds[name] = [S.face_kind(v, t) for t in f]
    # the collinear faces are thin, not degenerate, but for the one lattice face between its two neighbours of one ulp
    assert kinds["collinear"] == [S.THIN] * 18 + [S.THIN, S.DEGENERATE, S.THIN]
    for name in ("needle_random", "needle_axis", "cap_random", "cap_axis"):
        v, f, _ = families[name]
        for k, t in enumerate(f):
            ratio = exact_altitude(*v[t]) / max(np.linalg.norm(v[t[i]] - v[t[i - 1]]) for i in range(3))
            nominal = C.nominal_ratio(name, k)
            if nominal <= 30:                                             # below, the rounding of the corners shows
                assert abs(math.log2(ratio) + nominal) < 0.01, (name, k, ratio)
            # a factor sqrt(2) either side of the threshold, and everything else, falls on its side of it
            want = (S.THIN if nominal > S.THIN_K else S.PROPER,) + ((S.DEGENERATE,) if nominal == 50 else ())
            assert kinds[name][k] in want, (name, k, nominal)             # at 2^-50 rounding may leave no face at all


@pytest.mark.parametrize("name", ["cap_axis", "cap_random", "collinear", "needle_axis", "needle_random"])
def test_rule_on_slivers(families, name):
    v, f, q = families[name]
    short = over = 0.0
    for k, t in enumerate(f):
        s, o, _ = check_face(v[t], q[k], S.face_kind(v, t))
        short, over = max(short, s), max(over, o)
    print(f"{name}: largest shortfall {short:.3e}, largest overshoot {over:.3e} of max(D, M)")


def test_a_query_on_a_cap_is_not_reported_above_it(families):
    """The case that started this: a query on a cap of height 2^-20 came out tens of heights away."""
    v, f, q = families["cap_random"]
    k = [i for i in range(len(f)) if C.nominal_ratio("cap_random", i) == 20][0]          # the one at the origin
    tri, alt = v[f[k]], exact_altitude(*v[f[k]])
    on = q[k][:7]                                                         # the lattice at height 0
    proper = np.sqrt(S.dist_sq(on, S.closest_on_face(on, *tri, S.PROPER)[0]))
    thin = np.sqrt(S.dist_sq(on, S.closest_on_face(on, *tri, S.face_kind(v, f[k]))[0]))
    print(f"cap 2^-20, alt {alt:.3e}: Ericson's tests give up to {proper.max():.3e}, the thin rule {thin.max():.3e}")
    assert thin.max() <= alt + R_TOL * 4.0                                # the face and these queries lie within 4


# ---- the plan's bounds and the fold over meshes that hold slivers ---------------------------------------------------------

def sliver_meshes():
    """name -> (vertices, faces, queries): the strip with its own queries; the squeezed tube with lattice samples of
    itself, the same displaced, and points of its box."""
    v, f, q = C.sliver_strip()
    tv, tf = C.squeezed_tube()
    rng = np.random.default_rng(21)
    s = mm.sample_mesh_surface((tv, tf), 2)[0][::8]                       # 738 of them: with the rest, 4 blocks of 512
    tq = np.concatenate([s, s + 0.01 * rng.standard_normal(s.shape), rng.uniform(tv.min(axis=0), tv.max(axis=0), (120, 3))])
    return {"strip": (v, f, q), "tube": (tv, tf, tq)}


@pytest.fixture(scope="module")
def meshes():
    return sliver_meshes()


def scale_of(*arrays):
    """max(D, M) of the points: the diagonal of their box and their largest |coordinate|."""
    pts = np.concatenate([np.reshape(a, (-1, 3)) for a in arrays])
    return max(float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0))), float(np.abs(pts).max()))


def thin_altitude(v, f):
    """(number of thin faces, the largest exact altitude among them)."""
    alts = [exact_altitude(*v[t]) for t in f if S.face_kind(v, t) == S.THIN]
    return len(alts), max(alts)


def test_the_meshes_hold_what_they_say(meshes):
    v, f, q = meshes["strip"]
    assert len(f) >= 513 and len(q) >= 1025 and thin_altitude(v, f)[0] == len(f) // 4
    assert abs(math.log2(thin_altitude(v, f)[1] / 0.5) + 20) < 0.01
    tv, tf, tq = meshes["tube"]
    n, alt = thin_altitude(tv, tf)
    assert len(tf) == 984 and n >= 24 + 6 and alt <= 2.0 ** -20 * 1.01     # the band of 24 needles and the 6 caps


@pytest.mark.parametrize("name", ["strip", "tube"])
def test_plan_bounds_hold_for_the_computed_distances(meshes, name):
    v, f, q = meshes[name]
    plan = surface.tri_plan(q, (v, f))
    qpb, ch = plan["qpb"], plan["chunk"]
    assert len(plan["a"]) >= 3 and len(plan["b"]) >= 2 * len(plan["a"])
    pairs = S.pair_sq(q[plan["query_perm"]], v, f[plan["face_order"]])
    items = np.concatenate([plan["a"], plan["b"]])
    for (q0, c0), lb2 in zip(items, np.concatenate([plan["a_lb2"], plan["b_lb2"]])):
        assert lb2 <= pairs[c0:c0 + ch, q0:q0 + qpb].min(), (q0, c0)
    n = must_skip(plan, q, v, f)
    print(f"{name}: {len(plan['b'])} items in pass B, must_skip = {n}")
    if name == "strip":
        assert n > 0


def exact_distances(p, v, f, margin):
    """(exact squared distance, face) ascending, of the faces a bounding sphere does not rule out by more than
    `margin` beyond the nearest corner."""
    tri = v[f]
    cen = tri.mean(axis=1)
    rad = np.sqrt(((tri - cen[:, None, :]) ** 2).sum(axis=2)).max(axis=1)
    dc = np.sqrt(((cen - p) ** 2).sum(axis=1))
    corner = np.sqrt(((tri - p) ** 2).sum(axis=2)).min()
    near = np.flatnonzero(dc - rad <= corner * (1.0 + 1e-9) + 1e-9 + margin)
    fp = _fr(p)
    return sorted((exact_sq(fp, _fr(tri[k, 0]), _fr(tri[k, 1]), _fr(tri[k, 2])), int(k)) for k in near)


@pytest.mark.parametrize("name", ["strip", "tube"])
def test_fold_against_the_exact_nearest(meshes, name):
    v, f, q = meshes[name]
    rng = np.random.default_rng(4)
    p = q[rng.choice(len(q), 300, replace=False)]
    both = np.concatenate([v, p])
    scale = max(float(np.linalg.norm(both.max(axis=0) - both.min(axis=0))), float(np.abs(both).max()))
    allow = thin_altitude(v, f)[1] + R_TOL * scale
    sq, face = S.scan(p, v, f)[:2]
    worst, decided = 0.0, 0
    for k in range(len(p)):
        exact = exact_distances(p[k], v, f, 2.0 * allow)
        want = math.sqrt(exact[0][0])
        worst = max(worst, abs(math.sqrt(sq[k]) - want))
        assert want - R_TOL * scale <= math.sqrt(sq[k]) <= want + allow, (k, sq[k], want)
        if len(exact) == 1 or math.sqrt(exact[1][0]) > want + allow:     # near-ties on slivers are legitimate
            decided += 1
            assert face[k] == exact[0][1], (k, face[k], exact[:2])
    print(f"{name}: largest |d - d_exact| = {worst:.3e}, allowance {allow:.3e}, face decided for {decided} of {len(p)}")
    assert decided > len(p) // 4


@pytest.mark.parametrize("name", ["strip", "tube"])
def test_shuffled_faces_give_the_same_bits(meshes, name):
    v, f, q = meshes[name]
    perm = np.random.default_rng(13).permutation(len(f))
    assert same_bits(S.scan(q, v, f)[0], S.scan(q, v, f[perm])[0])
