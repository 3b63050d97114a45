"""An exact oracle for mesh cross-sections: `fractions.Fraction` on the f64 inputs, nothing rounded but the final division
by |n|.  It shares no code with the checker (tests/mm_checkers/mesh_sections.py) and restates none of its sums: heights
and sides by rule 1's convention, crossing points, distances to a mesh edge, and the area and area centroid of a listed
polygon about its own first point (translation-free), an even-odd point-in-polygon test that knows its boundary, and the
convex hull of coplanar points."""
import math
from fractions import Fraction as F

INSIDE, OUTSIDE, BOUNDARY = 1, 0, -1


def fr(p):
    """a point or vector of floats as exact rationals"""
    return tuple(F(float(x)) for x in p)


def fr_rows(a):
    return [fr(r) for r in a]


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def height(o, n, x):
    """the exact height of x over the plane (o, n), not divided by |n|"""
    return dot(n, sub(x, o))


def side(h):
    """rule 1: h < 0 is below (0), everything else above (1)"""
    return 0 if h < 0 else 1


def crossing(a, b, ha, hb):
    """the exact point of the edge a-b on the plane; the heights have different sides, so ha != hb"""
    t = ha / (ha - hb)
    return tuple(a[k] + t * (b[k] - a[k]) for k in range(3))


def dist2_to_segment(p, a, b):
    """the exact squared distance from p to the closed segment a-b"""
    ab, ap = sub(b, a), sub(p, a)
    den = dot(ab, ab)
    t = F(0) if den == 0 else min(F(1), max(F(0), dot(ap, ab) / den))
    q = sub(ap, tuple(t * x for x in ab))
    return dot(q, q)


def fan_terms(pts):
    """d_i x d_(i+1) about the first point, for i = 0 .. m - 1 (the first and the last are zero)"""
    m = len(pts)
    d = [sub(p, pts[0]) for p in pts]
    return [cross(d[i], d[(i + 1) % m]) for i in range(m)], d


def vector_area(pts):
    c, _d = fan_terms(pts)
    return tuple(sum(x[k] for x in c) / 2 for k in range(3))


def signed_area_times_norm(pts, n):
    """vector area . n: the signed area about n times |n|, exact"""
    return dot(vector_area(pts), n)


def norm64(n):
    """|n| as the f64 the rule divides by"""
    x, y, z = (float(v) for v in n)
    return math.sqrt((x * x + y * y) + z * z)


def signed_area(pts, n):
    """the signed area about n as an exact rational over the f64 |n|"""
    return signed_area_times_norm(pts, n) / F(norm64(n))


def fan_weights(pts, n):
    """w_i = (d_i x d_(i+1)) . n, exact"""
    c, _d = fan_terms(pts)
    return [dot(x, n) for x in c]


def fan_magnitude(pts, n):
    """sum over the fan of |n_k| (|d_a e_b| + |d_b e_a|): every product that enters W, taken positive -- the scale of
    the rounding error of any f64 evaluation of W about the first point"""
    m = len(pts)
    d = [sub(p, pts[0]) for p in pts]
    total = F(0)
    for i in range(m):
        a, b = d[i], d[(i + 1) % m]
        q = (abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]), abs(a[0] * b[1]) + abs(a[1] * b[0]))
        total += sum(abs(n[k]) * q[k] for k in range(3))
    return total


def centroid(pts, n):
    """the exact area centroid of the polygon (None where its signed area is 0)"""
    c, d = fan_terms(pts)
    m = len(pts)
    w = [dot(x, n) for x in c]
    W = sum(w)
    if W == 0:
        return None
    return tuple(pts[0][k] + sum(w[i] * (d[i][k] + d[(i + 1) % m][k]) for i in range(m)) / (3 * W) for k in range(3))


def drop_axes(n):
    """(u, v): the two axes kept by the projection that drops the largest |n| component, the first among equals"""
    an = [abs(x) for x in n]
    drop = 0
    for a in (1, 2):
        if an[a] > an[drop]:
            drop = a
    return (1 if drop == 0 else 0), (1 if drop == 2 else 2)


def point_in_polygon(q, pts, n):
    """INSIDE, OUTSIDE or BOUNDARY, even-odd, in the dominant projection of n"""
    iu, iv = drop_axes(n)
    inside = False
    m = len(pts)
    for i in range(m):
        a, b = pts[i], pts[(i + 1) % m]
        au, av, bu, bv = a[iu] - q[iu], a[iv] - q[iv], b[iu] - q[iu], b[iv] - q[iv]
        if au * bv - av * bu == 0 and min(au, bu) <= 0 <= max(au, bu) and min(av, bv) <= 0 <= max(av, bv):
            return BOUNDARY
        if (av > 0) != (bv > 0) and 0 < au + (-av) * (bu - au) / (bv - av):
            inside = not inside
    return INSIDE if inside else OUTSIDE


def convex_hull(points, n):
    """the hull polygon of coplanar points (Andrew's monotone chain in the dominant projection), as 3-D points"""
    iu, iv = drop_axes(n)
    uniq = sorted({(p[iu], p[iv]): p for p in points}.items())
    if len(uniq) < 3:
        return [p for _k, p in uniq]
    turn = lambda o, a, b: (a[0][0] - o[0][0]) * (b[0][1] - o[0][1]) - (a[0][1] - o[0][1]) * (b[0][0] - o[0][0])   # noqa: E731
    lower, upper = [], []
    for seq, out in ((uniq, lower), (uniq[::-1], upper)):
        for x in seq:
            while len(out) >= 2 and turn(out[-2], out[-1], x) <= 0:
                out.pop()
            out.append(x)
    return [p for _k, p in lower[:-1] + upper[:-1]]


def polygon_length(pts):
    """the perimeter in f64 from exact squared lengths"""
    m = len(pts)
    return sum(math.sqrt(float(dot(sub(pts[(i + 1) % m], pts[i]), sub(pts[(i + 1) % m], pts[i])))) for i in range(m))


def exact_cut(vF, faces, o, n):
    """From exact sides: {face: ((key, point), (key, point))} of the crossed faces of one plane, each segment directed
    so that the inside of an outward-oriented mesh is on its left about n; and the sides of the vertices."""
    h = [height(o, n, x) for x in vF]
    s = [side(x) for x in h]
    cut, point = {}, {}
    for i, t in enumerate(faces):
        if len(set(t)) < 3 or s[t[0]] == s[t[1]] == s[t[2]]:
            continue
        ends = []
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if s[a] != s[b]:
                key = (min(a, b), max(a, b))
                if key not in point:
                    point[key] = crossing(vF[key[0]], vF[key[1]], h[key[0]], h[key[1]])
                ends.append((key, point[key]))
        along = cross(n, cross(sub(vF[t[1]], vF[t[0]]), sub(vF[t[2]], vF[t[0]])))
        if dot(sub(ends[1][1], ends[0][1]), along) < 0:
            ends.reverse()
        cut[i] = tuple(ends)
    return cut, s


def section_area_times_norm(cut, n):
    """the exact signed area (times |n|) the directed segments enclose: the section of the solid, with no chaining"""
    if not cut:
        return F(0)
    ref = next(iter(cut.values()))[0][1]
    return sum(dot(cross(sub(a, ref), sub(b, ref)), n) for (_ka, a), (_kb, b) in cut.values()) / 2
