"""Mesh cross-sections against exact cuts, on the host (no GPU): the checker's ``scan`` and the product's host hooks
(``section_cut_host`` then ``section_chain``, equal to the checker bit for bit) on worst-case inputs, every point and
measure compared with tests/section_exact.py (rationals on the f64 inputs).

E1 points on their mesh edge, E2 points on the plane, E3 topology of closed manifold input, E4 direction, E5 area,
E6 centroid, E7 selection, E8 invariance under a move of the origin inside its plane.  The constants: DESIGN 4.28.
C1 and C2 are derived; C3 and C4 are declared measured there (eight times the worst ratio of these very cases, the
printed "worst" figures: E5 0.064, E6 0.035).  E6 adds to the issue's bound eps * max|coordinate| of the loop: the centroid
is stored at the magnitude of its absolute coordinates, as the points of E2 are, and no f64 result can do better.
Which branch of E6 a loop has to meet -- the box of a flat loop or the centroid bound -- is the oracle's say
(``flatness``), never the rule's; two families of hand-made loops given to the chain as segments (exactly collinear
loops whose W is rounding noise, thin triangles) hold the flat condition from both sides."""
import functools
import hashlib
import math

import numpy as np
import pytest

import section_exact as Q
from mm_checkers import mesh_sections as X
from test_section_host import cube, join, same_arrays, tube
from test_trim_host import octahedron

import multimoda_rs_amd as mm

S = mm.section
EPS = 2.0 ** -52
C1, C2 = 4.5, 4.5                     # derived: 2.5 sqrt(3) and 4, with room for the second-order terms
C3, C4 = 0.52, 0.28                   # measured on these cases: 8 x 0.064 and 8 x 0.035
F = Q.F

DELTAS, OFFS = (1e-3, 1e-6, 1e-9, 1e-12), (0.0, 1.0, 100.0, 1e4)
FAR = (1e3, -1e3, 1e3)


class Case:
    def __init__(self, v, f, o, n, closed=True, lattice=False, select=False, kind=None, ulp_planes=()):
        self.v, self.f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
        self.o, self.n = np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(n, dtype=np.float64).reshape(-1, 3)
        self.closed, self.lattice, self.select, self.kind, self.ulp_planes = closed, lattice, select, kind, set(ulp_planes)
        assert len(self.f) < 1000 and len(self.o) <= 100 and len(self.o) == len(self.n)

    def args(self):
        return self.v, self.f, self.o, self.n


# ---- the cases ------------------------------------------------------------------------------------------------------

def corner_origin(delta, off, shift):
    b = 1.0 - delta
    return [shift[0] + (b + off), shift[1] + (b - off), shift[2] + b]


def corner_loops(shift):
    """the unit cube under planes with n = (1, 1, 1) just below the corner (1, 1, 1): hexagons of size delta, the origin
    moved by off * (1, -1, 0)"""
    v, f = cube()
    o = [corner_origin(d, off, shift) for d in DELTAS for off in OFFS]
    return Case(v + np.array(shift), f, o, [[1.0, 1.0, 1.0]] * len(o))


def lattice_torus():
    """16 x 20 quads on a 1/64 grid, outward; z depends on the row alone, so z planes go through whole rows"""
    R, r, na, nb = 2.0, 0.75, 20, 16
    th, ph = 2.0 * np.pi * np.arange(na) / na, 2.0 * np.pi * np.arange(nb) / nb
    v = np.array([[(R + r * math.cos(p)) * math.cos(t), (R + r * math.cos(p)) * math.sin(t), r * math.sin(p)] for t in th for p in ph])
    v = np.round(v * 64.0) / 64.0
    f = []
    for i in range(na):
        for j in range(nb):
            a, b, c, d = i * nb + j, ((i + 1) % na) * nb + j, ((i + 1) % na) * nb + (j + 1) % nb, i * nb + (j + 1) % nb
            f += [(a, b, c), (a, c, d)]
    o, n, ulp = [], [], []
    rows = sorted(set(v[:nb, 2].tolist()))
    assert rows[0] == -r and rows[-1] == r and len(rows) == 9
    for z in rows:                                                       # through every row; the tangent planes are the ends
        o.append([0.0, 0.0, z]); n.append([0.0, 0.0, 1.0])
        for z1 in (math.nextafter(z, math.inf), math.nextafter(z, -math.inf)):
            ulp.append(len(o)); o.append([0.0, 0.0, z1]); n.append([0.0, 0.0, 1.0])
    for z in rows[::2]:
        o.append([2.0, 0.0, z]); n.append([0.0, 0.0, -0.5])
    # vertical planes: through two meridians, tangent to the inner equator in a vertex (two loops touch there) and either
    # side of it, tangent to the outer equator, through the hole
    for oo, nn in (([2.0, 0.0, 0.0], [0.0, 1.0, 0.0]), ([1.25, 1.5, 0.0], [1.0, 0.0, 0.0]), ([1.25, 0.0, 0.0], [-1.0, 0.0, 0.0]),
                   ([1.125, 0.0, 0.0], [1.0, 0.0, 0.0]), ([1.375, 0.0, 0.0], [1.0, 0.0, 0.0]), ([2.75, 0.0, 0.0], [1.0, 0.0, 0.0]),
                   ([2.75, 0.0, 0.0], [-1.0, 0.0, 0.0]), ([0.0, 2.0, 0.0], [2.0, 0.0, 0.0]), ([0.0, 0.0, 0.0], [1.0, 1.0, 0.0]),
                   ([1.25, 0.0, 0.0], [0.25, 0.0, 1.0]), ([1.25, 0.0, 0.0], [1.0, 0.25, 0.5])):
        o.append(oo); n.append(nn)
    # tilted planes: through the hole (two separate loops), nearly flat ones (nested pairs), and in between
    for oo in ([0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.125], [-2.0, 0.0, 0.0], [1.375, 0.0, 0.125], [1.5, 1.5, 0.25]):
        for nn in ([0.25, 0.0, 1.0], [0.5, 0.25, 1.0], [1.0, 0.0, 0.25], [1.0, 0.25, 0.5], [-0.25, 1.0, 0.5], [0.25, 0.25, -1.0]):
            o.append(oo); n.append(nn)
    assert len(o) >= 70
    return Case(v, f, o, n, lattice=True, select=True, kind="torus", ulp_planes=ulp)


def icosahedron():
    t = 1.625                                                            # the golden ratio on the 1/16 grid
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return np.array(v, dtype=float), np.array(f)


def lattice_convex(v, f):
    """planes through vertices, along edges, through faces and through the inside; origins on 1/8, normals on 1/4"""
    through, n = [], []
    centre = np.round(v.mean(axis=0) * 8.0) / 8.0
    normals = [[0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.25, 0.5, 1.0], [-1.0, 0.25, 0.0], [1.0, -1.0, 0.5]]
    for t in f[:6]:                                                      # the planes of six faces, from either side
        a, b, c = v[t]
        nn = np.cross(b - a, c - a)
        if np.array_equal(nn * 4.0, np.round(nn * 4.0)) and np.array_equal(a * 8.0, np.round(a * 8.0)):
            through += [a, a]; n += [nn, -nn]
    for oo in list(v[:5]) + [0.5 * (v[f[0][0]] + v[f[0][1]]), centre, centre + [0.125, 0.0, 0.125]]:
        if np.array_equal(oo * 8.0, np.round(oo * 8.0)):
            for nn in normals:
                through.append(oo); n.append(nn)
    vF, faces = Q.fr_rows(v), [tuple(int(i) for i in t) for t in f]
    o = [origin_off_the_loop(vF, faces, a, nn) for a, nn in zip(through, n)]
    touch = [i for i, (a, q) in enumerate(zip(through, o)) if q is None]      # a vertex or an edge alone: three are enough
    keep = [i for i in range(len(o)) if i not in touch[3:]]
    return Case(v, f, [list(through[i]) if o[i] is None else o[i] for i in keep], [n[i] for i in keep], lattice=True, select=True,
                kind="convex")


def origin_off_the_loop(vF, faces, a, n):
    """A point of the plane through a, on the 1/8 grid, that the exact section of the convex body holds in its inside --
    or, failing that, one outside it; a itself where the grid has
    neither nearby or the plane misses; None where the plane only touches.  Decided by the oracle alone."""
    aF, nF = Q.fr(a), Q.fr(n)
    cut, _s = Q.exact_cut(vF, faces, aF, nF)
    hull = Q.convex_hull([x for seg in cut.values() for _k, x in seg], nF)
    if len(hull) < 3:
        return None if hull else list(a)
    n4 = [int(round(x * 4.0)) for x in n]
    moves = sorted((w for w in np.ndindex(9, 9, 9) if sum((w[k] - 4) * n4[k] for k in range(3)) == 0),
                   key=lambda w: sum((x - 4) ** 2 for x in w))
    outside = None
    for w in moves:
        q = [float(a[k]) + (w[k] - 4) / 8.0 for k in range(3)]
        where = Q.point_in_polygon(Q.fr(q), hull, nF)
        if where == Q.INSIDE:
            return q
        if where == Q.OUTSIDE and outside is None:
            outside = q
    return outside if outside is not None else list(a)


def steps(x, ks):
    """x moved by 0, +-1, +-2, +-4 ulp and by +-8 * 2^-k: ``_steps`` of tests/test_intersect_host.py with the ulp steps
    the issue lists and size = 8, the power of two at the tube's extent (it is 9.5 long), so that k = 52 is one ulp of
    the largest coordinate and the ulp steps cover what lies below"""
    out, up, down = [x], x, x
    for i in range(1, 5):
        up, down = math.nextafter(up, math.inf), math.nextafter(down, -math.inf)
        if i != 3:
            out += [up, down]
    for k in ks:
        out += [x + 8.0 * 2.0 ** -k, x - 8.0 * 2.0 ** -k]
    return out


def near_parallel():
    """planes within rounding of a face of a jittered closed tube: the normal is the cross product of two of its edges,
    the origin a point of the face moved along the normal's dominant axis.  The first face takes every k = 30 .. 52 from
    a vertex (53 planes); the second, from the middle of an edge, every third k (23 planes), which keeps the case under
    the 100 planes a case may have"""
    v, f = tube(15, 20, 1.5, 0.5, caps=True, jitter=0.05, seed=3)
    o, n = [], []
    for face, mid, ks in ((137, False, range(30, 53)), (412, True, range(30, 53, 3))):
        a, b, c = v[f[face]]
        nn = np.cross(b - a, c - a)
        base = 0.5 * (a + b) if mid else a
        ax = int(np.argmax(np.abs(nn)))
        for x in steps(float(base[ax]), ks):
            oo = base.copy()
            oo[ax] = x
            o.append(oo); n.append(nn)
    return Case(v, f, o, n)


def near_edge():
    """planes within rounding of a supporting plane along an edge of a jittered octahedron: the loop is a needle between
    the edge's two ends whose width is rounding -- a flat loop that is not zero"""
    v, f = octahedron()
    v = v * 1.3 + np.random.default_rng(5).uniform(-0.05, 0.05, v.shape)
    o, n = [], []
    for ia, ib in ((0, 2), (1, 4), (3, 5)):
        a, b = v[ia], v[ib]
        nn = np.cross(b - a, np.cross(0.5 * (a + b), b - a))
        ax = int(np.argmax(np.abs(nn)))
        for x in steps(float(a[ax]), range(30, 53, 2)):
            oo = a.copy()
            oo[ax] = x
            o.append(oo); n.append(nn)
    return Case(v, f, o, n)


def far_origin(k):
    """two arms side by side, the thin one 1/50 of the wide one's radius and k wide radii away; the origins sit on the
    wide arm's axis"""
    v, f = join(tube(10, 5, 1.0, centre=(0.0, 0.0)), tube(10, 5, 0.02, centre=(float(k), 0.25)))
    o, n = [], []
    for x in (1.5, 2.5, 3.25):
        for nn in ([1.0, 0.0, 0.0], [1.0, 0.5 / k, 0.05], [2.0, -0.3 / k, 0.1]):
            o.append([x, 0.0, 0.0]); n.append(nn)
    return Case(v, f, o, n, closed=False, select=True)


@functools.lru_cache(maxsize=None)
def cases():
    return {"corner_loops": corner_loops((0.0, 0.0, 0.0)), "corner_loops_far": corner_loops(FAR), "lattice_torus": lattice_torus(),
            "convex_cube": lattice_convex(*cube()), "convex_octahedron": lattice_convex(*octahedron()),
            "convex_icosahedron": lattice_convex(*icosahedron()), "near_parallel": near_parallel(), "near_edge": near_edge(),
            "far_origin_1": far_origin(1), "far_origin_30": far_origin(30), "far_origin_1000": far_origin(1000)}


NAMES = ("corner_loops", "corner_loops_far", "lattice_torus", "convex_cube", "convex_octahedron", "convex_icosahedron",
         "near_parallel", "near_edge", "far_origin_1", "far_origin_30", "far_origin_1000")


# ---- the oracle's side, once per case -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    c = cases()[name]
    return Q.fr_rows(c.v), [tuple(int(i) for i in t) for t in c.f], Q.fr_rows(c.o), Q.fr_rows(c.n)


@functools.lru_cache(maxsize=None)
def exact_cuts(name):
    vF, faces, oF, nF = exact_inputs(name)
    return [Q.exact_cut(vF, faces, o, n)[0] for o, n in zip(oF, nF)]


@functools.lru_cache(maxsize=None)
def checked(name):
    return X.scan(*cases()[name].args())


def arrays_of(res):
    return {k: np.asarray(res[k] if isinstance(res, dict) else getattr(res, k)) for k in X.ARRAYS}


def hooks(name):
    """the host hooks on a case, equal to the checker bit for bit"""
    v, f, o, n = cases()[name].args()
    seg = S.section_cut_host((v, f), o, n)
    assert seg.tobytes() == X.to_records(checked(name)["segments"]).tobytes()
    got = S.section_chain(seg, o, n)
    same_arrays(got, checked(name))
    return got


# ---- E1 to E7 on a result -------------------------------------------------------------------------------------------

def box_holds(pts, q, grow):
    return all(min(p[k] for p in pts) - grow <= q[k] <= max(p[k] for p in pts) + grow for k in range(3))


FLAT, ROUND, EITHER = "flat", "round", "either"


def flatness(pts, n):
    """The oracle's say on rule 6's flat condition, from the exact W and the exact B (``fan_magnitude``) of the listed
    points: the rule's W is within half its threshold T = (m + 6) eps B of the exact one, so a loop with
    |W| <= 0.4 T must be taken for flat and one with |W| >= 1.6 T must not (0.5 and 1.5 less the rounding of B itself
    and the second-order terms); in between either is right.  Returns (FLAT | ROUND | EITHER, exact W, exact B)."""
    W, B = sum(Q.fan_weights(pts, n)), Q.fan_magnitude(pts, n)
    T = (len(pts) + 6) * F(EPS) * B
    return (FLAT if 10 * abs(W) <= 4 * T else ROUND if 10 * abs(W) >= 16 * T else EITHER), W, B


def centroid_check(fl, pts, n, cen, scale):
    """E6 on one closed loop: fl its listed points, pts the same as rationals, cen the reported centroid.  Which branch
    to ask for is the oracle's say (``flatness``).  Returns the zone, {check: text} of what failed -- E6f the box of a
    flat loop (where either branch is right, one of the two), E6d the derived bound on a loop that is not flat, E6 the
    issue's form there -- and {check: error over its bound without the constant}."""
    zone, Wx, Bx = flatness(pts, n)
    in_flat_box = box_holds(fl, cen, C1 * EPS * scale)
    if zone == FLAT:
        return zone, ({} if in_flat_box else {"E6f": "flat (exact |W| / B = %.3g), centroid %r outside the loop's box"
                                                     % (float(abs(Wx) / Bx) if Bx else 0.0, cen)}), {}
    m, w, cx = len(fl), Q.fan_weights(pts, n), Q.centroid(pts, n)
    D = math.sqrt(sum((max(q[k] for q in fl) - min(q[k] for q in fl)) ** 2 for k in range(3)))
    err6 = math.sqrt(float(sum((F(cen[k]) - cx[k]) ** 2 for k in range(3)))) if np.isfinite(cen).all() else math.inf
    rho = float(sum(abs(x) for x in w) / abs(Wx))
    unit = m * EPS * D * rho
    stored = EPS * max(abs(x) for q in fl for x in q)                    # the centroid is rounded where its coordinates are
    bound6d = EPS * D * (0.5 * (m + 10) * float(Bx / abs(Wx)) * (1.0 + rho) + 1.0) + stored          # derived
    if zone == EITHER:
        return zone, ({} if in_flat_box or err6 <= bound6d else
                      {"E6f": "neither the mean of a flat loop nor within %.3g of the centroid: %r" % (bound6d, cen)}), {}
    texts = {}
    if not err6 <= bound6d:
        texts["E6d"] = "centroid off by %.3g, derived bound %.3g (loop size %.3g)" % (err6, bound6d, D)
    if not err6 <= C4 * unit + stored:
        texts["E6"] = "centroid off by %.3g, bound %.3g (loop size %.3g)" % (err6, C4 * unit + stored, D)
    elif not box_holds(fl, cen, C4 * unit + stored):
        texts["E6"] = "centroid %r outside the loop's box" % (cen,)
    return zone, texts, {"E6d": err6 / bound6d, "E6": max(0.0, err6 - stored) / unit if unit > 0 else 0.0}


_evaluated = {}


def evaluate(name, res):
    """{"fails": {E: [text]}, "worst": {E: ratio of the error to its bound without the constant}, ...}; a function of the
    arrays alone, so equal bits are judged once"""
    A = arrays_of(res)
    key = (name, hashlib.sha256(b"".join(A[k].tobytes() for k in X.ARRAYS)).hexdigest())
    if key not in _evaluated:
        _evaluated[key] = _evaluate(name, A)
    return _evaluated[key]


def _evaluate(name, A):
    c = cases()[name]
    vF, faces, oF, nF = exact_inputs(name)
    fails = {"E%d" % k: [] for k in range(1, 8)}
    fails["E5d"], fails["E6d"], fails["E6f"] = [], [], []
    worst = {"E1": 0.0, "E2": 0.0, "E5": 0.0, "E6": 0.0, "E5d": 0.0, "E6d": 0.0}
    off, P = A["contour_off"].tolist(), len(c.o)
    scale = float(np.abs(c.v).max())
    loops = [[] for _ in range(P)]                                      # per plane: (contour, exact points, exact area, E5 bound)
    crossed = [set() for _ in range(P)]
    zones = {FLAT: 0, ROUND: 0, EITHER: 0}
    for ct in range(len(off) - 1):
        p, kind = int(A["contour_plane"][ct]), int(A["contour_kind"][ct])
        o, n, where = oF[p], nF[p], "%s plane %d contour %d" % (name, p, ct)
        idx = list(range(off[ct], off[ct + 1]))
        pts = [Q.fr(A["points"][i]) for i in idx]
        for i, x in zip(idx, pts):
            lo, hi = (int(e) for e in A["point_edge"][i])
            a, b = vF[lo], vF[hi]
            M = max(abs(t) for t in a + b)                              # E1
            d2 = Q.dist2_to_segment(x, a, b)
            if d2 > (F(C1) * F(EPS) * M) ** 2:
                fails["E1"].append("%s point %d: %.3g from its edge, bound %.3g" % (where, i, math.sqrt(float(d2)), C1 * EPS * float(M)))
            if M > 0:
                worst["E1"] = max(worst["E1"], math.sqrt(float(d2)) / (EPS * float(M)))
            h = Q.height(o, n, x)                                       # E2
            room = sum(abs(n[k]) * (abs(a[k] - o[k]) + abs(b[k] - o[k]) + max(abs(a[k]), abs(b[k]))) for k in range(3))
            if abs(h) > F(C2) * F(EPS) * room:
                fails["E2"].append("%s point %d: height %.3g, bound %.3g" % (where, i, float(h), C2 * EPS * float(room)))
            if room > 0:
                worst["E2"] = max(worst["E2"], float(abs(h) / (F(EPS) * room)))
        m = len(idx)
        if c.closed:                                                    # E3
            if kind != X.CLOSED:
                fails["E3"].append("%s: kind %d on closed manifold input" % (where, kind))
        if kind == X.CLOSED:
            for j, i in enumerate(idx):
                face = int(A["point_face"][i])
                tri, k0, k1 = set(faces[face]), A["point_edge"][i].tolist(), A["point_edge"][idx[(j + 1) % m]].tolist()
                if not (set(k0) <= tri and set(k1) <= tri and k0 != k1):
                    fails["E3"].append("%s: points %d and its successor are not on two edges of face %d" % (where, i, face))
                if face in crossed[p]:
                    fails["E3"].append("%s: face %d appears twice" % (where, face))
                crossed[p].add(face)
        if kind != X.CLOSED:
            continue
        fl = [A["points"][i].tolist() for i in idx]
        D = math.sqrt(sum((max(q[k] for q in fl) - min(q[k] for q in fl)) ** 2 for k in range(3)))
        s2 = Q.signed_area_times_norm(pts, n)
        exact_area = s2 / F(Q.norm64(n))
        area = float(A["contour_area"][ct])
        bound5 = C3 * m * EPS * D * D
        if s2 < 0:                                                      # E4
            fails["E4"].append("%s: listed clockwise about n, exact area %.3g (reported %.3g)" % (where, float(exact_area), area))
        if s2 == 0 and not area <= bound5:
            fails["E4"].append("%s: exact area 0, reported %.3g, bound %.3g" % (where, area, bound5))
        err5 = abs(F(area) - exact_area) if math.isfinite(area) else F(10) ** 300       # E5
        if err5 > F(bound5):
            fails["E5"].append("%s: area %.17g, exact %.17g, error %.3g, bound %.3g" % (where, area, float(exact_area), float(err5), bound5))
        if D > 0:
            worst["E5"] = max(worst["E5"], float(err5) / (m * EPS * D * D))
        bound5d = 0.25 * (m + 6) * EPS * float(Q.fan_magnitude(pts, n)) / Q.norm64(n) + EPS * abs(float(exact_area))   # derived
        if err5 > F(bound5d):
            fails["E5d"].append("%s: area error %.3g, derived bound %.3g" % (where, float(err5), bound5d))
        if bound5d > 0:
            worst["E5d"] = max(worst["E5d"], float(err5) / bound5d)
        loops[p].append((ct, pts, exact_area, bound5))
        zone, texts, ratios = centroid_check(fl, pts, n, A["contour_centroid"][ct].tolist(), scale)       # E6
        zones[zone] += 1
        for e, text in texts.items():
            fails[e].append("%s: %s" % (where, text))
        for e, x in ratios.items():
            worst[e] = max(worst[e], x)
    cuts = exact_cuts(name) if c.lattice else None
    if c.lattice:                                                       # E3: the crossed set from exact sides
        for p in range(P):
            if crossed[p] != set(cuts[p]):
                fails["E3"].append("%s plane %d: crossed faces differ from the exact sides' by %r" % (name, p, sorted(crossed[p] ^ set(cuts[p]))))
    left_out = []
    if c.select:                                                        # E7
        for p in range(P):
            where_o = [Q.point_in_polygon(oF[p], pts, nF[p]) for _ct, pts, _a, _b in loops[p]]
            if Q.BOUNDARY in where_o:
                left_out.append(p)
                continue
            holds = [lp for lp, w_o in zip(loops[p], where_o) if w_o == Q.INSIDE]
            want = {lp[0] for lp in holds if lp[2] == min(x[2] for x in holds)} or {-1}
            if int(A["selected"][p]) not in want:
                fails["E7"].append("%s plane %d: selected %d, the oracle %r" % (name, p, int(A["selected"][p]), sorted(want)))
        if len(left_out) * 10 > P:
            fails["E7"].append("%s: %d of %d planes have their origin on a loop: %r" % (name, len(left_out), P, left_out))
    skipped_nesting = 0
    for p in range(P) if c.kind else ():                                # E5 against a section that needs no chaining
        o, n = oF[p], nF[p]
        norm = F(Q.norm64(n))
        slack = sum(b for _ct, _pts, _a, b in loops[p])
        if c.kind == "convex":
            hull = Q.convex_hull([x for seg in cuts[p].values() for _k, x in seg], n)
            want = abs(Q.signed_area_times_norm(hull, n)) / norm if len(hull) >= 3 else F(0)
            got = sum(F(float(A["contour_area"][ct])) for ct, _pts, _a, _b in loops[p])
            slack += C1 * EPS * scale * (Q.polygon_length(hull) if len(hull) >= 2 else 0.0)
            if len(loops[p]) > 1:
                fails["E5"].append("%s plane %d: %d loops on a convex body" % (name, p, len(loops[p])))
        else:
            signs = nesting_signs([pts for _ct, pts, _a, _b in loops[p]], n)
            if signs is None:
                skipped_nesting += 1
                continue
            want = Q.section_area_times_norm(cuts[p], n) / norm
            got = sum(sg * F(float(A["contour_area"][ct])) for sg, (ct, _pts, _a, _b) in zip(signs, loops[p]))
            slack += C1 * EPS * scale * sum(float(A["contour_length"][ct]) for ct, _pts, _a, _b in loops[p])
        if abs(got - want) > F(slack):
            fails["E5"].append("%s plane %d: the section's area %.17g, exact %.17g, bound %.3g" % (name, p, float(got), float(want), slack))
    return {"fails": fails, "worst": worst, "n_loops": sum(len(x) for x in loops), "zones": zones, "left_out": len(left_out),
            "skipped_nesting": skipped_nesting}


def nesting_signs(polys, n):
    """+1 for a loop inside an even number of the others, -1 for a hole; None where a loop has no vertex off the others'
    boundaries (coincident loops, as on a tangent plane)"""
    signs = []
    for i, pts in enumerate(polys):
        others = [q for j, q in enumerate(polys) if j != i]
        for x in pts:
            where = [Q.point_in_polygon(x, q, n) for q in others]
            if Q.BOUNDARY not in where:
                signs.append(-1 if where.count(Q.INSIDE) % 2 else 1)
                break
        else:
            return None
    return signs


ALL_E = ("E1", "E2", "E3", "E4", "E5", "E5d", "E6", "E6d", "E6f", "E7")


def judge(name, res, which=ALL_E):
    """E6 is the issue's form on a loop that is not flat, E6d the derived form there, E6f the box of a flat loop (and,
    where the oracle allows either branch, one of the two).  near_edge is this file's own case, not the issue's: its
    needles have sum|w| / |W| = 1 and a centroid whose conditioning is B / |W| ~ length / width, so the issue's form
    cannot hold there; the derived one and the flat box stand."""
    r = evaluate(name, res)
    if name == "near_edge":
        which = tuple(e for e in which if e != "E6")
    print("%s: %d closed loops (%d flat, %d either), worst E1 %.3g of %g, E2 %.3g of %g, E5 %.3g of %g, E6 %.3g of %g, derived E5 %.3g "
          "of 1, derived E6 %.3g of 1; %d planes left out of E7, %d out of the nesting check"
          % (name, r["n_loops"], r["zones"][FLAT], r["zones"][EITHER], r["worst"]["E1"], C1, r["worst"]["E2"], C2, r["worst"]["E5"], C3,
             r["worst"]["E6"], C4, r["worst"]["E5d"], r["worst"]["E6d"], r["left_out"], r["skipped_nesting"])
          + (" (the issue's form of E6 is not asserted here)" if name == "near_edge" else ""))
    for e in which:
        assert not r["fails"][e], (e, len(r["fails"][e]), r["fails"][e][:6])
    return r


# ---- the tests ------------------------------------------------------------------------------------------------------

def test_the_oracle_on_known_polygons():
    sq = Q.fr_rows([[0, 0, 5], [1, 0, 5], [1, 1, 5], [0, 1, 5]])
    n = Q.fr([0, 0, 2])
    assert Q.signed_area(sq, n) == 1 and Q.signed_area(sq[::-1], n) == -1 and Q.centroid(sq, n) == (F(1, 2), F(1, 2), F(5))
    far = [tuple(x + F(10) ** 30 for x in p) for p in sq]
    assert Q.signed_area(far, n) == 1                                   # translation-free
    assert Q.point_in_polygon(Q.fr([0.5, 0.5, 5]), sq, n) == Q.INSIDE and Q.point_in_polygon(Q.fr([1.5, 0.5, 5]), sq, n) == Q.OUTSIDE
    assert Q.point_in_polygon(Q.fr([1, 0.25, 5]), sq, n) == Q.BOUNDARY and Q.point_in_polygon(Q.fr([1, 1, 5]), sq, n) == Q.BOUNDARY
    assert Q.dist2_to_segment(Q.fr([2, 1, 5]), sq[0], sq[1]) == 2 and Q.dist2_to_segment(Q.fr([0.5, 1, 5]), sq[0], sq[1]) == 1
    hull = Q.convex_hull(sq + Q.fr_rows([[0.5, 0.5, 5], [0.5, 0, 5]]), n)
    assert sorted(hull) == sorted(sq) and abs(Q.signed_area(hull, n)) == 1
    assert Q.side(Q.height(Q.fr([0, 0, 1]), n, Q.fr([3, 3, 1]))) == 1 and Q.side(F(-1, 10 ** 30)) == 0
    assert Q.crossing(Q.fr([0, 0, 0]), Q.fr([0, 0, 3]), F(-1), F(2)) == (0, 0, 1)


@pytest.mark.parametrize("name", ["lattice_torus", "convex_cube", "convex_octahedron", "convex_icosahedron"])
def test_lattice_inputs_have_exact_heights(name):
    """the precondition, on the inputs alone: the f64 height of rule 1 is the exact height of every (plane, vertex), so
    the oracle's sides are the rule's.  A plane one ulp off a row cannot have that for the other rows (z - o.z rounds);
    there the two sides agree, and the height of the row itself is exact."""
    c = cases()[name]
    vF, faces, oF, nF = exact_inputs(name)
    assert np.array_equal(c.v * 64.0, np.round(c.v * 64.0))
    for p, (o, n) in enumerate(zip(c.o.tolist(), c.n.tolist())):
        if p not in c.ulp_planes:
            grid = 64.0 if sum(x != 0.0 for x in n) == 1 else 8.0         # a plane through a row sits on the vertices' grid
            assert all(x * grid == round(x * grid) for x in o) and all(x * 4.0 == round(x * 4.0) for x in n)
        near = 0
        for x, xF in zip(c.v.tolist(), vF):
            h, hx = X.height(o, n, x), Q.height(oF[p], nF[p], xF)
            if p in c.ulp_planes:
                assert X.side(h) == Q.side(hx)
                near += abs(hx) < 1e-15 and F(h) == hx
            else:
                assert F(h) == hx
        assert p not in c.ulp_planes or near >= 20
    # closed, outward: every directed edge once and its reverse once; a positive volume
    directed = [(t[k], t[(k + 1) % 3]) for t in faces for k in range(3)]
    assert len(set(directed)) == len(directed) and {(b, a) for a, b in directed} == set(directed)
    assert sum(Q.dot(vF[t[0]], Q.cross(vF[t[1]], vF[t[2]])) for t in faces) > 0
    if c.kind == "convex":
        for t in faces:
            nf = Q.cross(Q.sub(vF[t[1]], vF[t[0]]), Q.sub(vF[t[2]], vF[t[0]]))
            assert all(Q.dot(nf, Q.sub(x, vF[t[0]])) <= 0 for x in vF)


@pytest.mark.parametrize("impl", ["checker", "hooks"])
@pytest.mark.parametrize("name", NAMES)
def test_exact_cut(name, impl):
    res = checked(name) if impl == "checker" else hooks(name)
    r = judge(name, res)
    A, c = arrays_of(res), cases()[name]
    if name == "corner_loops":                                          # the loops of the issue's table are there
        for i in range(0, 16, 4):
            ct = int(A["plane_off"][i])
            assert A["plane_off"][i + 1] == ct + 1 and A["contour_off"][ct + 1] - A["contour_off"][ct] == 6
    if name == "lattice_torus":
        per_plane = np.diff(A["plane_off"])
        assert (per_plane >= 2).sum() >= 20 and r["skipped_nesting"] <= 4 and r["n_loops"] > 100
    if name.startswith("far_origin"):
        assert (np.diff(A["plane_off"]) == 2).all() and (A["selected"] >= 0).all()
    if name == "near_parallel":
        assert r["n_loops"] >= len(c.o) // 2
    if name == "near_edge":
        assert r["zones"][FLAT] >= 3 and r["zones"][ROUND] >= 10       # needles on either side of the condition


def collinear_loops(count=1000, seed=11):
    """Closed loops of 4 to 8 f64 points that lie on one line exactly (integers p_0 + t u, scaled by 2^-53), built so
    that p_i - p_0 is not an f64: p_0 sits just inside -1 (against u) and the others beyond 0, and the difference of two
    53-bit numbers of opposite sign needs 54 bits.  Their exact W is 0; the rule's d_i are rounded, so its w_i are noise
    of either sign.  As the segments of one plane, each loop a component of its own."""
    rng = np.random.default_rng(seed)
    segs, loops, key = [], [], 0
    for _ in range(count):
        m = int(rng.integers(4, 9))
        u = [int(x) for x in rng.integers(1, 8, 3) * rng.choice([-1, 1], 3)]
        p0 = [(-1 if x > 0 else 1) * (2 ** 53 - 1 - 2 * int(j)) for x, j in zip(u, rng.integers(0, 1000, 3))]
        tmax = min((2 ** 53 - 1 + abs(p0[k])) // abs(u[k]) for k in range(3))
        ts = [0] + [int(t) for t in rng.integers(tmax // 2, tmax, m - 1)]
        ints = [[p0[k] + t * u[k] for k in range(3)] for t in ts]
        assert all(abs(x) < 2 ** 53 for p in ints for x in p)
        pts = [tuple(float(x) * 2.0 ** -53 for x in p) for p in ints]
        keys = [(key + i, key + i + 1) for i in range(m)]
        for i in range(m):
            j = (i + 1) % m
            (ka, pa), (kb, pb) = sorted([(keys[i], pts[i]), (keys[j], pts[j])])
            segs.append((0, len(segs), ka, kb, pa, pb))
        loops.append(pts)
        key += m + 1
    return segs, loops


def test_collinear_loops_whose_sum_is_rounding_noise_are_flat():
    """The flat condition itself.  The exact W of every loop here is 0, so the oracle calls it flat and its centroid
    has to lie in its box (E6, flat branch); its reported area is noise within E5's bounds (E4, second clause).  The
    rule's own W is a nonzero sum of noise on about half of them, and on some of those p_0 + G / (3 W) lies outside
    the box by up to twice its size -- asserted here as the premise, from the rule's sums on the listed points -- so
    a rule that is flat only where W == 0.0 fails this test."""
    segs, loops = collinear_loops()
    o, n = [0.0, 0.0, 0.0], [1.0, 0.5, -0.25]
    contours, _best = X.chain_plane(segs, o, n)
    got = S.section_chain(X.to_records(segs), [o], [n])
    assert len(contours) == len(loops) and all(ct["kind"] == X.CLOSED for ct in contours)
    assert X.same_bits(got.contour_centroid, np.array([ct["centroid"] for ct in contours]))
    assert X.same_bits(got.contour_area, np.array([ct["area"] for ct in contours]))
    assert X.same_bits(got.points, np.array([p for ct in contours for p in ct["points"]]))
    nF, norm = Q.fr(n), Q.norm64(n)
    noisy = misplaced = 0
    for ct, mine in zip(contours, loops):
        fl = [list(p) for p in ct["points"]]
        assert sorted(map(tuple, fl)) == sorted(mine) and tuple(fl[0]) == mine[0]
        pts, m = Q.fr_rows(fl), len(fl)
        zone, Wx, Bx = flatness(pts, nF)
        assert Wx == 0 and zone == FLAT and Q.vector_area(pts) == (0, 0, 0)
        grow = C1 * EPS * 1.0
        assert box_holds(fl, ct["centroid"], grow), (fl, ct["centroid"])
        D = math.sqrt(sum((max(q[k] for q in fl) - min(q[k] for q in fl)) ** 2 for k in range(3)))
        assert abs(ct["area"]) <= min(C3 * m * EPS * D * D, 0.25 * (m + 6) * EPS * float(Bx) / norm), (fl, ct["area"])
        _s, W, _B, G = X.loop_signed(fl, n)                             # the premise: what W == 0.0 alone would let through
        if W != 0.0:
            noisy += 1
            misplaced += not box_holds(fl, [fl[0][k] + G[k] / (3.0 * W) for k in range(3)], grow)
    print("collinear loops: %d of %d have a nonzero W of noise; p_0 + G / (3 W) leaves the box of %d" % (noisy, len(loops), misplaced))
    assert noisy >= len(loops) // 4 and misplaced >= 5


def thin_triangles(seed=17):
    """Triangles p_0, p_0 + u, p_0 + s u + 2^-k v of width 2^-k over length 1, k = 20 .. 56, in random directions: the
    area centroid lies at (1 + s) / 3 along u and the length-weighted mean at 1 / 2, |2 s - 1| / 6 apart (s is 0.1 or
    0.9), so taking a loop that is not flat for flat shows.  As the segments of one plane each, with the plane's normal."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(20, 57):
        for s in (0.1, 0.9, 0.1, 0.9):
            u, v = rng.normal(size=3), rng.normal(size=3)
            u /= np.linalg.norm(u)
            v -= u * (u @ v)
            v /= np.linalg.norm(v)
            p0 = rng.uniform(-1.0, 1.0, 3)
            pts = [tuple(p0.tolist()), tuple((p0 + u).tolist()), tuple((p0 + s * u + 2.0 ** -k * v).tolist())]
            segs = []
            for i in range(3):
                (ka, pa), (kb, pb) = sorted([((i, i + 1), pts[i]), (((i + 1) % 3, (i + 1) % 3 + 1), pts[(i + 1) % 3])])
                segs.append((0, i, ka, kb, pa, pb))
            out.append((k, segs, p0.tolist(), np.cross(u, v).tolist()))
    return out


def test_thin_triangles_are_flat_only_below_the_condition():
    """The other side of the flat condition: needles whose mean is not their centroid.  Where the oracle says the loop
    is not flat (``flatness``: exact |W| >= 1.6 T) the centroid is within the derived bound of E6 of the exact one.  The
    length-weighted mean is 0.13 of the triangle away from it, and the bound, which grows with B / |W|, falls below that
    some way above the condition: with the checker's factor made 30 times larger this test fails on five triangles (widths
    2^-45 to 2^-48), with 4 times it does not -- that close to the condition the centroid is no better known than the
    mean.  Where the oracle says flat, the centroid is in the box; in between, one of the two."""
    zones, worst = {FLAT: 0, ROUND: 0, EITHER: 0}, 0.0
    for k, segs, o, n in thin_triangles():
        contours, _best = X.chain_plane(segs, o, n)
        got = S.section_chain(X.to_records(segs), [o], [n])
        assert len(contours) == 1 and contours[0]["kind"] == X.CLOSED
        assert X.same_bits(got.contour_centroid, np.array([contours[0]["centroid"]]))
        assert X.same_bits(got.points, np.array(contours[0]["points"]))
        fl = [list(p) for p in contours[0]["points"]]
        zone, texts, ratios = centroid_check(fl, Q.fr_rows(fl), Q.fr(n), contours[0]["centroid"], 2.0)
        assert not texts.get("E6f") and not texts.get("E6d"), (k, zone, texts)
        zones[zone] += 1
        worst = max(worst, ratios.get("E6d", 0.0))
        assert zone == ROUND or k > 46, (k, zone)                      # B <= 2 sqrt(3) |d||e|, so |W| / B >= 2^-48 there
    print("thin triangles: %r, worst derived E6 %.3g of 1" % (zones, worst))
    assert zones[ROUND] >= 100 and zones[FLAT] >= 4


def loop_fields(ct):
    return (ct["kind"], ct["keys"], ct["faces"], ct["points"], ct["area"], ct["length"], ct["centroid"])


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), FAR])
def test_moving_the_origin_in_its_plane_changes_the_selection_alone(shift):
    """E8: the segments of the plane of off = 0, chained with the origin of every off: points, order, areas, lengths and
    centroids equal to the bit.  (The planes of two values of off are not the same plane in f64 -- o.x + o.y rounds --
    so the cut itself is not repeated.)"""
    v, f = cube()
    v = v + np.array(shift)
    n = [1.0, 1.0, 1.0]
    for delta in DELTAS:
        o0 = corner_origin(delta, 0.0, shift)
        segs, _skipped = X.segments(v, f, [o0], [n])
        rec = S.section_cut_host((v, f), [o0], [n])
        assert rec.tobytes() == X.to_records(segs).tobytes()
        want = X.chain_plane(segs, o0, n)[0]
        first = S.section_chain(rec, [o0], [n])
        assert len(want) == 1 and want[0]["kind"] == X.CLOSED
        for off in OFFS[1:]:
            o = corner_origin(delta, off, shift)
            got = X.chain_plane(segs, o, n)[0]
            assert [loop_fields(ct) for ct in got] == [loop_fields(ct) for ct in want], (delta, off)
            moved = S.section_chain(rec, [o], [n])
            for k in X.ARRAYS:
                assert k == "selected" or X.same_bits(getattr(moved, k), getattr(first, k)), (delta, off, k)


def records_of(res, p):
    """The segment records of plane p rebuilt from a result's closed loops, as plane 0: what ``section_chain`` takes."""
    A = arrays_of(res)
    segs = []
    for ct in range(int(A["plane_off"][p]), int(A["plane_off"][p + 1])):
        assert A["contour_kind"][ct] == X.CLOSED
        a, m = int(A["contour_off"][ct]), int(A["contour_off"][ct + 1] - A["contour_off"][ct])
        for i in range(m):
            j = (i + 1) % m
            ends = sorted([(tuple(A["point_edge"][a + i].tolist()), tuple(A["points"][a + i].tolist())),
                           (tuple(A["point_edge"][a + j].tolist()), tuple(A["points"][a + j].tolist()))])
            segs.append((0, int(A["point_face"][a + i]), ends[0][0], ends[1][0], ends[0][1], ends[1][1]))
    return X.to_records(sorted(segs, key=lambda s: s[1]))


def origin_moves_nothing_but_the_selection(name, res):
    """E8 on a finished result of the corner loops: the loops of every plane, chained anew from their own records about
    the origin of off = 0 of the same delta, are the same bits"""
    A, c = arrays_of(res), cases()[name]
    for p in range(len(c.o)):
        lo, hi = int(A["plane_off"][p]), int(A["plane_off"][p + 1])
        if hi == lo:
            continue
        again = S.section_chain(records_of(res, p), [c.o[p - p % 4]], [c.n[p]])
        a, b = int(A["contour_off"][lo]), int(A["contour_off"][hi])
        for k, sl in (("points", slice(a, b)), ("point_edge", slice(a, b)), ("point_face", slice(a, b)), ("contour_area", slice(lo, hi)),
                      ("contour_length", slice(lo, hi)), ("contour_centroid", slice(lo, hi)), ("contour_kind", slice(lo, hi))):
            assert X.same_bits(getattr(again, k), A[k][sl]), (name, p, k)


@pytest.mark.parametrize("name", ["corner_loops", "corner_loops_far"])
def test_a_result_chained_anew_about_another_origin(name):
    origin_moves_nothing_but_the_selection(name, hooks(name))
