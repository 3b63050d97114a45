"""Worst cases for the three promises of the winding number (include/mm_ccta.h, "winding number"): `touch` catches every
query whose face may sit on the wrong side of its 2 pi jump, `err` bounds |w - exact|, and the rule does not depend on the
scale of the coordinates.  Shared by tests/test_winding_attack_host.py (checker and host hook, no device) and
tests/test_gpu_winding_attack.py (the device against the checker).  Plain numpy and integer arithmetic; every family is
seeded, and the checker (tests/mm_checkers/winding_number.py) runs once per case and process.

The exact oracle.  A double is an integer times a power of two, so the twelve coordinates of (p, A, B, C) are integers at
a common scale and a . (b x c) of their exact differences is an integer: `exact_num` returns it as a Fraction, `over_face`
says whether p's projection along the face normal lies in the closed triangle, and `owner_classes` puts every query into
one of ON (exactly on the closed face), PLANE_OUT (exactly in the plane, outside the closed triangle) and OFF.

The value reference stays chk.reference (80-bit long double).  It is trusted for a query only where every owner face
has an exact |num| / L of at least 2^-58 (the long-double num is off by a few 2^-64 L) or is PLANE_OUT, where that face's
term is continuous.  A query that is ON has no value: the only acceptable answer is err = inf.

Families (name -> `get(name)` = (points, vertices, faces), `meta(name)` = what the tests need to know about them):
* ladder_*: `plane_ladder` -- through every stride-th face, three interior base points, and through every second of those
  faces its three edge midpoints and three corners too; each base snapped to the double nearest the face's plane along
  the normal's dominant axis, then moved along that axis by 0, +-1..8 ulp and +-size 2^-k, k = 36..52 (51 rungs).  On
  sphere512 (stride 16), the open tube (stride 18) and sphere512 translated by (1e4, -2e4, 3e4), flattened by
  (1, 1, 2^-20) and needled by (1, 2^-12, 2^-24).  The edge and corner ladders take every second face only because the
  long-double reference over them is the slowest step of the host tests.
* wrong_sign_*: `wrong_sign_grid` -- faces with corners of magnitude 20 passing over (0.5, 0.5, 0.5), after Kettner et
  al., "Classroom examples of robustness problems in geometric computations": queries on a grid of one-ulp steps whose
  dominant coordinate is solved exactly and rounded, where the f64 sign of num is often wrong or zero.
* scaled_<k>: ladder_sphere times 2^k, exact.
* lattice_box, lattice_box_inward, lattice_octahedron: half-integer grids around solids with integer corners -- queries
  exactly on faces, edges, corners and on extended planes, and exact ties on the boundaries of `cone`.
* cover_five, cover_cancel, cover_nested: |w| > 1, w = 0 by cancellation, w in {0, 1, 2}.
* cone_ties, cone_tie_<i>: faces with integer den and num exactly on the boundaries between the cases of `cone`
  (im = +-re, re = 0), where the lattices above turned out to have none.
* limit_box: a box with corners at +-2^300, the coordinate limit, and queries inside, on a face and on a corner.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import winding_cases as wc
from mm_checkers import winding_number as chk

ON, PLANE_OUT, OFF = 0, 1, 2
TRUST_LOG2 = -58.0
ULP_STEPS = tuple(range(-8, 9))                                     # 0 included
POWER_STEPS = tuple(range(36, 53))
SCALES = (-299, -200, -180, -150, 250, 298)
SCALES_IDENTICAL = (-150, 250, 298)
GRID_FACES, GRID_HALF, GRID_ULPS = 24, 12, (-2, -1, 0, 1, 2)        # 24 faces x 25 x 25 x 5 = 75 000 queries
TRANSLATION = (1.0e4, -2.0e4, 3.0e4)


# ---- the exact oracle -------------------------------------------------------------------------------------------------

def _ints(vals):
    """the doubles as integers at one common power of two: ([int], e) with val = int * 2^e"""
    fr = [math.frexp(float(x)) for x in vals]
    es = [e - 53 for m, e in fr if m != 0.0]
    e0 = min(es) if es else 0
    return [(int(math.ldexp(m, 53)) << (e - 53 - e0)) if m != 0.0 else 0 for m, e in fr], e0


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _corners(p, A, B, C):
    z, e = _ints(list(p) + list(A) + list(B) + list(C))
    return tuple(z[0:3]), tuple(z[3:6]), tuple(z[6:9]), tuple(z[9:12]), e


def _num_int(p, A, B, C):
    p, A, B, C, e = _corners(p, A, B, C)
    return _dot(_sub(A, p), _cross(_sub(B, p), _sub(C, p))), 3 * e


def exact_num(p, A, B, C):
    """a . (b x c) of the exact differences a = A - p, b = B - p, c = C - p of the doubles, as a Fraction"""
    n, e = _num_int(p, A, B, C)
    return Fraction(n) * Fraction(2) ** e


def over_face(p, A, B, C):
    """exact: does the projection of p along the face normal lie in the closed triangle (the three edge determinants
    against the normal, as test_intersect_host.segment_in_triangle)"""
    p, A, B, C, _ = _corners(p, A, B, C)
    n = _cross(_sub(B, A), _sub(C, A))
    return all(_dot(_cross(_sub(w, u), _sub(p, u)), n) >= 0 for u, w in ((A, B), (B, C), (C, A)))


def _log2_int(n):
    n = abs(n)
    if n == 0:
        return -math.inf
    shift = max(0, n.bit_length() - 62)
    return math.log2(n >> shift) + shift


def rule_terms(p, A, B, C):
    """(num, den, L) of the rule in f64, in the header's order; p, A, B, C (n, 3), one face a query"""
    a, b, c = A - p, B - p, C - p
    d = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]                  # noqa: E731
    with np.errstate(over="ignore", under="ignore"):
        la, lb, lc = np.sqrt(d(a, a)), np.sqrt(d(b, b)), np.sqrt(d(c, c))
        L = (la * lb) * lc
        ux, uy, uz = (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2],
                      b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
        num = (a[:, 0] * ux + a[:, 1] * uy) + a[:, 2] * uz
        den = ((la * lb) * lc + d(a, b) * lc) + (d(b, c) * la + d(c, a) * lb)
    return num, den, L


def _rule_L(p, A, B, C):
    """L of the rule for one query and face: Python floats are unfused f64"""
    def length(x):
        dx, dy, dz = x[0] - p[0], x[1] - p[1], x[2] - p[2]
        return math.sqrt((dx * dx + dy * dy) + dz * dz)
    return (length(A) * length(B)) * length(C)


def owner_classes(points, v, f, owners):
    """Every query against its owner faces (a list of face indices a query).  Returns dict: `cls` (the class against
    the first owner), `on` (ON for any owner), `trusted` (every owner is PLANE_OUT or has exact |num| / L >= 2^-58),
    `sign` (int8, the exact sign of num for the first owner), `over` (over_face for the first owner), `log2_ratio`
    (log2 of the exact |num| / L for the first owner, -inf for 0, L the rule's f64 value)."""
    nq = points.shape[0]
    cls, sign = np.full(nq, OFF, dtype=np.int8), np.zeros(nq, dtype=np.int8)
    on, trusted, over = np.zeros(nq, dtype=bool), np.ones(nq, dtype=bool), np.zeros(nq, dtype=bool)
    ratio = np.full(nq, -np.inf)
    P, V, F = points.tolist(), v.tolist(), f.tolist()
    for i in range(nq):
        p = P[i]
        for j, face in enumerate(owners[i]):
            A, B, C = V[F[face][0]], V[F[face][1]], V[F[face][2]]
            n, e = _num_int(p, A, B, C)
            if n == 0:
                k = ON if over_face(p, A, B, C) else PLANE_OUT
                r = -math.inf
            else:
                k = OFF
                Lf = _rule_L(p, A, B, C)
                r = _log2_int(n) + e - math.log2(Lf) if Lf > 0.0 else math.inf
            on[i] |= k == ON
            trusted[i] &= (k == PLANE_OUT) or (k == OFF and r >= TRUST_LOG2)
            if j == 0:
                cls[i], sign[i], ratio[i] = k, (n > 0) - (n < 0), r
                over[i] = (k == ON) or (k == OFF and over_face(p, A, B, C))
    return {"cls": cls, "on": on, "trusted": trusted, "sign": sign, "over": over, "log2_ratio": ratio}


# ---- plane ladders ----------------------------------------------------------------------------------------------------

def _snap_to_plane(p, A, B, C, axis):
    """p with its `axis` coordinate replaced by the double nearest the plane of (A, B, C) through the other two"""
    z, e = _ints(list(p) + list(A) + list(B) + list(C))
    P, a, b, c = z[0:3], z[3:6], z[6:9], z[9:12]
    n = _cross(_sub(b, a), _sub(c, a))
    m1, m2 = (axis + 1) % 3, (axis + 2) % 3
    x = Fraction(a[axis]) - Fraction(n[m1] * (P[m1] - a[m1]) + n[m2] * (P[m2] - a[m2]), n[axis])
    out = np.array(p, dtype=np.float64)
    out[axis] = float(x * Fraction(2) ** e)
    return out


def _step_ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def plane_ladder(v, f, stride, seed=29):
    """(points, meta) with meta: `owner` (the laddered face), `owners` (the faces the query may lie on: the owner, for an
    edge rung the face across that edge too, for a corner rung every face at that corner), `kind` (0 interior, 1 edge
    midpoint, 2 corner), `rung` (index into the offsets: 0 first, then the ulp steps, then the powers), `h` (the realised
    offset along the dominant axis times |n_axis| / |n|: the distance from the snapped base's plane position) and `size`
    (the face's longest edge)."""
    rng = np.random.default_rng(seed)
    at_vertex = {}
    for i, t in enumerate(f):
        for k in t:
            at_vertex.setdefault(int(k), []).append(i)
    pts, owner, owners, kind, hs, sizes, rungs = [], [], [], [], [], [], []
    for count, i in enumerate(range(0, f.shape[0], stride)):
        ia, ib, ic = (int(k) for k in f[i])
        a, b, c = v[ia], v[ib], v[ic]
        n = np.cross(b - a, c - a)
        axis = int(np.argmax(np.abs(n)))
        slope = abs(n[axis]) / np.linalg.norm(n)
        size = max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
        r = rng.dirichlet((1.0, 1.0, 1.0))
        bases = [(0, w[0] * a + w[1] * b + w[2] * c, [i]) for w in ((0.5, 0.25, 0.25), (0.125, 0.25, 0.625), r)]
        for (x, y), (kx, ky) in (((a, b), (ia, ib)), ((b, c), (ib, ic)), ((c, a), (ic, ia)))[:3 * (1 - count % 2)]:
            across = [j for j in at_vertex[kx] if j != i and j in at_vertex[ky]]
            bases.append((1, 0.5 * (x + y), [i] + across))
        for x, kx in ((a, ia), (b, ib), (c, ic))[:3 * (1 - count % 2)]:
            bases.append((2, x.copy(), [i] + [j for j in at_vertex[kx] if j != i]))
        for k, base, own in bases:
            base = _snap_to_plane(base, a, b, c, axis)
            offsets = [("ulp", s) for s in ULP_STEPS]
            offsets += [("pow", sg * size * 2.0 ** -e) for e in POWER_STEPS for sg in (1.0, -1.0)]
            for j, (how, s) in enumerate(offsets):
                p = base.copy()
                p[axis] = _step_ulps(base[axis], s) if how == "ulp" else base[axis] + s
                pts.append(p)
                owner.append(i)
                owners.append(own)
                kind.append(k)
                rungs.append(j)
                hs.append((p[axis] - base[axis]) * slope)
                sizes.append(size)
    meta = {"owner": np.array(owner), "owners": owners, "kind": np.array(kind), "rung": np.array(rungs), "h": np.array(hs),
            "size": np.array(sizes)}
    return np.array(pts), meta


LADDERS = {"ladder_sphere": ("sphere512", 16, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
           "ladder_tube": ("tube", 18, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
           "ladder_translated": ("sphere512", 16, (1.0, 1.0, 1.0), TRANSLATION),
           "ladder_flat": ("sphere512", 16, (1.0, 1.0, 2.0 ** -20), (0.0, 0.0, 0.0)),
           "ladder_needle": ("sphere512", 16, (1.0, 2.0 ** -12, 2.0 ** -24), (0.0, 0.0, 0.0))}


# ---- the wrong-sign grid ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wrong_sign_grid():
    """dict: `vertices` (72, 3) and `faces` (24, 3), the merged mesh; `points` (75 000, 3); `owner` the face of every
    query; and, per query against its owner, the f64 `num`, `den`, `L` of the rule and the exact `sign`, `over`,
    `log2_ratio` (owner_classes).  `wrong`: the f64 sign of num differs from the exact sign, f64 zero with exact nonzero
    included."""
    rng = np.random.default_rng(20261021)
    anchor = np.array([0.5, 0.5, 0.5])
    verts, pts, owner = [], [], []
    for i in range(GRID_FACES):
        while True:
            tri = rng.uniform(-20.0, 20.0, size=(3, 3))
            w = rng.dirichlet((2.0, 2.0, 2.0))
            tri = tri + (anchor - w @ tri)                            # an interior point moved to the anchor
            n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            if w.min() > 0.1 and np.abs(n).max() > 50.0 and np.abs(tri).max() > 10.0:
                break
        axis = int(np.argmax(np.abs(n)))
        m1, m2 = (axis + 1) % 3, (axis + 2) % 3
        for s in range(-GRID_HALF, GRID_HALF + 1):
            for t in range(-GRID_HALF, GRID_HALF + 1):
                p = anchor.copy()
                p[m1], p[m2] = _step_ulps(anchor[m1], s), _step_ulps(anchor[m2], t)
                p = _snap_to_plane(p, tri[0], tri[1], tri[2], axis)
                for k in GRID_ULPS:
                    x = p.copy()
                    x[axis] = _step_ulps(p[axis], k)
                    pts.append(x)
                    owner.append(i)
        verts.append(tri)
    v = np.vstack(verts)
    f = np.arange(3 * GRID_FACES, dtype=np.int64).reshape(-1, 3)
    points, owner = np.array(pts), np.array(owner)
    num, den, L = rule_terms(points, v[f[owner, 0]], v[f[owner, 1]], v[f[owner, 2]])
    c = owner_classes(points, v, f, [[int(o)] for o in owner])
    wrong = (np.sign(num).astype(np.int8) != c["sign"]) & (c["sign"] != 0)
    # the family is only worth its time while the f64 sign of num really fails on it
    assert int(wrong.sum()) >= 1000, int(wrong.sum())
    return {"vertices": v, "faces": f, "points": points, "owner": owner, "num": num, "den": den, "L": L, "wrong": wrong,
            "sign": c["sign"], "over": c["over"], "log2_ratio": c["log2_ratio"], "cls": c["cls"]}


def wrong_sign_single(i):
    """face i of the grid alone, with its own 3 125 queries: (points, vertices, faces, selection into the merged arrays)"""
    g = wrong_sign_grid()
    sel = np.flatnonzero(g["owner"] == i)
    return g["points"][sel], g["vertices"][3 * i:3 * i + 3].copy(), np.array([[0, 1, 2]], dtype=np.int64), sel


# ---- lattices and covers ----------------------------------------------------------------------------------------------

BOX_LO, BOX_HI = (-1.0, -2.0, -1.0), (2.0, 1.0, 3.0)
NEST_INNER, NEST_OUTER = ((-0.625,) * 3, (0.625,) * 3), ((-1.125,) * 3, (1.125,) * 3)


def _half_grid(lo, hi):
    ax = np.arange(2 * lo, 2 * hi + 1) / 2.0
    return np.array([(x, y, z) for x in ax for y in ax for z in ax])


def box_side(q, lo, hi):
    """by coordinate comparison: 1 strictly inside the box, 0 strictly outside, -1 on its surface"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    inside = ((q > lo) & (q < hi)).all(axis=1)
    closed = ((q >= lo) & (q <= hi)).all(axis=1)
    return np.where(inside, 1, np.where(closed, -1, 0))


def octahedron_side(q):
    s = np.abs(q).sum(axis=1)                                         # exact on the half-integer grid
    return np.where(s < 3.0, 1, np.where(s == 3.0, -1, 0))


# Faces seen from the origin whose corners have integer coordinates and integer distances, so that den and num are
# integers, on each boundary between two cases of `cone`: (a, b, c), num, den, and the (turns, sign of pi / pr) the rule's
# table gives a single such face: the first case that holds.
CONE_TIES = ((((-9, -6, -2), (-8, -1, 4), (6, 3, -2)), 78, -78, (1, 1)),          # im = -re, im > 0: 135 degrees = 1 turn + 45
             (((-9, -6, -2), (-6, -9, 2), (4, 3, 0)), -30, -30, (-1, -1)),        # im = re, im < 0: -135 = -1 turn - 45
             (((-9, -6, -2), (-9, 0, 0), (2, 2, -1)), 90, 90, (0, 1)),            # im = re, im > 0: 45 stays
             (((-9, -6, -2), (-9, 0, 0), (2, 1, 2)), -90, 90, (0, -1)),           # im = -re, im < 0: -45 stays
             (((-9, -6, -2), (-9, 6, 2), (9, -2, -6)), 576, 0, (1, 0)),           # re = 0, im > 0: 90 = 1 turn
             (((-9, -6, -2), (-9, 6, 2), (9, -6, 2)), -432, 0, (-1, 0)))          # re = 0, im < 0: -90 = -1 turn


def cone_tie(i):
    """tie face i alone, seen from the origin and from (1, 0.5, 0.25): (points, vertices, faces)"""
    v = np.array(CONE_TIES[i][0], dtype=np.float64)
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]]), v, np.array([[0, 1, 2]], dtype=np.int64)


# ---- the cases --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ladder(name):
    mesh, stride, scale, shift = LADDERS[name]
    v, f = getattr(wc, mesh)()
    v = v * np.array(scale) + np.array(shift)
    pts, meta = plane_ladder(v, f, stride)
    return pts, v, f, meta


@functools.lru_cache(maxsize=None)
def get(name):
    """(points, vertices, faces)"""
    if name in LADDERS:
        return _ladder(name)[:3]
    if name.startswith("scaled_"):
        q, v, f = get("ladder_sphere")
        s = 2.0 ** int(name[7:])
        return q * s, v * s, f
    if name == "wrong_sign_merged":
        g = wrong_sign_grid()
        return g["points"], g["vertices"], g["faces"]
    if name.startswith("wrong_sign_"):
        return wrong_sign_single(int(name[11:]))[:3]
    if name == "lattice_box":
        return (_half_grid(-3, 4),) + wc.box(BOX_LO, BOX_HI)
    if name == "lattice_box_inward":
        v, f = wc.box(BOX_LO, BOX_HI)
        return _half_grid(-3, 4), v, f[:, ::-1].copy()
    if name == "lattice_octahedron":
        return (_half_grid(-4, 4),) + wc.octahedron()
    if name == "cone_ties":                                           # all six in one mesh: one call for the device
        v = np.vstack([np.array(t[0], dtype=np.float64) for t in CONE_TIES])
        return cone_tie(0)[0], v, np.arange(v.shape[0], dtype=np.int64).reshape(-1, 3)
    if name.startswith("cone_tie_"):
        return cone_tie(int(name[9:]))
    if name == "limit_box":
        big = 2.0 ** 300                                              # the largest coordinates the entry points accept
        q = np.array([[0, 0, 0], [0.5, -0.25, 0.125], [1, 1, 1], [1, 0.5, 0], [-1, 0, 0.25], [0.5, 0.5, -0.75]]) * big
        return (q,) + wc.box((-big,) * 3, (big,) * 3)
    rng = np.random.default_rng(20261022)
    if name == "cover_five":
        v, f = wc.sphere512()
        return rng.uniform(-1.5, 1.5, size=(200, 3)), v, np.vstack([f] * 5)
    if name == "cover_cancel":
        v, f = wc.sphere512()
        return rng.uniform(-1.5, 1.5, size=(200, 3)), v, np.vstack([f, f[:, ::-1]])
    if name == "cover_nested":
        (vi, fi), (vo, fo) = wc.box(*NEST_INNER), wc.box(*NEST_OUTER)
        return rng.integers(-6, 7, size=(200, 3)) / 4.0, np.vstack([vi, vo]), np.vstack([fi, fo + 8])
    raise KeyError(name)


LADDER_CASES = tuple(LADDERS)
SCALED_CASES = tuple(f"scaled_{k}" for k in SCALES)
LATTICE_CASES = ("lattice_box", "lattice_box_inward", "lattice_octahedron")
COVER_CASES = ("cover_five", "cover_cancel", "cover_nested")
SINGLE_CASES = tuple(f"wrong_sign_{i}" for i in range(GRID_FACES))
DEVICE_CASES = LADDER_CASES + ("wrong_sign_merged",) + LATTICE_CASES + COVER_CASES + SCALED_CASES + ("limit_box", "cone_ties")
TIE_CASES = tuple(f"cone_tie_{i}" for i in range(len(CONE_TIES)))
HOST_CASES = DEVICE_CASES + SINGLE_CASES + TIE_CASES


@functools.lru_cache(maxsize=None)
def expected(name):
    """the checker's full result for a case"""
    q, v, f = get(name)
    return chk.winding(q, v, f, wc.plan)


@functools.lru_cache(maxsize=None)
def expected_reference(name):
    """chk.reference where the checker's err is finite (nothing is asserted about a value elsewhere, and the long-double
    sum is the slowest step of these tests); nan elsewhere"""
    q, v, f = get(name)
    fin = np.isfinite(expected(name)["err"])
    ref = np.full(q.shape[0], np.nan, dtype=np.longdouble)
    if fin.any():
        ref[fin] = chk.reference(q[fin], v, f)
    return ref


@functools.lru_cache(maxsize=None)
def meta(name):
    """What is known about the queries of a case without the rule.  Ladders: plane_ladder's meta plus owner_classes.
    Lattices and covers: `exact` (the winding number by construction; nan on a surface) and `on` (on the surface)."""
    q, v, f = get(name)
    if name in LADDERS:
        m = dict(_ladder(name)[3])
        m.update(owner_classes(q, v, f, m["owners"]))
        return m
    if name.startswith("scaled_"):
        return meta("ladder_sphere")                                  # scaling by a power of two keeps every class
    if name in ("lattice_box", "lattice_box_inward"):
        side = box_side(q, BOX_LO, BOX_HI)
        sgn = -1.0 if name.endswith("inward") else 1.0
    elif name == "lattice_octahedron":
        side, sgn = octahedron_side(q), 1.0
    elif name == "cover_five":
        side, sgn = np.where((q * q).sum(axis=1) < 0.9, 1, np.where((q * q).sum(axis=1) > 1.0, 0, -2)), 5.0
    elif name == "cover_cancel":
        side, sgn = np.zeros(q.shape[0], dtype=np.int64), 0.0
    elif name == "cover_nested":
        side = box_side(q, *NEST_OUTER) + box_side(q, *NEST_INNER)
        assert (box_side(q, *NEST_OUTER) >= 0).all() and (box_side(q, *NEST_INNER) >= 0).all()
        sgn = 1.0
    else:
        raise KeyError(name)
    exact = np.where(side < 0, np.nan, sgn * np.maximum(side, 0))
    return {"exact": exact, "on": side == -1, "between": side == -2}


def exact_surface_by_oracle(name):
    """the lattice queries that the exact oracle finds ON a face of the solid: every query against every face"""
    q, v, f = get(name)
    every = list(range(f.shape[0]))
    return owner_classes(q, v, f, [every] * q.shape[0])["on"]


# ---- the proofs, for any result: the checker's, the host hook's or the device's (a dict of arrays) ---------------------

def truth(name):
    """(value to compare w with, where it may be compared): exact by construction, or the trusted long-double reference"""
    m = meta(name)
    if "exact" in m:
        return m["exact"], ~np.isnan(m["exact"])
    return expected_reference(name).astype(np.float64), m["trusted"]


def _gap(w, ref):
    with np.errstate(invalid="ignore"):
        return np.abs(w - ref)


def check_err_and_decisions(name, r, two_sided=False):
    """`err` holds and no decided query is wrong, for a result r (the checker's, the host's or the device's)"""
    ref, known = truth(name)
    inside = chk.classify(r["w"], r["err"], two_sided=two_sided) if two_sided else r["inside"]
    ok = np.isfinite(r["err"]) & known
    gap = _gap(r["w"], ref)
    tight = (gap[ok] / r["err"][ok]).max() if ok.any() else None
    print(name, "queries", r["w"].shape[0], "finite and comparable", int(ok.sum()), "largest |w - ref| / err", tight)
    assert (gap[ok] <= r["err"][ok]).all()
    x = np.abs(ref) if two_sided else ref
    assert (x[known & (inside == 1)] > 0.5).all() and (x[known & (inside == 0)] < 0.5).all()
    return tight


def check_nothing_on_a_face_is_decided(name, r):
    on = meta(name)["on"]
    assert on.any()
    assert np.isinf(r["err"][on]).all() and (r["inside"][on] == -1).all()
    return int(on.sum())


def check_no_wrong_sign_is_decided(err, sel=slice(None)):
    g = wrong_sign_grid()
    attacked = (g["wrong"] & g["over"])[sel]
    assert np.isinf(err[attacked]).all()
    return int(attacked.sum())
