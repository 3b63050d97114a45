"""What tests/test_clip_exact_host.py and tests/test_gpu_clip_exact.py share: the case table of the exact clip tests, the
checker's result of every case (computed once), and ``judge``, which sends a result and its complement through X1-X9 of
tests/clip_exact.py as they apply, printing every figure before it asserts.

The cases are the smallest that reach their path: lattice solids (exact heights, so the oracle's sides are the rule's), a
plane through rows of vertices, complement pairs, K = 2 with one failing cut, ten cuts, a mesh whose every face is cut,
cut faces on the boundaries of the scans and the waves, and two families of rounding worst cases found by a seeded
search at import."""
import functools
import types
from fractions import Fraction as F

import numpy as np

import clip_cases as CC
import clip_exact as E
from mm_checkers import mesh_clip as Y
from test_section_exact_host import icosahedron, lattice_torus
from test_section_host import join, tube

import multimoda_rs_amd as mm

KEEP, SCOPE = mm.clip.KEEP, mm.clip.SCOPE


class Case:
    def __init__(self, v, f, o, n, keep, scope, cap=True, ext=None, lattice=False, closed=True, outward=0, x8=True):
        K = len(o)
        self.v, self.f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
        self.o, self.n = np.array(o, dtype=np.float64).reshape(-1, 3), np.array(n, dtype=np.float64).reshape(-1, 3)
        self.keep = [keep] * K if isinstance(keep, str) else list(keep)
        self.scope = [scope] * K if isinstance(scope, str) else list(scope)
        self.cap, self.ext = cap, ext
        self.lattice, self.closed, self.outward, self.x8 = lattice, closed, outward, x8

    def args(self, flip=False):
        other = {"below": "above", "above": "below"}
        keep = [other[k] for k in self.keep] if flip else self.keep
        return (self.v, self.f, self.o, self.n, keep, self.scope, self.cap, self.ext)

    def problem(self, flip=False):
        p = _problem(self)
        return p.flipped() if flip else p


@functools.lru_cache(maxsize=None)
def _problem(case):
    return E.Problem(case.v, case.f, case.o, case.n, CC.codes(case.keep, KEEP, len(case.o)), CC.codes(case.scope, SCOPE, len(case.o)),
                     case.cap, case.ext)


# ---- the meshes -----------------------------------------------------------------------------------------------------------

def tie_prism():
    """a square (corners (+-1, +-1, 0)) under a diamond (corners on the axes at z = 2): eight isosceles side faces, four
    apex up and four apex down; under the plane z = 1 every one has two diagonals of exactly equal length (3.25 = 3.25
    for the first kind, 2.25 = 2.25 for the second).  Outward."""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0, -1, 2], [1, 0, 2], [0, 1, 2], [-1, 0, 2]], dtype=float)
    f = []
    for i in range(4):
        j = (i + 1) % 4
        f += [(i, j, 4 + i), (j, 4 + j, 4 + i)]
    f += [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7)]
    f = np.array(f, dtype=np.int64)
    centre = v.mean(axis=0)
    for t in f:                                                          # convex: every face looks away from the centre
        a, b, c = v[t]
        assert np.dot(np.cross(b - a, c - a), a - centre) > 0
    return v, f


def _lattice_cases(c):
    vt, ft = (lambda t: (t.v, t.f))(lattice_torus())
    vi, fi = icosahedron()
    vp, fp = tie_prism()
    solids = {
        # the tube of the torus cut twice where it passes x = +-2: the half y < 1/8 stays
        "torus2": (vt, ft, [[2.0, 0.125, 0.0], [-2.0, 0.125, 0.0]], [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], ["below", "above"], "loop"),
        "icosa": (vi, fi, [[0.125, 0.0, 0.125]], [[1.0, 0.25, 0.5]], "below", "plane"),
        "tie_prism": (vp, fp, [[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], "above", "plane"),
    }
    for name, (v, f, o, n, keep, scope) in solids.items():
        for orient, faces in (("out", f), ("in", f[:, ::-1].copy())):
            for ext in (None, (1.0, 1), (0.75, 2), (1.25, 5)):
                c[f"{name}_{orient}_L{ext[1] if ext else 0}"] = Case(v, faces, o, n, keep, scope, True, ext, lattice=True,
                                                                    outward=1 if orient == "out" else -1)
    # a plane through two rows of vertices of the torus (z = r sin(3 pi / 8), snapped): edges on the plane, apexes on it
    z = sorted(set(vt[:16, 2].tolist()))[-2]
    c["torus_rows"] = Case(vt, ft, [[0.0, 0.0, z]], [[0.0, 0.0, 1.0]], "above", "plane", True, None, lattice=True, outward=1)


def ten_cut_mesh():
    """a closed tube from x = 0 to 12 and, beyond either end, a small closed tube of its own"""
    shift = lambda m, x: (m[0] + [x, 0.0, 0.0], m[1])                     # noqa: E731
    body = tube(8, 49, 1.0, 0.25, caps=True, jitter=0.01, seed=21)
    left = shift(tube(6, 3, 0.5, 0.25, caps=True, jitter=0.01, seed=22), -3.0)
    right = shift(tube(6, 3, 0.5, 0.25, caps=True, jitter=0.01, seed=23), 15.0)
    return join(body, left, right)


def _other_cases(c):
    for name in ("tube_both_ends", "torus_two_cuts"):
        v, f, o, n, keep, scope, cap, ext = CC.CASES[name]
        c[name] = Case(v, f, o, n, keep, scope, cap, ext, outward=1)
    v, f, o, n = CC.CASES["tube_both_ends"][:4]
    c["tube_capped"] = Case(v, f, o, n, ["above", "below"], "loop", True, None, outward=1)
    # K = 2, one cut fails: the torus stays in one piece, the tube does not
    vt, ft = CC.torus(24, 10, jitter=0.01, seed=2)
    vu, fu = tube(8, 10, 1.0, 0.5, jitter=0.01, seed=14)
    v, f = join((vt, ft), (vu + [20.0, 0.0, 0.0], fu))
    cuts = [([3.0, 0.1, 0.0], [0.05, 1.0, 0.0]), ([22.2, 0.0, 0.0], [1.0, 0.02, 0.0])]
    for name, order in (("k2_fail_first", (0, 1)), ("k2_fail_second", (1, 0))):
        c[name] = Case(v, f, [cuts[i][0] for i in order], [cuts[i][1] for i in order], "below", "loop", True, None, closed=False, x8=False)
    # ten cuts: 8 LOOP cuts leave the segments S1, S3, S5, S7 of the tube; 2 PLANE cuts, far apart, trim the small
    # tubes beyond its ends off the mesh.  The stations are 1.25 apart on rings 0.25 apart: no face is in two cut sets.
    # (A PLANE cut through S0 or S8 would have its kept side dropped by the LOOP cut next to it: C2's orphan rule.)
    xs = [1.1 + 1.25 * i for i in range(8)]
    o = [[x, 0.0, 0.0] for x in xs] + [[-1.0, 0.0, 0.0], [13.5, 0.0, 0.0]]
    n = [[1.0, 0.02 * (-1) ** i, 0.01] for i in range(8)] + [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    c["ten_cuts"] = Case(*ten_cut_mesh(), o, n, ["above", "below"] * 4 + ["above", "below"], ["loop"] * 8 + ["plane"] * 2, True, None,
                         outward=1, x8=False)
    # every face is cut: two rings, a plane between them
    c["every_face_cut"] = Case(*tube(12, 2, 1.0, 1.0, jitter=0.01, seed=15), [[0.5, 0.0, 0.0]], [[1.0, 0.03, 0.02]], "below", "plane",
                               True, None, closed=False, outward=1)


# ---- the orphan rule: a cut whose kept side another cut drops ----------------------------------------------------------------

def _orphan_cases(c):
    v, f = tube(8, 30, 1.0, 0.25, jitter=0.01, seed=3)
    length = 29 * 0.25
    o = [[0.3 * length, 0.0, 0.0], [0.7 * length, 0.0, 0.0]]
    n = [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    c["orphan_below_below"] = Case(v, f, o, n, "below", "loop", True, None, closed=False, x8=False)
    c["orphan_above_above"] = Case(v, f, o, n, "above", "loop", True, None, closed=False, x8=False)
    c["orphan_loop_plane"] = Case(v, f, o, n, "below", ["plane", "loop"], True, None, closed=False, x8=False)
    c["orphan_plane_loop"] = Case(v, f, o, n, "above", ["loop", "plane"], True, None, closed=False, x8=False)


ORPHAN_STATUS = {"orphan_below_below": [Y.OK, Y.KEPT_SIDE_DROPPED], "orphan_above_above": [Y.KEPT_SIDE_DROPPED, Y.OK],
                 "orphan_loop_plane": [Y.OK, Y.KEPT_SIDE_DROPPED], "orphan_plane_loop": [Y.KEPT_SIDE_DROPPED, Y.OK]}


# ---- cut faces on the boundaries of the scans and the waves -------------------------------------------------------------------

BOUNDARY_AT = (15, 16, 63, 64, 255, 256, 4095, 4096)


@functools.lru_cache(maxsize=None)
def boundary_base():
    """scan_tiles' mesh padded with far-away untouched triangles to nf = 8193 = 2 * 4096 + 1, and per cut face the pieces
    its cuts leave (1: apex kept, 2: apex dropped), from the checker's result of the padded mesh"""
    v, f, o, n, keep, scope, cap, ext = CC.CASES["scan_tiles"]
    pad = 8193 - len(f)
    far = np.array([[1e3 + i, 1e3 + (j == 1), 1e3 + (j == 2)] for i in range(pad) for j in range(3)], dtype=np.float64)
    f = np.concatenate([f, len(v) + np.arange(3 * pad, dtype=np.int64).reshape(-1, 3)])
    v = np.concatenate([v, far])
    assert len(f) % 4096 == 1
    case = Case(v, f, o, n, keep, scope, cap, ext, closed=False, x8=False)
    want = checked_of(case)
    parents = want.face_origin[want.face_kind == Y.PIECE]
    left = {int(p): int(c) for p, c in zip(*np.unique(parents, return_counts=True))}
    return case, left


def boundary_faces(first_kind):
    """the padded case with its faces permuted: cut faces that leave 1 and 2 pieces, alternating from ``first_kind``, at
    BOUNDARY_AT and at nf - 1; and the permutation (new face -> face of the base)"""
    case, left = boundary_base()
    nf = len(case.f)
    by_kind = {k: [p for p, c in sorted(left.items()) if c == k] for k in (1, 2)}
    perm = np.arange(nf)
    where = np.arange(nf)                                                # base face -> its place
    targets = list(BOUNDARY_AT) + [nf - 1]
    assert min(len(by_kind[1]), len(by_kind[2])) >= len(targets)
    placed = {}
    for i, t in enumerate(targets):
        kind = first_kind if i % 2 == 0 else 3 - first_kind
        face = by_kind[kind].pop()
        a, b = where[face], t
        perm[a], perm[b] = perm[b], perm[a]
        where[perm[a]], where[perm[b]] = a, b
        placed[t] = kind
    assert all(left[int(perm[t])] == k for t, k in placed.items())
    return Case(case.v, case.f[perm], case.o, case.n, case.keep, case.scope, case.cap, case.ext, closed=False, x8=False), perm


def boundary_vertices():
    """the padded case with its vertices renamed so that kept and dropped vertices alternate over the indices 4088 ..
    4103, across the boundary 4095 / 4096 of the keep-flag scan; and the renaming (new vertex -> vertex of the base)"""
    case, _left = boundary_base()
    want = checked_of(case)
    nv = len(case.v)
    kept = np.zeros(nv, dtype=bool)
    kept[want.vertex_origin[want.vertex_origin >= 0]] = True
    pools = {True: [int(i) for i in np.nonzero(kept)[0] if i < 4000], False: [int(i) for i in np.nonzero(~kept)[0] if i < 4000]}
    perm = np.arange(nv)
    where = np.arange(nv)
    for t in range(4088, 4104):
        x = pools[t % 2 == 0].pop()
        a, b = where[x], t
        perm[a], perm[b] = perm[b], perm[a]
        where[perm[a]], where[perm[b]] = a, b
    assert [bool(kept[perm[t]]) for t in range(4088, 4104)] == [t % 2 == 0 for t in range(4088, 4104)]
    inverse = np.empty(nv, dtype=np.int64)
    inverse[perm] = np.arange(nv)
    return Case(case.v[perm], inverse[case.f], case.o, case.n, case.keep, case.scope, case.cap, case.ext, closed=False, x8=False), perm


def as_sets(res, vertex_map=None, face_map=None, decimals=None):
    """a result as sets that do not depend on the order of the input: vertices (origin, bits) and faces (origin, kind, the
    corners named by origin or, for a new vertex, by their bits -- rotated to start at the smallest name).  A crossing
    point is computed from the lower vertex index to the higher (rule 3), so renaming the vertices moves it by a
    rounding: with ``decimals`` new vertices are named and compared by their coordinates rounded to that."""
    vo = res.vertex_origin.tolist()
    bits = lambda i, o: (res.vertices[i] if decimals is None or o >= 0 else np.round(res.vertices[i], decimals) + 0.0).tobytes()   # noqa: E731
    name = [("v", int(vertex_map[o]) if vertex_map is not None else o) if o >= 0 else ("m", o, bits(i, o)) for i, o in enumerate(vo)]
    faces = []
    for t, o, k in zip(res.faces.tolist(), res.face_origin.tolist(), res.face_kind.tolist()):
        q = [name[i] for i in t]
        r = min(range(3), key=lambda j: q[j])
        origin = int(face_map[o]) if (face_map is not None and o >= 0) else o
        faces.append((origin, k, q[r], q[(r + 1) % 3], q[(r + 2) % 3]))
    return sorted((n, bits(i, vo[i])) for i, n in enumerate(name)), sorted(faces)


# ---- rounding worst cases -------------------------------------------------------------------------------------------------------

ZERO_NX = 0.1


@functools.lru_cache(maxsize=None)
def zero_heights():
    """An open tube along y of three rings of 32, under the PLANE cut o = 0, n = (nx, -1, 0).  The middle ring sits at
    y = fl(nx * x): the rule's unfused height fl(fl(nx * x) - y) is exactly zero (above) while the exact height
    nx * x - y is the rounding error of the product, of either sign.  A contracted multiply-add returns that error
    instead of zero.  Returns the case and the indices of the middle ring."""
    rng = np.random.default_rng(31)
    m = 32
    ang = 2.0 * np.pi * (np.arange(m) + rng.uniform(-0.2, 0.2, m)) / m
    rings = []
    for y in (1.0, None, -1.0):                                          # above the plane is y < nx x: ring 2
        x, z = np.cos(ang) * (1.0 + rng.uniform(-0.01, 0.01, m)), np.sin(ang) * (1.0 + rng.uniform(-0.01, 0.01, m))
        rings.append(np.stack([x, np.array([ZERO_NX * float(a) for a in x]) if y is None else np.full(m, y), z], 1))
    v = np.concatenate(rings)
    f = []
    for i in range(2):
        for j in range(m):
            a, b = i * m + j, i * m + (j + 1) % m
            f += [(a, b, b + m), (a, b + m, a + m)]
    case = Case(v, np.array(f, dtype=np.int64), [[0.0, 0.0, 0.0]], [[ZERO_NX, -1.0, 0.0]], "above", "plane", True, None, closed=False)
    return case, list(range(m, 2 * m))


def zero_height_facts(case, ring):
    """(vertices of the ring whose unfused height is +-0.0, those of them whose exact height is negative, positive)"""
    nx = case.n[0, 0]
    zero = neg = pos = 0
    for i in ring:
        x, y, z = case.v[i].tolist()
        h = (nx * (x - 0.0) + (-1.0) * (y - 0.0)) + 0.0 * (z - 0.0)
        exact = F(nx) * F(x) - F(y)
        zero += h == 0.0
        neg += h == 0.0 and exact < 0
        pos += h == 0.0 and exact > 0
    return zero, neg, pos


def _d2(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def _d2_contracted(p, q):
    """the same sum with each multiply-add contracted: fma(dz, dz, fma(dy, dy, dx * dx)), one rounding per fma"""
    dx, dy, dz = (F(a) - F(b) for a, b in zip(p, q))
    dx, dy, dz = F(float(dx)), F(float(dy)), F(float(dz))
    s = F(float(dx * dx))
    s = F(float(dy * dy + s))
    return float(dz * dz + s)


@functools.lru_cache(maxsize=None)
def near_ties(wanted=24, wanted_flips=6, seed=37):
    """Separate triangles a = (., ., 2), b = (., ., 0), c = (., ., 0) under the plane z = 1: t = 1/2, so the loop points
    are the midpoints of a-b and a-c.  x and y lie in (-1, 1) on a grid of 2^-40, but for c.x, which a seeded search
    then moves on the grid of 2^-52 to where the exact squared diagonals |m_ab - c|^2 and |b - m_ca|^2 differ, but by
    less than one rounding of the three-term sum (eps * d2).  The midpoints stay exactly representable, so the exact
    diagonals are known before anything runs.  The first ``wanted_flips`` faces are such that a contracted sum,
    fma(dz, dz, fma(dy, dy, dx * dx)), decides the other way than the rule's unfused one.  Returns the case and the two
    counts."""
    rng = np.random.default_rng(seed)
    tris, flips = [], 0
    g, u = 2.0 ** -40, 2.0 ** -52
    ex = lambda p, q: sum((F(x) - F(y)) ** 2 for x, y in zip(p, q))          # noqa: E731
    mid = lambda p, q: tuple(p[d] + 0.5 * (q[d] - p[d]) for d in range(3))   # noqa: E731
    for _trial in range(20000):
        if len(tris) == wanted:
            break
        r = [float(x) * g for x in np.round(rng.uniform(-0.25, 0.25, 5) / g)]
        a, b = (r[0], r[1], 2.0), (-0.75 + r[2], r[3], 0.0)
        cx = 0.75
        diff = lambda x: _d2(mid(a, b), (x, r[4], 0.0)) - _d2(b, mid(a, (x, r[4], 0.0)))   # noqa: E731
        for _newton in range(8):                                         # near the root of the difference, in floats
            cx -= diff(cx) / ((diff(cx + 2.0 ** -20) - diff(cx)) / 2.0 ** -20)
        best = None
        for k in range(-4, 5):
            c = (round(cx / u) * u + k * u, r[4], 0.0)
            m_ab, m_ca = mid(a, b), mid(a, c)
            if not 0.5 < c[0] < 1.0 or any(F(m_ab[d]) != (F(a[d]) + F(b[d])) / 2 or F(m_ca[d]) != (F(a[d]) + F(c[d])) / 2 for d in range(3)):
                continue
            d_c, d_b = ex(m_ab, c), ex(b, m_ca)
            if d_c == d_b or abs(d_c - d_b) >= F(u) * d_c:
                continue
            flip = (_d2(m_ab, c) < _d2(b, m_ca)) != (_d2_contracted(m_ab, c) < _d2_contracted(b, m_ca))
            if best is None or flip > best[0]:
                best = (flip, c)
        if best is None or (flips < wanted_flips and not best[0]):
            continue
        flips += best[0]
        tris.append((a, b, best[1]))
    v = np.array([p for t in tris for p in t], dtype=np.float64)
    f = np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)
    case = Case(v, f, [[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]], "below", "plane", False, None, closed=False)
    return case, len(tris), flips


# ---- the table, the checker's results, the comparison --------------------------------------------------------------------------

def _cases():
    c = {}
    _lattice_cases(c)
    _other_cases(c)
    _orphan_cases(c)
    return c


CASES = _cases()
LATTICE = [n for n, c in CASES.items() if c.lattice]
PAIRS = [n for n, c in CASES.items() if c.x8]
NOT_APPLIED = ("k2_fail_first", "k2_fail_second") + tuple(ORPHAN_STATUS)


def as_result(want, K):
    """the checker's dict as an object with the fields of a ClippedMesh that the oracle reads"""
    rims, r = [[] for _ in range(K)], 0
    if want["applied"]:
        for k in range(K):
            for _ in range(int(want["cut_status"][k, 2])):
                rims[k].append(want["rim_index"][int(want["rim_off"][r]):int(want["rim_off"][r + 1])].copy())
                r += 1
    st = want["cut_status"]
    return types.SimpleNamespace(vertices=want["vertices"], faces=want["faces"], vertex_origin=want["vertex_origin"],
                                 face_origin=want["face_origin"], face_kind=want["face_kind"], rims=rims, cut_status=st[:, 0].copy(),
                                 cut_points=st[:, 1].copy(), cut_loops=st[:, 2].copy(), cut_faces=st[:, 3].copy(),
                                 applied=bool(want["applied"]), report=dict(want["counts"]))


_CHECKED = {}


def checked_dict(case, flip=False):
    key = (id(case), flip)
    if key not in _CHECKED:
        _CHECKED[key] = (case, CC.check(*case.args(flip)))               # the case is kept alive with its result
    return _CHECKED[key][1]


def checked_of(case, flip=False):
    return as_result(checked_dict(case, flip), len(case.o))


def run(case, fn, flip=False, **kw):
    """the case (or its complement) through ``fn``, equal to the checker bit for bit"""
    v, f, o, n, keep, scope, cap, ext = case.args(flip)
    got = fn((v, f), o, n, keep=keep, scope=scope, cap=cap, extension=ext, **kw)
    return CC.same_as_checker(got, checked_dict(case, flip))


def show(name, what, found):
    print(name, what, {k: x for k, x in found.items() if k not in ("bad", "used")}, "bad:", found["bad"][:3])
    return found


def judge(name, res, other=None, planar=None):
    """X1-X9 as they apply to the case: ``res`` the run, ``other`` the run with every keep flipped (the cases in PAIRS).
    Returns the figures."""
    case = CASES[name] if isinstance(name, str) else name
    p = case.problem()
    w = E.View(res)
    out = {}
    assert res.applied, res.cut_status
    out["x9"] = show(name, "X9", E.x9_order(p, w))
    out["x5"] = show(name, "X5", E.x5_rims(p, w))
    if case.cap:
        out["x6"] = show(name, "X6", E.x6_caps(p, w, case.outward))
    if case.ext:
        out["x7"] = show(name, "X7", E.x7_extension(p, w))
    if case.closed and case.cap:
        out["x4"] = show(name, "X4", E.x4_whole(w))
    if other is not None:
        w2 = E.View(other)
        cuts = E.cut_sets(w, w2)
        assert len(cuts) == sum(int(x) for x in res.cut_faces)
        out["x2"] = show(name, "X2", E.x2_pieces(p, w, w2, cuts, planar=case.lattice if planar is None else planar))
        out["x8"] = show(name, "X8", E.x8_complement(p, w, w2, cuts, closed=case.closed))
        if case.lattice:
            assert E.heights_are_exact(p)
            out["x1"] = show(name, "X1", E.x1_sides(p, w, cuts))
            out["x1_other"] = show(name, "X1 (complement)", E.x1_sides(p.flipped(), w2, cuts))
            out["x3"] = show(name, "X3", E.x3_diagonals(p, w, w2, cuts))
            assert out["x1"]["n_checked"] == len(case.v) == out["x1_other"]["n_checked"]
            if case.closed and case.cap and not case.ext:
                assert E.exact_loop_points(p, w, cuts) == E.exact_loop_points(p, w2, cuts)
                if E.exact_loop_points(p, w, cuts) and E.exact_loop_points(p, w2, cuts):
                    assert out["x8"]["volume_exact"], out["x8"]
                    out["x8"]["asserted_exact"] = True
    for key, found in out.items():
        assert not found["bad"], (name, key, found["bad"][:5])
    return out


def closed_pieces(res):
    """the connected pieces of a result, each judged by X4"""
    w = E.View(res)
    return [E.x4_manifold(w.V, faces) for faces in E.components(w.faces)]
