"""An exact oracle for mesh clipping: `fractions.Fraction` on the f64 inputs and on the stored f64 coordinates of a result.
It shares nothing with the checker (tests/mm_checkers/mesh_clip.py): it never builds a clipped mesh of its own, it judges
a finished one -- vertices, faces, vertex_origin, face_origin, face_kind, rims, statuses, loop-point counts -- against
the inputs and the text of C1-C8 (include/mm_ccta.h).  Primitives come from tests/section_exact.py.  Every property
returns what it found (a dict with the list ``bad`` of violations and the figures a test prints), so a test can show the
worst case and assert on counts.

X1 sides       On inputs whose f64 heights are exact: every kept old vertex lies on the kept side of every PLANE cut;
               every old corner of a kept piece lies on the kept side of its cut; the dropped vertices are exactly those
               on the drop side of a PLANE cut or connected, through faces in no cut set (a BFS over the input, here), to
               a drop-side corner of a cut face of a LOOP cut.  Every vertex is classified: none is left out.
X2 pieces      Per cut face, the kept pieces of a run and of its complement (every keep flipped) are three; their exact
               vector areas sum to that of the pentagon a, m_ab, b, c, m_ca (true for any stored points: the inner
               edges cancel); with ``planar`` each has a non-negative exact dot product with the parent's vector area.
X3 diagonal    Which diagonal the two quad pieces share, against exact squared lengths of the stored points: the
               strictly shorter one, b - m_ca at an exact tie.  The ties are counted.
X4 manifold    Every directed edge once and its reverse once, every vertex used, the exact vector areas sum to zero.
X5 rims        Every edge of ring 0 of a closed loop of cut k is an edge of exactly one kept piece of cut k; with an
               extension every edge of the outermost ring is an edge of exactly one extension face (and ring 0's too);
               with a cap every edge of the outermost ring is an edge of exactly one cap face.
X6 caps        The cap faces of loop r sum, in exact vector area, to plus or minus the vector area of the polygon
               rims[k][r] (a telescoping identity, whatever the centre; rule 5 lists every loop anticlockwise about n,
               C6 turns the cap after the adjacent pieces, so the sign is the mesh's).  Summed over the loops of a cut
               its dot product with sgn n is positive on an outward input and negative on the same input with its faces
               reversed (per cut: the inner loop of a nested pair rightly looks the other way).
X7 extension   Ring j against ring 0.  C6: q = fl(p + fl(fl(sgn * fl(j * step)) * u)), step = fl(ext_length / L), u =
               fl(n / nn), nn = fl(sqrt(fl(sum of squares))).  With w = 2^-53 = eps / 2 the unit roundoff, relative
               errors to first order: a square w and up to two sums, so the sum of squares 3 w, halved by the root,
               which rounds: nn 2.5 w; the division: u 3.5 w; step w, j * step w more, the product with u w more (sgn
               is exact): the offset t u_k is off by at most 6.5 w |t| <= 3.25 eps ext_length.  The final sum rounds
               by w |q_k| <= 0.5 eps (|p_k| + ext_length).  Per component
               |q_k - (p_k + t n_k / |n|)| <= 3.75 eps ext_length + 0.5 eps |p_k| <= 4.25 eps max(|p|, ext_length),
               asserted as **C7 = 4.5** (4.25 and the second-order terms), t = sgn j ext_length / L exact.
X8 complement  A run and the run with every keep flipped, both applied: kept old vertices disjoint, untouched parents
               disjoint, per cut face the kept pieces disjoint and together C4's three; loop points equal in bits;
               with caps and no extension the cap faces of one are the reversed cap faces of the other.  Volume, on a
               closed input, capped, no extension: V_below + V_above - V_input.  The caps cancel (reversed copies on the
               same vertices) and the untouched faces are shared out, so V_below + V_above is the volume of S', the
               input with every cut face replaced by its three pieces.  With every loop point moved to the nearest
               point of its edge, S' becomes a flat re-triangulation of the input: the same volume.  Moving one vertex
               m of a closed surface by e changes 6 V by e . sum of q x r over its triangles (m, q, r), which is 2 e .
               (the vector area of m's link), and the link of a loop point spans, to first order, no more than the two
               cut faces of its edge.  |e| is at most E1's c1 eps M (DESIGN 4.28, M the largest |coordinate|), every cut
               face has two loop points, so |V_below + V_above - V_input| <= c1 eps M * (2/3) * sum of the cut faces'
               areas; a face's area is inradius * perimeter / 2, and a disc inside the cube [-M, M]^3 has a radius of at
               most sqrt(3/2) M (the hexagonal section), so the area is at most 0.62 perimeter M and the sum at most
               0.41 c1 eps M * perimeter * M per face, which is below what is asserted, the issue's
               **sum over cut faces of c1 eps M * perimeter * M / 2**; the ratio is printed.  Where every loop point is
               the exact crossing (``exact_loop_points``) S' is the flat re-triangulation itself and the test asserts
               equality.
X9 order       C5 and C7 from the result's own maps: kept old vertices first, ascending; new vertices grouped per cut in
               cut order; kinds in blocks 0/1, 2, 3; parents non-decreasing in the first block; cuts non-decreasing in
               the other two.
"""
import math
from collections import deque
from fractions import Fraction as F

import numpy as np

import section_exact as Q

BELOW, ABOVE, LOOP, PLANE = 0, 1, 0, 1
UNTOUCHED, PIECE, EXTENSION, CAP = 0, 1, 2, 3
EPS = F(2) ** -52
C1_E1 = F(9, 2)                       # a loop point is within c1 eps M of its edge
C7 = F(9, 2)


class Problem:
    """the inputs of one clip_mesh call, as floats and as rationals"""

    def __init__(self, v, f, origins, normals, keep, scope, cap=False, extension=None):
        self.v = np.ascontiguousarray(v, dtype=np.float64)
        self.f = [tuple(int(i) for i in t) for t in np.asarray(f).reshape(-1, 3)]
        self.o, self.n = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        self.K = len(self.o)
        self.keep, self.scope, self.cap = [int(x) for x in keep], [int(x) for x in scope], bool(cap)
        self.ext_length, self.L = (float(extension[0]), int(extension[1])) if extension else (0.0, 0)
        self.vF, self.oF, self.nF = Q.fr_rows(self.v), Q.fr_rows(self.o), Q.fr_rows(self.n)
        self.h = [[Q.height(self.oF[k], self.nF[k], x) for x in self.vF] for k in range(self.K)]
        self.side = [[Q.side(x) for x in row] for row in self.h]

    def sgn(self, k):
        return 1 if self.keep[k] == BELOW else -1

    def flipped(self):
        p = Problem.__new__(Problem)
        p.__dict__.update(self.__dict__)
        p.keep = [1 - x for x in self.keep]
        return p


class View:
    """a result with its corners named so that two runs can be compared: ("v", old index) or ("m", cut, j) for the j-th
    new vertex of the cut (C5: loop points first)"""

    def __init__(self, res):
        self.res = res
        self.V = Q.fr_rows(res.vertices)
        self.vo, self.fo, self.fk = res.vertex_origin.tolist(), res.face_origin.tolist(), res.face_kind.tolist()
        self.faces = [tuple(t) for t in res.faces.tolist()]
        seen, self.name, self.first_new = {}, [], {}
        for i, o in enumerate(self.vo):
            if o >= 0:
                self.name.append(("v", o))
            else:
                k = -1 - o
                self.first_new.setdefault(k, i)
                self.name.append(("m", k, seen.get(k, 0)))
                seen[k] = seen.get(k, 0) + 1
        self.point = {n: self.V[i] for i, n in enumerate(self.name)}
        self.kept = {o for o in self.vo if o >= 0}
        self.pieces = {}                                   # parent -> [named corners] in the result's order
        for t, o, k in zip(self.faces, self.fo, self.fk):
            if k == PIECE:
                self.pieces.setdefault(o, []).append(tuple(self.name[i] for i in t))
        self.untouched = {o for o, k in zip(self.fo, self.fk) if k == UNTOUCHED}

    def cut_of(self, parent):
        (k,) = {n[1] for piece in self.pieces[parent] for n in piece if n[0] == "m"}
        return k


def cut_sets(*views):
    """{cut face: its cut}, from the pieces of a run and its complement (a cut face all of whose pieces are dropped in
    one run keeps some in the other)"""
    out = {}
    for w in views:
        for parent in w.pieces:
            k = w.cut_of(parent)
            assert out.setdefault(parent, k) == k
    return out


def rotations(t):
    return {t, (t[1], t[2], t[0]), (t[2], t[0], t[1])}


def apex_frame(p, face, k):
    """(a, b, c) of C4 from exact sides"""
    t = p.f[face]
    s = [p.side[k][i] for i in t]
    assert not s[0] == s[1] == s[2], "a cut face that the plane does not cross"
    a = 2 if s[0] == s[1] else (1 if s[0] == s[2] else 0)
    return t[a], t[(a + 1) % 3], t[(a + 2) % 3]


def tri_area(P):
    return tuple(x / 2 for x in Q.cross(Q.sub(P[1], P[0]), Q.sub(P[2], P[0])))


def heights_are_exact(p):
    """rule 1's unfused f64 height equals the exact height, for every (plane, vertex)"""
    for k in range(p.K):
        o, n = p.o[k].tolist(), p.n[k].tolist()
        for x, hx in zip(p.v.tolist(), p.h[k]):
            h = (n[0] * (x[0] - o[0]) + n[1] * (x[1] - o[1])) + n[2] * (x[2] - o[2])
            if F(h) != hx:
                return False
    return True


# ---- X1 -------------------------------------------------------------------------------------------------------------------

def x1_sides(p, w, cuts):
    bad, nv = [], len(p.vF)
    dropped = [i not in w.kept for i in range(nv)]
    for k in range(p.K):
        if p.scope[k] == PLANE:
            bad += [("kept on the drop side of plane", k, i) for i in w.kept if p.side[k][i] != p.keep[k]]
    for parent, pieces in w.pieces.items():
        k = cuts[parent]
        bad += [("kept piece corner on the drop side", parent, n[1]) for piece in pieces for n in piece
                if n[0] == "v" and p.side[k][n[1]] != p.keep[k]]
    adj = [[] for _ in range(nv)]
    for i, t in enumerate(p.f):
        if i not in cuts:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                adj[a].append(b); adj[b].append(a)
    reach = [False] * nv
    todo = deque()
    for face, k in cuts.items():
        if p.scope[k] == LOOP:
            for i in p.f[face]:
                if p.side[k][i] != p.keep[k] and not reach[i]:
                    reach[i] = True
                    todo.append(i)
    while todo:
        x = todo.popleft()
        for y in adj[x]:
            if not reach[y]:
                reach[y] = True
                todo.append(y)
    n_checked = 0
    for i in range(nv):
        must = reach[i] or any(p.scope[k] == PLANE and p.side[k][i] != p.keep[k] for k in range(p.K))
        n_checked += 1
        if must != dropped[i]:
            bad.append(("dropped without a reason" if dropped[i] else "kept though it hangs on a drop side", i))
    return {"bad": bad, "n_checked": n_checked, "n_vertices": nv, "n_dropped": sum(dropped)}


# ---- X2, X3 ---------------------------------------------------------------------------------------------------------------

def face_parts(p, w1, w2, face, k):
    """the named frame of a cut face (a, m_ab, b, c, m_ca) and the kept pieces of both runs; None where no run kept
    the apex piece"""
    a, b, c = apex_frame(p, face, k)
    both = w1.pieces.get(face, []) + w2.pieces.get(face, [])
    apex = [q for q in both if ("v", a) in q]
    if len(apex) != 1:
        return None, both, (a, b, c)
    q = apex[0]
    while q[0] != ("v", a):
        q = (q[1], q[2], q[0])
    return (("v", a), q[1], ("v", b), ("v", c), q[2]), both, (a, b, c)


def x2_pieces(p, w1, w2, cuts, planar=False):
    bad, n_faces = [], 0
    point = dict(w2.point); point.update(w1.point)
    for i, x in enumerate(p.vF):
        point[("v", i)] = x
    for face, k in cuts.items():
        frame, both, _abc = face_parts(p, w1, w2, face, k)
        n_faces += 1
        if frame is None or len(both) != 3 or frame[1][0] != "m" or frame[4][0] != "m":
            bad.append(("not three pieces with one apex piece", face, both))
            continue
        if any(w1.point[n] != w2.point[n] for q in both for n in q if n[0] == "m" and n in w1.point and n in w2.point):
            bad.append(("a loop point differs between the runs", face))
        areas = [tri_area([point[n] for n in q]) for q in both]
        if tuple(sum(x[d] for x in areas) for d in range(3)) != Q.vector_area([point[n] for n in frame]):
            bad.append(("the pieces do not tile the pentagon", face))
        if planar:
            parent = tri_area([p.vF[i] for i in p.f[face]])
            bad += [("a piece turned against its parent", face, q) for q, x in zip(both, areas) if Q.dot(x, parent) < 0]
    return {"bad": bad, "n_cut_faces": n_faces}


def x3_diagonals(p, w1, w2, cuts):
    bad, ties, n = [], 0, 0
    point = dict(w2.point); point.update(w1.point)
    for face, k in cuts.items():
        frame, both, _abc = face_parts(p, w1, w2, face, k)
        if frame is None:
            bad.append(("no apex piece", face))
            continue
        a, m_ab, b, c, m_ca = frame
        d_c = Q.dot(Q.sub(point[m_ab], p.vF[c[1]]), Q.sub(point[m_ab], p.vF[c[1]]))
        d_b = Q.dot(Q.sub(p.vF[b[1]], point[m_ca]), Q.sub(p.vF[b[1]], point[m_ca]))
        ties += d_c == d_b
        want = [(m_ab, b, c), (m_ab, c, m_ca)] if d_c < d_b else [(m_ab, b, m_ca), (b, c, m_ca)]
        quad = [q for q in both if a not in q]
        n += 1
        if len(quad) != 2 or not all(any(q in rotations(x) for q in quad) for x in want):
            bad.append(("the other diagonal", face, float(d_c), float(d_b), quad))
    return {"bad": bad, "n_ties": ties, "n_quads": n}


# ---- X4 -------------------------------------------------------------------------------------------------------------------

def edge_counts(faces):
    count = {}
    for t in faces:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            count[(a, b)] = count.get((a, b), 0) + 1
    return count


def x4_manifold(V, faces):
    """V: exact points, faces: index triples (a whole result or one connected piece of it)"""
    count = edge_counts(faces)
    bad = [("directed edge", e, c, count.get((e[1], e[0]), 0)) for e, c in count.items() if c != 1 or count.get((e[1], e[0]), 0) != 1]
    used = {i for t in faces for i in t}
    total = tuple(sum(x) for x in zip(*[tri_area([V[i] for i in t]) for t in faces])) if faces else (0, 0, 0)
    if total != (0, 0, 0):
        bad.append(("vector areas do not cancel", [float(x) for x in total]))
    return {"bad": bad, "used": used, "n_faces": len(faces)}


def x4_whole(w):
    out = x4_manifold(w.V, w.faces)
    out["bad"] += [("unused vertex", i) for i in range(len(w.V)) if i not in out["used"]]
    return out


def components(faces):
    """the faces grouped by vertex connectivity"""
    root = {}

    def find(x):
        while root.setdefault(x, x) != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    for t in faces:
        root[find(t[1])] = find(t[0]); root[find(t[2])] = find(t[0])
    out = {}
    for t in faces:
        out.setdefault(find(t[0]), []).append(t)
    return list(out.values())


def signed_volume6(V, faces):
    return sum(Q.dot(V[t[0]], Q.cross(V[t[1]], V[t[2]])) for t in faces)


# ---- X5, X6, X7 -----------------------------------------------------------------------------------------------------------

def rings(p, w, k):
    """per closed loop of cut k: [ring 0, ..., ring L] as vertex indices of the result, from C5's order and rims[k]"""
    rims = [r.tolist() for r in w.res.rims[k]]
    stride = sum(len(r) for r in rims)
    if not rims:
        return []
    first, L = w.first_new[k], p.L
    n_points = int(w.res.cut_points[k])
    if L == 0:
        return [[r] for r in rims]
    assert n_points == stride, "an extension on a cut with open contours: ring 0 is not named by the rims"
    out, at = [], 0
    for r in rims:
        ring0 = list(range(first + at, first + at + len(r)))
        assert r == [first + n_points + (L - 1) * stride + at + i for i in range(len(r))], "C5: the outermost ring"
        out.append([ring0] + [[first + n_points + (j - 1) * stride + at + i for i in range(len(r))] for j in range(1, L + 1)])
        at += len(r)
    return out


def ring_edges(ring):
    return [frozenset((ring[i], ring[(i + 1) % len(ring)])) for i in range(len(ring))]


def x5_rims(p, w):
    bad, n_edges = [], 0
    owners = {}                                            # (kind, cut) -> {undirected edge: faces that hold it}
    for t, o, kind in zip(w.faces, w.fo, w.fk):
        if kind == UNTOUCHED:
            continue
        k = -1 - o if kind != PIECE else None
        if kind == PIECE:
            ks = {-1 - w.vo[i] for i in t if w.vo[i] < 0}
            k = ks.pop() if len(ks) == 1 else None
        d = owners.setdefault((kind, k), {})
        for e in (frozenset((t[0], t[1])), frozenset((t[1], t[2])), frozenset((t[2], t[0]))):
            d[e] = d.get(e, 0) + 1
    for k in range(p.K):
        for r, loop in enumerate(rings(p, w, k)):
            checks = [(PIECE, loop[0], "ring 0 / piece")]
            if p.L:
                checks += [(EXTENSION, loop[0], "ring 0 / extension"), (EXTENSION, loop[-1], "outermost ring / extension")]
            if p.cap:
                checks.append((CAP, loop[-1], "outermost ring / cap"))
            for kind, ring, what in checks:
                d = owners.get((kind, k), {})
                for e in ring_edges(ring):
                    n_edges += 1
                    if d.get(e, 0) != 1:
                        bad.append((what, k, r, sorted(e), d.get(e, 0)))
    return {"bad": bad, "n_edges": n_edges}


def x6_caps(p, w, outward):
    """outward: +1 for an outward-oriented input, -1 for the same input with its faces reversed, 0 for neither (the
    direction is then not judged).  The identity is per loop; the direction is per cut, over all its loops, because the
    inner loop of a nested pair (a plane through the hole of a torus) rightly looks the other way."""
    bad, n_loops = [], 0
    for k in range(p.K):
        caps = [t for t, o, kind in zip(w.faces, w.fo, w.fk) if kind == CAP and o == -1 - k]
        sn = tuple(p.sgn(k) * x for x in p.nF[k])
        whole = (F(0), F(0), F(0))
        loops = rings(p, w, k)
        for r, loop in enumerate(loops):
            rim = loop[-1]
            mine = [t for t in caps if t[0] in set(rim) and t[1] in set(rim)]
            n_loops += 1
            if len(mine) != len(rim) or len({t[2] for t in mine}) != 1:
                bad.append(("cap faces of the loop", k, r, len(mine), len(rim)))
                continue
            total = tuple(sum(x) for x in zip(*[tri_area([w.V[i] for i in t]) for t in mine]))
            poly = Q.vector_area([w.V[i] for i in rim])
            if total != poly and total != tuple(-x for x in poly):
                bad.append(("the cap does not sum to its polygon", k, r))
            whole = tuple(a + b for a, b in zip(whole, total))
        if loops and outward and Q.dot(whole, sn) * outward <= 0:
            bad.append(("the cap looks the wrong way", k, float(Q.dot(whole, sn))))
    return {"bad": bad, "n_loops": n_loops}


def exact_sqrt(x, bits=200):
    """sqrt of a rational to 2^-bits relative"""
    s = F(2) ** (2 * bits)
    return F(math.isqrt(int(x * s * s)), 1) / s


def x7_extension(p, w):
    bad, worst, n = [], F(0), 0
    ext = F(p.ext_length)
    for k in range(p.K):
        norm = exact_sqrt(Q.dot(p.nF[k], p.nF[k]))
        for r, loop in enumerate(rings(p, w, k)):
            for j in range(1, p.L + 1):
                t = p.sgn(k) * j * ext / p.L
                for i0, ij in zip(loop[0], loop[j]):
                    P, q = w.V[i0], w.V[ij]
                    scale = max(max(abs(x) for x in P), ext)
                    for d in range(3):
                        ratio = abs(q[d] - (P[d] + t * p.nF[k][d] / norm)) / (EPS * scale)
                        worst = max(worst, ratio)
                        n += 1
                        if ratio > C7:
                            bad.append(("ring point off its place", k, r, j, float(ratio)))
    return {"bad": bad, "worst_ratio": float(worst), "n_components": n}


# ---- X8 -------------------------------------------------------------------------------------------------------------------

def exact_loop_points(p, w, cuts):
    """every loop point of every piece is the exact crossing of its edge (stored bits == exact crossing)"""
    for face, k in cuts.items():
        a, b, c = apex_frame(p, face, k)
        for q in w.pieces.get(face, []):
            if ("v", a) not in q:
                continue
            while q[0] != ("v", a):
                q = (q[1], q[2], q[0])
            for m, other in ((q[1], b), (q[2], c)):
                if w.point[m] != Q.crossing(p.vF[a], p.vF[other], p.h[k][a], p.h[k][other]):
                    return False
    return True


def x8_complement(p, w1, w2, cuts, closed=False):
    """w1: the run, w2: the run with every keep flipped"""
    bad = []
    if not (w1.res.applied and w2.res.applied):
        return {"bad": [("not applied", w1.res.cut_status.tolist(), w2.res.cut_status.tolist())]}
    if w1.kept & w2.kept:
        bad.append(("kept in both runs", sorted(w1.kept & w2.kept)[:5]))
    if w1.untouched & w2.untouched:
        bad.append(("untouched in both runs", sorted(w1.untouched & w2.untouched)[:5]))
    for face, k in cuts.items():
        frame, both, _abc = face_parts(p, w1, w2, face, k)
        if frame is None or len(both) != 3:
            bad.append(("not three pieces over the two runs", face, len(both)))
            continue
        a, m_ab, b, c, m_ca = frame
        want = [{(a, m_ab, m_ca)}, {(m_ab, b, c), (m_ab, b, m_ca)}, {(m_ab, c, m_ca), (b, c, m_ca)}]
        got = [[any(q in rotations(x) for x in alt) for alt in want] for q in both]
        if sorted(row.index(True) if True in row else -1 for row in got) != [0, 1, 2]:
            bad.append(("the pieces of the two runs are not C4's three", face, both))
        # one run holds the apex piece, the other the quad (a LOOP cut may leave a run neither)
        mine = {q for q in w1.pieces.get(face, [])}
        if mine & set(w2.pieces.get(face, [])):
            bad.append(("a piece kept in both runs", face))
    n_points = 0
    for k in range(p.K):
        m = int(w1.res.cut_points[k])
        if m != int(w2.res.cut_points[k]):
            bad.append(("loop points counted differently", k))
            continue
        a = w1.res.vertices[w1.first_new[k]:w1.first_new[k] + m] if m else np.zeros((0, 3))
        b = w2.res.vertices[w2.first_new[k]:w2.first_new[k] + m] if m else np.zeros((0, 3))
        n_points += m
        if a.tobytes() != b.tobytes():
            bad.append(("loop points differ in bits", k))
    out = {"bad": bad, "n_loop_points": n_points}
    if p.cap and p.L == 0:
        named = lambda w: [tuple(w.name[i] for i in t) for t, kind in zip(w.faces, w.fk) if kind == CAP]     # noqa: E731
        c1, c2 = named(w1), named(w2)
        if len(c1) != len(c2) or any((y[1], y[0], y[2]) != x for x, y in zip(c1, c2)):
            bad.append(("cap faces are not reversed copies", len(c1), len(c2)))
        out["n_caps"] = len(c1)
        if closed:
            v_in = signed_volume6(p.vF, p.f)
            diff = abs(signed_volume6(w1.V, w1.faces) + signed_volume6(w2.V, w2.faces) - v_in) / 6
            M = max(abs(x) for row in p.vF for x in row)
            bound = F(0)
            for face in cuts:
                P = [p.vF[i] for i in p.f[face]]
                per = sum(exact_sqrt(Q.dot(Q.sub(P[(i + 1) % 3], P[i]), Q.sub(P[(i + 1) % 3], P[i])), 80) for i in range(3))
                bound += C1_E1 * EPS * M * per * M / 2
            out.update(volume_diff=float(diff), volume_bound=float(bound), volume_ratio=float(diff / bound) if bound else 0.0,
                       volume_exact=diff == 0)
            if diff > bound:
                bad.append(("the volumes do not add up", float(diff), float(bound)))
    return out


# ---- X9 -------------------------------------------------------------------------------------------------------------------

def x9_order(p, w):
    bad = []
    vo = w.vo
    n_old = sum(o >= 0 for o in vo)
    if any(o < 0 for o in vo[:n_old]) or any(a >= b for a, b in zip(vo[:n_old], vo[1:n_old])):
        bad.append("kept old vertices do not come first, ascending")
    cuts = [-1 - o for o in vo[n_old:]]
    if any(o < 0 or o >= p.K for o in cuts) or any(a > b for a, b in zip(cuts, cuts[1:])):
        bad.append("new vertices are not grouped per cut in cut order")
    block = [0 if k in (UNTOUCHED, PIECE) else (1 if k == EXTENSION else 2) for k in w.fk]
    if any(a > b for a, b in zip(block, block[1:])):
        bad.append("face kinds do not come in blocks")
    n0 = block.count(0)
    if any(o < 0 for o in w.fo[:n0]) or any(a > b for a, b in zip(w.fo[:n0], w.fo[1:n0])):
        bad.append("parents decrease in the first block")
    for kind, code in ((EXTENSION, 1), (CAP, 2)):
        ks = [-1 - o for o, b in zip(w.fo, block) if b == code]
        if any(k < 0 or k >= p.K for k in ks) or any(a > b for a, b in zip(ks, ks[1:])):
            bad.append(f"faces of kind {kind} are not grouped per cut in cut order")
    seen = {}
    for o, k in zip(w.fo[:n0], w.fk[:n0]):
        seen.setdefault(o, set()).add(k)
    if any(len(s) != 1 for s in seen.values()):
        bad.append("a parent both untouched and in pieces")
    if any(o >= 0 and w.V[i] != p.vF[o] for i, o in enumerate(vo)):
        bad.append("a kept old vertex changed its bits")
    return {"bad": bad, "n_old": n_old, "n_first_block": n0}
