"""Sliver faces on which the closest point of a triangle (include/mm_ccta.h, "surface distance"; csrc/mm_tri_device.h) is
easiest to get wrong, shared by tests/test_surface_sliver_host.py (the rule against exact rational arithmetic, host only)
and tests/test_gpu_surface_sliver.py (the device against the checker).  Data only; every case is seeded.

A family is (vertices, faces, queries): at most 48 faces of 3 vertices of their own, and 48 queries for each face
(queries[k] belongs to face k; the device tests run all of them against all faces).

* needles: a = 0, b = 2 e1, c = 2 e1 + h e2 -- the short third edge; h = 2^(1-k) makes smallest altitude / longest edge
  2^-k up to O(h^2).
* caps: a = 0, b = 2 e1, c = 1.3 e1 + h e2 -- the obtuse corner over the long edge.
* k in RATIOS: 8 ... 50 as the issue of this test sets them and THIN_K -+ 1/2, a factor sqrt(2) either side of the
  threshold of the thin rule (tests/mm_checkers/surface_distance.py: THIN_K).
* "random": (e1, e2, e3) a random rotation; "axis": the coordinate axes, cyclically -- the thinnest possible box.
* every face at the origin, translated by 100 and by 1e4 (each coordinate by another multiple, rounded as it falls).
* collinear: c = a + t (b - a) as rounded, not degenerate by the rule's exact test; and lattice faces whose c is one ulp
  either side of exactly collinear, with the degenerate one between them.
"""
import numpy as np

from mm_checkers import surface_distance as S

RATIOS = (8, 12, 16, S.THIN_K - 0.5, S.THIN_K + 0.5, 20, 24, 30, 40, 50)
OFFSETS = (0.0, 100.0, 1.0e4)
HEIGHTS = (0.0, 2.0 ** -40, 2.0 ** -10, 0.5)                # of the longest edge, along the normal
STEPS = (-3.0, -1.0, -0.25, 0.25, 1.0, 3.0)                 # altitudes outside an edge (negative: inside)
LATTICE = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.5, 0.5), (0.5, 0, 0.5), (0.375, 0.25, 0.375))
PER_FACE = 48


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _queries(a, b, c, alt):
    """48 queries of the face (a, b, c) given in its own frame (the face in the plane z = 0, `alt` its nominal
    altitude): the lattice at the four heights, the steps outside each edge at 0.37 of it, and beyond both ends of the
    longest edge."""
    tri = np.array([a, b, c], dtype=np.float64)
    edges = [(tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])]
    longest = max(np.linalg.norm(v - u) for u, v in edges)
    q = []
    for h in HEIGHTS:
        for w in LATTICE:
            q.append(np.asarray(w) @ tri + [0.0, 0.0, h * longest])
    inside = tri.mean(axis=0)
    for u, v in edges:
        e = (v - u) / np.linalg.norm(v - u)
        out = np.array([e[1], -e[0], 0.0])
        if out @ (inside - u) > 0:
            out = -out
        for s in STEPS:
            q.append(u + 0.37 * (v - u) + out * (s * alt))
    u, v = max(edges, key=lambda uv: np.linalg.norm(uv[1] - uv[0]))
    q += [u - 0.25 * (v - u), v + 0.125 * (v - u) + [0.0, alt, 0.0]]
    assert len(q) == PER_FACE
    return np.array(q)


def _family(shape, placement, seed):
    rng = np.random.default_rng(seed)
    vs, qs = [], []
    for n, (k, off) in enumerate((k, off) for k in RATIOS for off in OFFSETS):
        h = 2.0 ** (1.0 - k)
        a, b = np.zeros(3), np.array([2.0, 0.0, 0.0])
        c = np.array([2.0, h, 0.0]) if shape == "needle" else np.array([1.3, h, 0.0])
        frame = _rotation(rng) if placement == "random" else np.roll(np.eye(3), n % 3, axis=0)
        shift = off * np.array([1.0, -0.75, 0.5])
        vs.append(np.array([a, b, c]) @ frame + shift)
        qs.append(_queries(a, b, c, h) @ frame + shift)
    v = np.concatenate(vs)
    return v, np.arange(len(v)).reshape(-1, 3), np.array(qs)


def _own_frame(a, b, c, alt):
    """Queries of a face given in world coordinates: a frame from the longest edge and any direction across it."""
    e1 = (b - a) / np.linalg.norm(b - a)
    e2 = np.cross(e1, [0.0, 0.0, 1.0] if abs(e1[2]) < 0.9 else [1.0, 0.0, 0.0])
    e2 /= np.linalg.norm(e2)
    frame = np.array([e1, e2, np.cross(e1, e2)])
    local = [(x - a) @ frame.T for x in (a, b, c)]
    return _queries(local[0], local[1], local[2], alt) @ frame + a


def _collinear(seed):
    rng = np.random.default_rng(seed)
    vs, qs = [], []
    for off in OFFSETS:
        for t in (0.25, 0.5, 0.7, 1.0 / 3.0, 1.5, -0.5):
            while True:
                a = rng.uniform(-1.0, 1.0, 3) + off * np.array([1.0, -0.75, 0.5])
                b = a + rng.uniform(-1.0, 1.0, 3)
                c = a + t * (b - a)
                tri = np.array([a, b, c])
                if S.face_kind(tri, (0, 1, 2)) != S.DEGENERATE:       # rounding left it a (thin) face
                    break
            u, w, third = {1.5: (a, c, b), -0.5: (c, b, a)}.get(t, (a, b, c))     # (u, w) the longest edge
            vs.append(tri)
            qs.append(_own_frame(u, w, third, 2.0 ** -40))
    a, b, c = np.array([1.0, 1.0, 1.0]), np.array([3.0, 5.0, 7.0]), np.array([2.0, 3.0, 4.0])
    for cy in (np.nextafter(3.0, 0.0), 3.0, np.nextafter(3.0, 9.0)):
        tri = np.array([a, b, [c[0], cy, c[2]]])
        vs.append(tri)
        qs.append(_own_frame(a, b, tri[2], 2.0 ** -40))
    v = np.concatenate(vs)
    return v, np.arange(len(v)).reshape(-1, 3), np.array(qs)


def families():
    """name -> (vertices, faces, queries (n_faces, 48, 3))."""
    out = {f"{shape}_{placement}": _family(shape, placement, 100 + 10 * i + j)
           for i, shape in enumerate(("needle", "cap")) for j, placement in enumerate(("random", "axis"))}
    out["collinear"] = _collinear(7)
    return out


def nominal_ratio(name, face):
    """The k of face `face` of a needle or cap family (its smallest altitude / longest edge is 2^-k before rounding)."""
    return RATIOS[face // len(OFFSETS)]


def _tilt(v):
    cx, sx, cz, sz = np.cos(0.3), np.sin(0.3), np.cos(0.05), np.sin(0.05)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return v @ rx.T @ rz.T


def sliver_strip(n=516):
    """(vertices, faces, queries): n faces in a row along x (three chunks of 256), every fourth a cap of ratio 2^-20, the
    whole tilted so that no operation is exact; two queries a face (more than two blocks of 512): one on it and one
    raised from it by 2^-30, 2^-12 or 0.1."""
    v, q = [], []
    h = 0.5 * 2.0 ** -20
    for i in range(n):
        a, b = np.array([i, 0.25, 0.5]), np.array([i + 0.5, 0.25, 0.5])
        c = np.array([i + 0.2, 0.25 + h, 0.5]) if i % 4 == 3 else np.array([float(i), 0.75, 0.5])
        v += [a, b, c]
        on = 0.3 * a + 0.3 * b + 0.4 * c
        q += [on, on + [0.0, 0.0, (2.0 ** -30, 2.0 ** -12, 0.1)[i % 3]]]
    v = _tilt(np.array(v))
    return v, np.arange(len(v)).reshape(-1, 3), _tilt(np.array(q))


SQUEEZED_RINGS = (20, 21)       # ring 21 is brought to 2^-20 of the spacing above ring 20
CAP_RING = 10                   # every other vertex of this ring is moved onto the opposite edge of ring 11, plus 2^-20


def squeezed_tube():
    """wound_tube(12, 41) with ring 21 at 2^-20 above ring 20 (a band of needles) and every other vertex of ring 10 moved
    to 0.4 / 0.6 along the edge of ring 11 opposite to it, 2^-20 below it (caps).  The topology is the tube's."""
    from test_refine_host import wound_tube
    n = 12
    v, f = wound_tube(n, 41)
    v = v.copy()
    lo, hi = SQUEEZED_RINGS
    v[hi * n:(hi + 1) * n, 2] = v[lo * n, 2] + 2.0 ** -20
    ring, nxt = set(range(CAP_RING * n, (CAP_RING + 1) * n)), set(range((CAP_RING + 1) * n, (CAP_RING + 2) * n))
    moved = 0
    for t in f:
        mine = [int(x) for x in t if int(x) in ring]
        others = [int(x) for x in t if int(x) in nxt]
        if len(mine) == 1 and len(others) == 2 and mine[0] % 2 == 1:
            v[mine[0]] = 0.4 * v[others[0]] + 0.6 * v[others[1]] - [0.0, 0.0, 2.0 ** -20]
            moved += 1
    assert moved == n // 2
    return v, f
