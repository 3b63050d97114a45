"""Meshes, queries and cached checker results shared by tests/test_winding_host.py and tests/test_gpu_winding.py.  Every
case is small; the checker (tests/mm_checkers/winding_number.py) runs once per case and process."""
import functools

import numpy as np

from mm_checkers import winding_number as chk

H_LIST = (1e-3, 1e-6, 1e-9, 1e-12)


def plan(n_staged):
    from multimoda_rs_amd import winding
    return winding.winding_plan(n_staged)


def volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def uv_sphere(n_lon, n_lat, radius=1.0, center=(0.0, 0.0, 0.0)):
    """closed, outward: 2 n_lon (n_lat - 1) faces"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon                              # noqa: E731
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    last = len(v) - 1
    f += [(last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)) for j in range(n_lon)]
    return np.array(v) * radius + np.array(center), np.array(f, dtype=np.int64)


def tube(n_around=24, n_along=12, radius=0.5, length=2.0, center=(0.0, 0.0, 0.0)):
    """open at both ends, outward, along z: 2 n_around n_along faces"""
    v = [(radius * np.cos(2 * np.pi * j / n_around), radius * np.sin(2 * np.pi * j / n_around), length * (i / n_along - 0.5))
         for i in range(n_along + 1) for j in range(n_around)]
    at = lambda i, j: i * n_around + j % n_around                                    # noqa: E731
    f = []
    for i in range(n_along):
        for j in range(n_around):
            f += [(at(i, j), at(i, j + 1), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i + 1, j))]
    return np.array(v) + np.array(center), np.array(f, dtype=np.int64)


def box(lo, hi):
    """closed, outward, 12 faces"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(lo, hi)[(k >> d) & 1][d] for d in range(3)] for k in range(8)])
    f = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2),
         (1, 3, 7), (1, 7, 5)]
    return v, np.array(f, dtype=np.int64)


def octahedron():
    """Corners at distance 3 on the axes, faces alternating between the +x and the -x half.  Seen from (4, 0, 0) every
    corner is at an integer distance (1, 5 or 7) and every coordinate difference is an integer, so den and num of every
    face are integers and the fold multiplies Gaussian integers: a face of the near half and its mirror image multiply to
    a real number, every product fits 53 bits until the last, real, one, and the remainder's imaginary part is exactly 0."""
    v = np.array([[3, 0, 0], [-3, 0, 0], [0, 3, 0], [0, -3, 0], [0, 0, 3], [0, 0, -3]], dtype=np.float64)
    near = [(0, 2, 4), (0, 4, 3), (0, 3, 5), (0, 5, 2)]
    f = []
    for (a, b, c) in near:
        f += [(a, b, c), (1, c, b)]
    return v, np.array(f, dtype=np.int64)


def tetrahedron():
    """Corners with integer coordinates and integer norms (5, 5, 5, 10) on the far side of x + y + z = 7 from the origin:
    seen from the origin every den and num is an integer and the four-face product fits 53 bits."""
    v = np.array([[3, 4, 0], [4, 3, 0], [0, 3, 4], [6, 0, 8]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=np.int64)
    if volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v, f


def tetrahedron_about_origin():
    """corners at integer distances (1, 1, 1, 3) from the origin, which lies inside"""
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, -2, -2]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=np.int64)
    if volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v, f


@functools.lru_cache(maxsize=None)
def sphere8192():
    return uv_sphere(64, 65)


@functools.lru_cache(maxsize=None)
def sphere512():
    return uv_sphere(16, 17)


@functools.lru_cache(maxsize=None)
def queries513():
    """513 points in [-1.5, 1.5]^3: inside and outside the unit sphere"""
    return np.random.default_rng(20261020).uniform(-1.5, 1.5, size=(513, 3))


def sphere_cut(n_faces):
    v, f = sphere8192()
    return v, f[:n_faces].copy()


def point_triangle_distance(q, v, f):
    """(nq,) distance to the nearest face: the plane distance where the projection is inside, else the nearest edge"""
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    p = q[:, None, :]
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=2, keepdims=True)
    h = ((p - a) * n).sum(axis=2)
    proj = p - h[..., None] * n
    inside = np.ones(h.shape, dtype=bool)
    for (u, w) in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(w - u, proj - u) * n).sum(axis=2) >= 0
    best = np.where(inside, np.abs(h), np.inf)
    for (u, w) in ((a, b), (b, c), (c, a)):
        e = w - u
        t = np.clip(((p - u) * e).sum(axis=2) / (e * e).sum(axis=2), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (u + t[..., None] * e), axis=2))
    return best.min(axis=1)


def adversarial(v, f, stride):
    """Queries next to every stride-th face: (points, kind, h) with kind 0 = over the face's interior, 1 = over an edge
    midpoint, 2 = over a corner, 3 = in the face's plane outside the triangle; h = the offset along the face's normal (0.0:
    on the face, up to the rounding of the point itself)."""
    pts, kind, hs = [], [], []
    for i in range(0, f.shape[0], stride):
        a, b, c = v[f[i, 0]], v[f[i, 1]], v[f[i, 2]]
        n = np.cross(b - a, c - a)
        n = n / np.linalg.norm(n)
        inner = 0.5 * a + 0.25 * b + 0.25 * c
        bases = [(0, inner)] + [(1, 0.5 * (x + y)) for x, y in ((a, b), (b, c), (c, a))] + [(2, x) for x in (a, b, c)]
        for k, base in bases:
            for h in (0.0,) + H_LIST:
                for sgn in ((1.0,) if h == 0.0 else (1.0, -1.0)):
                    pts.append(base + (sgn * h) * n)
                    kind.append(k)
                    hs.append(sgn * h)
        pts.append(inner + 3.0 * (a - inner))
        kind.append(3)
        hs.append(0.0)
    return np.array(pts), np.array(kind), np.array(hs)


def with_degenerates(v, f, seed=5):
    """the mesh with degenerate faces -- a repeated index; three corners on one axis-parallel line, on three new
    vertices -- put in first, last and at random places"""
    rng = np.random.default_rng(seed)
    m = v.shape[0]
    v2 = np.vstack([v, [[0.25, 0.5, 0.75], [0.25, 0.5, 1.0], [0.25, 0.5, 2.0]]])
    faces = list(map(tuple, f))
    for t in ((3, 3, 7), (5, 9, 5), (2, 4, 4), (m, m, m), (m, m + 1, m + 2), (m + 2, m, m + 1)):
        faces.insert(int(rng.integers(0, len(faces) + 1)), t)
    faces.insert(0, (1, 1, 2))
    faces.append((m, m + 2, m + 1))
    return v2, np.array(faces, dtype=np.int64)


# name -> (points, vertices, faces): every case the device must reproduce bit for bit and that needs no engine
@functools.lru_cache(maxsize=None)
def case(name):
    q = queries513()
    if name == "octahedron":
        return (np.array([[0, 0, 0], [4, 0, 0], [1, 0.5, 0.25], [5, 5, 5], [-4, 0, 0], [1, 1, 1]], dtype=np.float64),) + octahedron()
    if name == "octahedron_inward":
        v, f = octahedron()
        return (np.array([[0, 0, 0], [4, 0, 0], [1, 0.5, 0.25]], dtype=np.float64), v, f[:, ::-1].copy())
    if name == "tetrahedron":
        return (np.array([[0, 0, 0], [3.25, 2.5, 3], [10, 10, 10]], dtype=np.float64),) + tetrahedron()
    if name == "tetrahedron_about_origin":
        return (np.array([[0, 0, 0], [2, 2, 2], [0.1, 0.1, 0.1]], dtype=np.float64),) + tetrahedron_about_origin()
    if name == "sphere8192":
        return (q,) + sphere8192()
    if name == "q513cut511":
        return (q,) + sphere_cut(511)
    if name.startswith("cut"):
        return (q[:7],) + sphere_cut(int(name[3:]))
    if name == "tube":
        return (np.vstack([q[:40] * np.array([0.5, 0.5, 1.0]), [[0, 0, 0], [0, 0, 0.9], [0, 0, 1.0], [0, 0, 1.5], [0.1, 0.2, -1.0]]]),) + tube()
    if name == "adversarial_sphere":
        v, f = sphere512()
        return (adversarial(v, f, 16)[0], v, f)
    if name == "adversarial_tube":
        v, f = tube()
        return (adversarial(v, f, 18)[0], v, f)
    if name == "degenerate":
        v, f = sphere512()
        return (q[:33],) + with_degenerates(v, f)
    if name == "degenerate_only":
        v, f = with_degenerates(*sphere512())
        keep = chk.staged_faces(v, f)
        return (q[:5], v, np.delete(f, keep, axis=0))
    raise KeyError(name)


BIT_CASES = ("octahedron", "octahedron_inward", "tetrahedron", "tetrahedron_about_origin", "sphere8192", "cut511", "cut513",
             "cut255", "cut256", "cut257", "cut1", "q513cut511", "tube", "adversarial_sphere", "adversarial_tube", "degenerate",
             "degenerate_only")


def get(name):
    return case(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the checker's full result for a case"""
    q, v, f = get(name)
    return chk.winding(q, v, f, plan)


@functools.lru_cache(maxsize=None)
def expected_reference(name):
    q, v, f = get(name)
    return chk.reference(q, v, f)
