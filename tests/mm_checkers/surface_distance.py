"""Plain numpy restatement of the surface distance (include/mm_ccta.h, "surface distance"): the yardstick for
csrc/mm_tri_kernels.hip and csrc/mm_surface.cpp.  Vectorised over the queries, one face at a time; numpy's elementwise
f64 operations are IEEE and unfused, so every line below is one rounding, in the header's order.

* `face_kind`: 0 a proper face, 1 a degenerate one, 2 a thin one (the header's f64 test on ab x ac and the longest edge).
* `closest_on_face`: Ericson's closest point of a proper face, the first test that holds winning; the segment rule of a
  degenerate one; of a thin one the segment rule and then the interior candidate; the region with it.
* `scan`: the fold over the faces in index order with strict <, unpruned: the lowest face index wins ties, a NaN never.
* `predict_report`: the integer report fields of mm_point_mesh_distance that do not depend on the data.
"""
import numpy as np

LAUNCHES = 4                    # fill, pass A, the who pass, the closest points; pass B is one more where it has items


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def along(u, e, t):
    """u + e * t per component: one product, one sum."""
    return u + e * np.asarray(t)[..., None]


def is_degenerate(v, face):
    i, j, k = (int(x) for x in face)
    if i == j or j == k or i == k:
        return True
    with np.errstate(all="ignore"):
        ab, ac = v[j] - v[i], v[k] - v[i]
        n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    return n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0


THIN_K = 17                     # thin: (smallest altitude / longest edge)^2 < 2^-34 as computed; see the header
THIN_SQ = 2.0 ** (-2 * THIN_K)
PROPER, DEGENERATE, THIN = 0, 1, 2


def face_kind(v, face):
    """0, 1 (degenerate: is_degenerate) or 2 (thin: dot(n, n) < 2^-34 * (l * l) with n = ab x ac and l the largest of
    dot(ab, ab), dot(ac, ac), dot(bc, bc), bc = c - b)."""
    if is_degenerate(v, face):
        return DEGENERATE
    i, j, k = (int(x) for x in face)
    with np.errstate(all="ignore"):
        ab, ac, bc = v[j] - v[i], v[k] - v[i], v[k] - v[j]
        n = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]])
        l = dot(ab, ab)
        for e in (ac, bc):
            m = dot(e, e)
            l = m if m > l else l
        return THIN if dot(n, n) < THIN_SQ * (l * l) else PROPER


def _segment(p, u, v):
    e = v - u
    l = dot(e, e)
    if l == 0.0:
        t = np.zeros(len(p))
    else:
        t = dot(p - u, e) / l
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))          # a NaN stays a NaN
    return along(u, e, t)


def dist_sq(p, q):
    d = p - q
    return dot(d, d)


def _segments(p, a, b, c):
    """(closest, its d2, region 4 5 6): the nearest of ab, bc, ca, the first on ties."""
    q = _segment(p, a, b)
    best = dist_sq(p, q)
    region = np.full(len(p), 4, dtype=np.int32)
    for r, (u, w) in ((5, (b, c)), (6, (c, a))):
        q2 = _segment(p, u, w)
        v2 = dist_sq(p, q2)
        take = v2 < best
        best = np.where(take, v2, best)
        q = np.where(take[:, None], q2, q)
        region = np.where(take, r, region).astype(np.int32)
    return q, best, region


def closest_on_face(p, a, b, c, kind):
    """(closest (n, 3), region (n,)) of the queries p (n, 3) on the face (a, b, c) of kind 0, 1 or 2 (face_kind; False and
    True stand for 0 and 1)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    n = len(p)
    kind = int(kind)
    with np.errstate(all="ignore"):
        if kind == DEGENERATE:
            q, _, region = _segments(p, a, b, c)
            return q, region
        ab, ac = b - a, c - a
        if kind == THIN:
            q, best, region = _segments(p, a, b, c)
            ap, bp, cp = p - a, p - b, p - c
            d1, d2 = dot(ab, ap), dot(ac, ap)
            d3, d4 = dot(ab, bp), dot(ac, bp)
            d5, d6 = dot(ab, cp), dot(ac, cp)
            vc = d1 * d4 - d3 * d2
            vb = d5 * d2 - d1 * d6
            va = d3 * d6 - d5 * d4
            s = (va + vb) + vc
            q0 = along(along(a, ab, vb / s), ac, vc / s)
            take = (va > 0.0) & (vb > 0.0) & (vc > 0.0) & (dist_sq(p, q0) < best)
            return np.where(take[:, None], q0, q), np.where(take, 0, region).astype(np.int32)
        ap = p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        cases = (
            (1, (d1 <= 0.0) & (d2 <= 0.0), lambda: np.broadcast_to(a, (n, 3))),
            (2, (d3 >= 0.0) & (d4 <= d3), lambda: np.broadcast_to(b, (n, 3))),
            (4, (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), lambda: along(a, ab, d1 / (d1 - d3))),
            (3, (d6 >= 0.0) & (d5 <= d6), lambda: np.broadcast_to(c, (n, 3))),
            (6, (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), lambda: along(a, ac, d2 / (d2 - d6))),
            (5, (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0), lambda: along(b, c - b, e43 / (e43 + e56))),
        )
        q = along(along(a, ab, vb / s), ac, vc / s)
        region = np.zeros(n, dtype=np.int32)
        open_ = np.ones(n, dtype=bool)
        for r, holds, point in cases:
            take = open_ & holds
            if take.any():
                q = np.where(take[:, None], point(), q)
                region[take] = r
            open_ &= ~holds
        return q, region


def scan(points, vertices, faces):
    """(sq (n,), face (n,) int64, closest (n, 3), region (n,) int32): every face against every query, unpruned."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = len(p)
    sq = np.full(n, np.inf)
    face = np.full(n, -1, dtype=np.int64)
    closest = np.full((n, 3), np.nan)
    region = np.full(n, -1, dtype=np.int32)
    for k, t in enumerate(f):
        q, r = closest_on_face(p, v[t[0]], v[t[1]], v[t[2]], face_kind(v, t))
        with np.errstate(all="ignore"):
            d = dist_sq(p, q)
            take = d < sq
        sq[take], face[take], closest[take], region[take] = d[take], k, q[take], r[take]
    return sq, face, closest, region


def pair_sq(points, vertices, faces):
    """(n_faces, n_queries): d2 of every pair."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(faces), len(p)))
    for k, t in enumerate(np.asarray(faces, dtype=np.int64).reshape(-1, 3)):
        with np.errstate(all="ignore"):
            out[k] = dist_sq(p, closest_on_face(p, v[t[0]], v[t[1]], v[t[2]], face_kind(v, t))[0])
    return out


def up256(n):
    return (n + 255) // 256 * 256


def predict_report(nq, nf, qpb, chunk):
    """The report fields the data does not decide: one item of pass A per query block, every other (block, chunk)
    combination in pass B; the uploads (staged faces of 96 bytes, queries of 24, items of 16) and the downloads (per
    query 8 + 8 + 24 + 4 bytes, one counter), each buffer rounded up to 256 bytes."""
    if nq == 0 or nf == 0:
        return dict(items_pass_a=0, items_pass_b=0, n_launches=0, bytes_uploaded=0, bytes_downloaded=0)
    nqb, nch = -(-nq // qpb), -(-nf // chunk)
    return dict(items_pass_a=nqb, items_pass_b=nqb * (nch - 1), n_launches=LAUNCHES + (1 if nch > 1 else 0),
                bytes_uploaded=up256(96 * nf) + up256(24 * nq) + up256(16 * nqb * nch),
                bytes_downloaded=up256(8 * nq) + up256(8 * nq) + up256(24 * nq) + up256(4 * nq) + 256)
