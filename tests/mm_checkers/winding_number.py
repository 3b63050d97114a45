"""Plain numpy restatement of the winding number (include/mm_ccta.h, "winding number"): the yardstick for
mm.mesh_winding_number and the functions built on it.  Vectorised over the queries, a Python loop over the faces; every
operation is one unfused f64 numpy operation in the header's order, np.frexp / np.ldexp are exact, and the final atan2 is
math.atan2, the C library's.  The grouping (faces per chunk, chunks per group) comes from mm_winding_plan.

`reference` is independent of the rule: sum_f atan2(num, den) / 2 pi in np.longdouble."""
import math

import numpy as np

C1, C2, RHO_MIN = 4.0, 9.0, 2.0 ** -40
TOUCH, TINY_Z, TINY_LEN2 = 2.0 ** -47, 2.0 ** -600, 2.0 ** -960


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def is_degenerate(v, t):
    """a repeated index, or every component of ab x ac exactly 0.0 ("surface distance")"""
    if t[0] == t[1] or t[1] == t[2] or t[0] == t[2]:
        return True
    a, b, c = v[t[0]], v[t[1]], v[t[2]]
    ab, ac = b - a, c - a
    nx, ny, nz = ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]
    return nx == 0.0 and ny == 0.0 and nz == 0.0


def staged_faces(v, f):
    """rule 1: the indices of the faces that are staged, in the caller's order"""
    return np.array([i for i in range(f.shape[0]) if not is_degenerate(v, f[i])], dtype=np.int64)


def cone(re, im):
    """rule 3, elementwise: (m, re', im')"""
    c1 = (im > re) & (im >= -re) & (im > 0.0)
    c2 = ~c1 & (im < -re) & (im <= re) & (im < 0.0)
    c3 = ~c1 & ~c2 & (re < 0.0)
    m = np.where(c1, 1, np.where(c2, -1, np.where(c3, np.where(im >= 0.0, 2, -2), 0))).astype(np.int64)
    r = np.where(c1, im, np.where(c2, -im, np.where(c3, -re, re)))
    i = np.where(c1, -re, np.where(c2, re, np.where(c3, -im, im)))
    return m, r, i


class State:
    """(n, P, rho, touch) of every query"""

    def __init__(self, nq):
        self.n = np.zeros(nq, dtype=np.int64)
        self.pr, self.pi = np.ones(nq), np.zeros(nq)
        self.rho = np.full(nq, np.inf)
        self.touch = np.zeros(nq, dtype=bool)


def turn(s, live, m, zr, zi):
    """rule 4 for the queries of `live`"""
    qr, qi = s.pr * zr - s.pi * zi, s.pr * zi + s.pi * zr
    m2, qr, qi = cone(qr, qi)
    assert (np.abs(m2[live]) <= 1).all()
    _, e = np.frexp(qr)
    s.n = np.where(live, s.n + (m + m2), s.n)
    s.pr = np.where(live, np.ldexp(qr, -e), s.pr)
    s.pi = np.where(live, np.ldexp(qi, -e), s.pi)


def fold_face(s, p, A, B, C):
    """rules 2, 5 and 6 for one face"""
    ax, ay, az = A[0] - p[:, 0], A[1] - p[:, 1], A[2] - p[:, 2]
    bx, by, bz = B[0] - p[:, 0], B[1] - p[:, 1], B[2] - p[:, 2]
    cx, cy, cz = C[0] - p[:, 0], C[1] - p[:, 1], C[2] - p[:, 2]
    aa, bb, cc = _dot(ax, ay, az, ax, ay, az), _dot(bx, by, bz, bx, by, bz), _dot(cx, cy, cz, cx, cy, cz)
    la, lb, lc = np.sqrt(aa), np.sqrt(bb), np.sqrt(cc)
    L = (la * lb) * lc
    ux, uy, uz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
    num = (ax * ux + ay * uy) + az * uz
    den = ((la * lb) * lc + _dot(ax, ay, az, bx, by, bz) * lc) + (_dot(bx, by, bz, cx, cy, cz) * la + _dot(cx, cy, cz, ax, ay, az) * lb)
    an, ad = np.abs(num), np.abs(den)
    mx = np.where(ad > an, ad, an)
    least = np.where(aa < bb, aa, bb)
    least = np.where(cc < least, cc, least)
    zero = (mx < TINY_Z) | (least < TINY_LEN2)
    live = ~zero
    s.touch |= live & (den <= 0.0) & (an <= TOUCH * L)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = mx / L
    s.rho = np.where(zero, 0.0, np.where(rho < s.rho, rho, s.rho))
    m, zr, zi = cone(den, num)
    turn(s, live, m, zr, zi)


def fold(points, v, f, plan):
    """Rules 1 to 7: dict(turns, p, rho, touch, n_staged).  plan(n_staged) -> dict with "chunk", "chunks_per_group" and
    "groups" (mm.winding.winding_plan)."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    keep = staged_faces(v, f)
    nq, ns = points.shape[0], keep.shape[0]
    pl = plan(ns)
    total = State(nq)
    per = pl["chunk"] * pl["chunks_per_group"]
    with np.errstate(over="ignore", under="ignore"):
        for g in range(pl["groups"]):
            s = State(nq)
            for j in range(g * per, min(ns, (g + 1) * per)):
                t = f[keep[j]]
                fold_face(s, points, v[t[0]], v[t[1]], v[t[2]])
            if g == 0:
                total = s
            else:
                total.touch = total.touch | s.touch
                total.rho = np.where(s.rho < total.rho, s.rho, total.rho)
                turn(total, np.ones(nq, dtype=bool), s.n, s.pr, s.pi)
    return {"turns": total.n.astype(np.int32), "p": np.stack([total.pr, total.pi], axis=1), "rho": total.rho,
            "touch": total.touch, "n_staged": int(ns)}


def result(turns, p, rho, touch, n_staged):
    """rule 8: (w, err)"""
    w = np.array([(float(n) * (math.pi / 2) + math.atan2(pi, pr)) / (2 * math.pi) for n, (pr, pi) in zip(turns, p)],
                 dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        err = float(n_staged) * (C1 + C2 / rho) * 2.0 ** -53
    return w, np.where(touch | (rho < RHO_MIN), np.inf, err)


def classify(w, err, threshold=0.5, two_sided=False):
    x = np.abs(w) if two_sided else w
    out = np.full(x.shape[0], -1, dtype=np.int8)
    out[x - err > threshold] = 1
    out[x + err < threshold] = 0
    return out


def winding(points, v, f, plan, threshold=0.5, two_sided=False):
    """everything mm.mesh_winding_number returns but the report"""
    r = fold(points, v, f, plan)
    r["w"], r["err"] = result(r["turns"], r["p"], r["rho"], r["touch"], r["n_staged"])
    r["inside"] = classify(r["w"], r["err"], threshold, two_sided)
    return r


def reference(points, v, f):
    """sum over the staged faces of atan2(num, den) / 2 pi in np.longdouble: independent of the bookkeeping"""
    ld = np.longdouble
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(ld)
    total = np.zeros(p.shape[0], dtype=ld)
    for i in staged_faces(v, f):
        a, b, c = (v[k].astype(ld)[None, :] - p for k in f[i])
        la, lb, lc = (np.sqrt((x * x).sum(axis=1)) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(axis=1)
        den = la * lb * lc + (a * b).sum(axis=1) * lc + (b * c).sum(axis=1) * la + (c * a).sum(axis=1) * lb
        total += np.arctan2(num, den)
    return total / (2 * np.arctan2(ld(0), ld(-1)))           # pi in long double


def first_run(mask, points):
    """(start, end, length) of the first maximal run of True, its segment lengths added in index order"""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return -1, -1, 0.0
    start = end = int(idx[0])
    while end + 1 < len(mask) and mask[end + 1]:
        end += 1
    length = 0.0
    for i in range(start, end):
        d = points[i + 1] - points[i]
        length += float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return start, end, length
