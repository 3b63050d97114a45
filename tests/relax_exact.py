"""An oracle for the mesh relaxation (include/mm_ccta.h, "mesh relaxation") that shares no arithmetic with the rule: plain
Python over fractions.Fraction, built from the f64 inputs and outputs.  It imports neither checker.

* `dist2_exact`: the exact squared distance of a point from a closed triangle -- the foot of the perpendicular where it
  falls inside, else the nearest of the three edges; a triangle without area counts as its edges.  No region tests in
  Ericson's order, no divisions before the last one.
* `nearest_exact`: the exact minimum over a mesh and the lowest face index that attains it.  Only the faces a prefilter
  in f64 cannot rule out are evaluated exactly.  The prefilter: the distance s to a face's boundary (three clamped
  segment projections, well conditioned on any face) and r, an upper bound of the face's inradius.  Where the closest
  point is interior, s^2 = d^2 + (its distance from the boundary)^2 <= d^2 + r^2, so s - r <= d <= s for every face; a
  face is kept unless s - r - tol > min s + tol, `tol` covering the f64 roundings of s and r.
* `grid_step_exact`: one iteration on a planar mesh that is its own reference, where everything up to the projection is
  exact in f64: the candidates x + lambda (mean of the neighbours - x), the exact sign of dot(m_old, m_new) per face, the
  vertices the guard takes back and the exact count of flipped faces.
"""
from fractions import Fraction

import numpy as np


def fr(p):
    """A point as three Fractions (an f64 is a rational; nothing is rounded)."""
    return tuple(x if isinstance(x, Fraction) else Fraction(float(x)) for x in p)


def sub(u, w):
    return (u[0] - w[0], u[1] - w[1], u[2] - w[2])


def dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def segment_d2(p, u, w):
    e, d = sub(w, u), sub(p, u)
    l = dot(e, e)
    if l == 0:
        return dot(d, d)
    t = dot(d, e)
    if t <= 0:
        return dot(d, d)
    if t >= l:
        d = sub(p, w)
        return dot(d, d)
    return dot(d, d) - t * t / l                                          # Pythagoras; one division


def dist2_exact(p, a, b, c):
    """The exact squared distance from p to the closed triangle (a, b, c); points as f64 triples or Fractions."""
    p, a, b, c = fr(p), fr(a), fr(b), fr(c)
    ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
    n = cross(ab, ac)
    nn = dot(n, n)
    if nn != 0:
        wc, wb = dot(cross(ab, ap), n), dot(cross(ap, ac), n)              # barycentric weights of c and b, times nn
        if wb >= 0 and wc >= 0 and wb + wc <= nn:
            h = dot(ap, n)
            return h * h / nn
    return min(segment_d2(p, a, b), segment_d2(p, b, c), segment_d2(p, c, a))


def _segment_distance(p, u, w):
    e = w - u
    l = (e * e).sum(axis=1)
    t = np.clip(((p - u) * e).sum(axis=1) / np.where(l > 0.0, l, 1.0), 0.0, 1.0)
    d = p - (u + e * t[:, None])
    return np.sqrt((d * d).sum(axis=1))


def nearest_exact(p, rv, rf, tol):
    """(exact minimum d2, the lowest face that attains it, {face: exact d2} of the faces evaluated)."""
    rv, rf = np.asarray(rv, dtype=np.float64).reshape(-1, 3), np.asarray(rf, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64)
    a, b, c = rv[rf[:, 0]], rv[rf[:, 1]], rv[rf[:, 2]]
    with np.errstate(all="ignore"):
        s = np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
        n = np.cross(b - a, c - a)
        per = np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - b, axis=1) + np.linalg.norm(a - c, axis=1)
        r = np.where(per > 0.0, np.linalg.norm(n, axis=1) / np.where(per > 0.0, per, 1.0), 0.0) * (1.0 + 1e-9)
        ruled_out = s - r - tol > np.nanmin(s) + tol                      # a NaN or an overflow rules nothing out
    keep = np.flatnonzero(~ruled_out)
    assert len(keep) > 0, "the prefilter kept no face"
    fp = fr(p)
    exact = {int(k): dist2_exact(fp, a[k], b[k], c[k]) for k in keep}
    best = min(exact.values())
    return best, min(k for k, d in exact.items() if d == best), exact


def neighbours(f, nv):
    nb = [set() for _ in range(nv)]
    for t in np.asarray(f, dtype=np.int64).reshape(-1, 3):
        for i in range(3):
            u, w = int(t[i]), int(t[(i + 1) % 3])
            if u != w:
                nb[u].add(w)
                nb[w].add(u)
    return nb


def _normals(x, f):
    return [cross(sub(x[j], x[i]), sub(x[k], x[i])) for i, j, k in f]


def grid_step_exact(v, f, free, lamb):
    """One iteration from the positions v (already on the planar reference, so step 0 changes nothing) with every
    candidate inside the reference, where the projection is the identity: returns
    (candidates {vertex: exact point}, the set of reverted vertices, the exact number of flipped faces, the smallest
    |dot(m_old, m_new)| over the faces relative to dot(m_old, m_old) -- how far every sign is from undecided)."""
    f = [tuple(int(i) for i in t) for t in np.asarray(f, dtype=np.int64).reshape(-1, 3)]
    free = np.asarray(free, dtype=bool)
    x = [fr(p) for p in np.asarray(v, dtype=np.float64).reshape(-1, 3)]
    nb = neighbours(f, len(x))
    lam = Fraction(float(lamb))
    cand, new = {}, list(x)
    for i in np.flatnonzero(free):
        i = int(i)
        mean = tuple(sum(x[j][a] for j in nb[i]) / len(nb[i]) for a in range(3))
        cand[i] = new[i] = tuple(x[i][a] + lam * (mean[a] - x[i][a]) for a in range(3))
    m_old, m_new = _normals(x, f), _normals(new, f)
    reverted, margin = set(), None
    for t, mo, mn in zip(f, m_old, m_new):
        if len(set(t)) < 3 or dot(mo, mo) == 0:
            continue
        s = dot(mo, mn)
        rel = abs(s) / dot(mo, mo)
        margin = rel if margin is None else min(margin, rel)
        if not s > 0:
            reverted.update(i for i in t if free[i])
    final = [x[i] if i in reverted else new[i] for i in range(len(x))]
    flipped = sum(1 for t, mi, mf in zip(f, m_old, _normals(final, f))
                  if len(set(t)) == 3 and dot(mi, mi) > 0 and dot(mi, mf) <= 0)
    return cand, reverted, flipped, margin
