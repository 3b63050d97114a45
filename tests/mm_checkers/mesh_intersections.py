"""Plain Python restatement of the mesh intersection check (include/mm_ccta.h, "mesh intersections"): the yardstick for
csrc/mm_isect_device.h, csrc/mm_intersect_kernels.hip and csrc/mm_intersect.cpp.  The box step is numpy over all faces;
the narrow phase runs pair by pair on Python floats, which are IEEE doubles and never fused, so every line below is one
rounding, in the header's order.

* `orient3d` / `orient2d`: the filtered signs (+1, -1, or 0 for "not certain").
* `pair_state`: the rule for two proper faces -> (state, coincident): DISJOINT, INTERSECTING or UNDECIDED.
* `scan` / `scan_two`: every pair of faces, unculled; per-face flags, the sorted pairs with their states, the counts.
* `predict_report`: the report integers that the items and the pair count decide.
"""
import numpy as np

DISJOINT, INTERSECTING, UNDECIDED = 0, 1, 2
CHUNK = 256
EPS = 2.0 ** -53
O3D_BOUND = (7.0 + 56.0 * EPS) * EPS            # o3derrboundA of the published predicate
O2D_BOUND = (3.0 + 16.0 * EPS) * EPS            # ccwerrboundA
TINY = 2.0 ** -900
INF = float("inf")


def orient3d(a, b, c, d):
    """The sign of det[a - d; b - d; c - d] where the stage-A bound proves it, else 0."""
    adx, bdx, cdx = a[0] - d[0], b[0] - d[0], c[0] - d[0]
    ady, bdy, cdy = a[1] - d[1], b[1] - d[1], c[1] - d[1]
    adz, bdz, cdz = a[2] - d[2], b[2] - d[2], c[2] - d[2]
    bdxcdy, cdxbdy = bdx * cdy, cdx * bdy
    cdxady, adxcdy = cdx * ady, adx * cdy
    adxbdy, bdxady = adx * bdy, bdx * ady
    det = (adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy)) + cdz * (adxbdy - bdxady)
    perm = (((abs(bdxcdy) + abs(cdxbdy)) * abs(adz) + (abs(cdxady) + abs(adxcdy)) * abs(bdz))
            + (abs(adxbdy) + abs(bdxady)) * abs(cdz))
    if not (perm < INF) or perm < TINY:
        return 0
    bound = O3D_BOUND * perm
    return 1 if det > bound else (-1 if -det > bound else 0)


def orient2d(a, b, c):
    """The sign of det[a - c; b - c] (2-D points) where the stage-A bound proves it, else 0."""
    left = (a[0] - c[0]) * (b[1] - c[1])
    right = (a[1] - c[1]) * (b[0] - c[0])
    det = left - right
    detsum = abs(left) + abs(right)
    if not (detsum < INF) or detsum < TINY:
        return 0
    bound = O2D_BOUND * detsum
    return 1 if det > bound else (-1 if -det > bound else 0)


def dominant_axis(p, q, r):
    """The axis of the largest |component| of (q - p) x (r - p), the first of equal ones."""
    ux, uy, uz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
    vx, vy, vz = r[0] - p[0], r[1] - p[1], r[2] - p[2]
    n = (abs(uy * vz - uz * vy), abs(uz * vx - ux * vz), abs(ux * vy - uy * vx))
    ax = 0
    if n[1] > n[ax]:
        ax = 1
    if n[2] > n[ax]:
        ax = 2
    return ax


def drop(p, ax):
    return (p[1] if ax == 0 else p[0], p[1] if ax == 2 else p[2])


def _separated_2d(t, u):
    """An edge of the 2-D triangle t with all corners of u certainly on its outer side."""
    for k in range(3):
        a, b, c = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
        inner = orient2d(a, b, c)
        if inner == 0:
            continue
        if orient2d(a, b, u[0]) == -inner and orient2d(a, b, u[1]) == -inner and orient2d(a, b, u[2]) == -inner:
            return True
    return False


def _rot(t, k):
    return (t[k], t[(k + 1) % 3], t[(k + 2) % 3])


def _lone(s):
    """Three certain signs, not all equal: the index of the one that differs from the other two."""
    return 0 if s[1] == s[2] else (1 if s[0] == s[2] else 2)


def _no_shared(t1, t2):
    s2 = (orient3d(t1[0], t1[1], t1[2], t2[0]), orient3d(t1[0], t1[1], t1[2], t2[1]), orient3d(t1[0], t1[1], t1[2], t2[2]))
    if s2[0] != 0 and s2[0] == s2[1] == s2[2]:
        return DISJOINT
    s1 = (orient3d(t2[0], t2[1], t2[2], t1[0]), orient3d(t2[0], t2[1], t2[2], t1[1]), orient3d(t2[0], t2[1], t2[2], t1[2]))
    if s1[0] != 0 and s1[0] == s1[1] == s1[2]:
        return DISJOINT
    if s1 == (0, 0, 0) and s2 == (0, 0, 0):                               # nearly coplanar
        ax = dominant_axis(*t1)
        a = tuple(drop(p, ax) for p in t1)
        b = tuple(drop(p, ax) for p in t2)
        return DISJOINT if _separated_2d(a, b) or _separated_2d(b, a) else UNDECIDED
    if 0 in s1 or 0 in s2:
        return UNDECIDED
    k1, k2 = _lone(s1), _lone(s2)
    p1, q1, r1 = _rot(t1, k1)
    p2, q2, r2 = _rot(t2, k2)
    if s1[k1] < 0:
        q2, r2 = r2, q2
    if s2[k2] < 0:
        q1, r1 = r1, q1
    e1 = orient3d(p1, q1, p2, q2)
    if e1 > 0:
        return DISJOINT
    e2 = orient3d(p1, r1, r2, p2)
    if e2 > 0:
        return DISJOINT
    return INTERSECTING if e1 < 0 and e2 < 0 else UNDECIDED


def _edge_against(q, r, sq, sr, t):
    """The segment q r (plane signs sq, sr against t) and the triangle t: (certainly crossing, certainly missing)."""
    e = (orient3d(q, r, t[0], t[1]), orient3d(q, r, t[1], t[2]), orient3d(q, r, t[2], t[0]))
    crossing = sq != 0 and sr == -sq and e[0] != 0 and e[0] == e[1] == e[2]
    missing = (1 in e) and (-1 in e)
    return crossing, missing


def _wedge_separates(a, b, c, u1, u2):
    """The edge a b of the 2-D triangle (a, b, c) with u1 and u2 certainly on its outer side."""
    inner = orient2d(a, b, c)
    return inner != 0 and orient2d(a, b, u1) == -inner and orient2d(a, b, u2) == -inner


def _one_shared(t1, t2, k1, k2):
    p1, q1, r1 = _rot(t1, k1)
    p2, q2, r2 = _rot(t2, k2)
    a1, b1 = orient3d(p2, q2, r2, q1), orient3d(p2, q2, r2, r1)
    if a1 != 0 and a1 == b1:
        return DISJOINT
    a2, b2 = orient3d(p1, q1, r1, q2), orient3d(p1, q1, r1, r2)
    if a2 != 0 and a2 == b2:
        return DISJOINT
    cross1, miss1 = _edge_against(q1, r1, a1, b1, (p2, q2, r2))
    if cross1:
        return INTERSECTING
    cross2, miss2 = _edge_against(q2, r2, a2, b2, (p1, q1, r1))
    if cross2:
        return INTERSECTING
    if miss1 and miss2:
        return DISJOINT
    if (a1, b1, a2, b2) != (0, 0, 0, 0):
        return UNDECIDED
    ax = dominant_axis(p1, q1, r1)                                        # nearly coplanar: the edges at the shared vertex
    s0, s1, s2 = drop(p1, ax), drop(q1, ax), drop(r1, ax)
    t0, t1, t2 = drop(p2, ax), drop(q2, ax), drop(r2, ax)
    if (_wedge_separates(s0, s1, s2, t1, t2) or _wedge_separates(s2, s0, s1, t1, t2)
            or _wedge_separates(t0, t1, t2, s1, s2) or _wedge_separates(t2, t0, t1, s1, s2)):
        return DISJOINT
    return UNDECIDED


def _two_shared(t1, t2, k1, k2):
    """k1, k2: the corner of each face that the other does not have."""
    c1, a, b = _rot(t1, k1)
    c2 = t2[k2]
    if orient3d(t1[0], t1[1], t1[2], c2) != 0 or orient3d(t2[0], t2[1], t2[2], c1) != 0:
        return DISJOINT
    ax = dominant_axis(*t1)
    a2, b2 = drop(a, ax), drop(b, ax)
    s1, s2 = orient2d(a2, b2, drop(c1, ax)), orient2d(a2, b2, drop(c2, ax))
    return DISJOINT if s1 != 0 and s2 == -s1 else UNDECIDED


def pair_state(t1, t2, id1=(0, 1, 2), id2=(3, 4, 5)):
    """(state, coincident) of two proper faces: corners as 3-tuples of floats, ids the canonical vertex ids.  In the self
    form t1 is the face with the lower index."""
    in2 = [k for k in range(3) if id1[k] in id2]
    in1 = [k for k in range(3) if id2[k] in id1]
    if len(in2) == 0:
        return _no_shared(t1, t2), False
    if len(in2) == 1:
        return _one_shared(t1, t2, in2[0], in1[0]), False
    if len(in2) == 2:
        return _two_shared(t1, t2, 3 - in2[0] - in2[1], 3 - in1[0] - in1[1]), False
    return INTERSECTING, True


def canonical_ids(vertices):
    """Per vertex the lowest index with equal coordinates (+0.0 == -0.0)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3) + 0.0
    ids = np.arange(len(v), dtype=np.int64)
    if len(v) == 0:
        return ids
    order = np.lexsort((ids, v[:, 2], v[:, 1], v[:, 0]))
    s = v[order]
    new = np.ones(len(v), dtype=bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    first = np.maximum.accumulate(np.where(new, np.arange(len(v)), 0))
    ids[order] = order[first]
    return ids


def is_degenerate(v, ids):
    i, j, k = (int(x) for x in ids)
    if i == j or j == k or i == k:
        return True
    ab, ac = v[1] - v[0], v[2] - v[0]
    n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    return n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0


def _arrays(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v, f


def _prepare(v, f, ids):
    tri = v[f].reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        deg = np.array([is_degenerate(tri[k], ids[k]) for k in range(len(f))], dtype=bool)
    lo = tri.min(axis=1) if len(f) else np.zeros((0, 3))
    hi = tri.max(axis=1) if len(f) else np.zeros((0, 3))
    tup = [tuple(tuple(float(x) for x in p) for p in t) for t in tri]
    return deg, lo, hi, tup


def _collect(na, nb, found, narrow, n_deg, self_form):
    found.sort()
    state_a, state_b = np.zeros(na, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
    for i, j, s, _ in found:
        state_a[i] |= s
        (state_a if self_form else state_b)[j] |= s
    out = {"pairs": np.array([(i, j) for i, j, _, _ in found], dtype=np.int64).reshape(-1, 2),
           "pair_state": np.array([s for _, _, s, _ in found], dtype=np.int8),
           "n_intersecting_pairs": sum(s == INTERSECTING for _, _, s, _ in found),
           "n_undecided_pairs": sum(s == UNDECIDED for _, _, s, _ in found),
           "n_coincident_pairs": sum(c for _, _, _, c in found), "n_degenerate_faces": n_deg, "narrow_tests": narrow}
    if self_form:
        out["face_state"] = state_a
    else:
        out["face_state"] = (state_a, state_b)
    return out


def scan(vertices, faces):
    """The self form, every pair i < j, unculled."""
    v, f = _arrays(vertices, faces)
    ids = canonical_ids(v)[f]
    deg, lo, hi, tup = _prepare(v, f, ids)
    found, narrow = [], 0
    idt = [tuple(int(x) for x in r) for r in ids]
    for i in range(len(f)):
        if deg[i]:
            continue
        near = np.flatnonzero(((lo[i + 1:] <= hi[i]) & (lo[i] <= hi[i + 1:])).all(axis=1) & ~deg[i + 1:]) + i + 1
        for j in near.tolist():
            narrow += 1
            s, c = pair_state(tup[i], tup[j], idt[i], idt[j])
            if s != DISJOINT:
                found.append((i, j, s, c))
    return _collect(len(f), 0, found, narrow, int(deg.sum()), True)


def scan_two(va, fa, vb, fb):
    """The two-mesh form, every face of a against every face of b, unculled; no vertex identities."""
    va, fa = _arrays(va, fa)
    vb, fb = _arrays(vb, fb)
    dega, loa, hia, tupa = _prepare(va, fa, fa)
    degb, lob, hib, tupb = _prepare(vb, fb, fb)
    found, narrow = [], 0
    for i in range(len(fa)):
        if dega[i]:
            continue
        near = np.flatnonzero(((lob <= hia[i]) & (loa[i] <= hib)).all(axis=1) & ~degb) if len(fb) else np.zeros(0, int)
        for j in near.tolist():
            narrow += 1
            s, c = pair_state(tupa[i], tupb[j])
            if s != DISJOINT:
                found.append((i, j, s, c))
    return _collect(len(fa), len(fb), found, narrow, int(dega.sum() + degb.sum()), False)


def up256(n):
    return (n + 255) // 256 * 256


def predict_report(nfa, nfb, items, n_pairs, max_pairs, self_form):
    """The report integers that follow from the sizes, the number of items the plan made and the number of pairs found:
    the chunk pairs before culling; two launches (the clear, the pairs) where there is an item; the uploads (staged faces
    of 96 bytes, items of 8) and the downloads (a flag byte per staged face, eight counters, the pair records of 8 bytes
    where they do not exceed the cap)."""
    nca, ncb = -(-nfa // CHUNK), -(-nfb // CHUNK)
    total = nca * (nca + 1) // 2 if self_form else nca * ncb
    if items == 0:
        return dict(items_total=total, n_launches=0, bytes_uploaded=0, bytes_downloaded=0, pairs_complete=1)
    return dict(items_total=total, n_launches=2, bytes_uploaded=up256(96 * (nfa + nfb)) + up256(8 * items),
                bytes_downloaded=up256(nfa + nfb) + 256 + (8 * n_pairs if n_pairs <= max_pairs else 0),
                pairs_complete=int(n_pairs <= max_pairs))
