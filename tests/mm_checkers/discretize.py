"""Plain numpy / Python restatement of the reference's vessel discretisation (src/ccta/discretizing/{projecting,
resampling,vessel_tree}.rs and src/types/native/discretized_tree.rs), the parity reference of the discretisation tests.
Nothing here touches the device or the native library.  Float arithmetic is Python or elementwise numpy f64 in the
reference's operation order (numpy never fuses a multiply and an add); atan2 is math.atan2, which is the C library's,
as the reference's f64::atan2 is.  Centerlines are (xyz (n, 3), tangents (n, 3), branch ids (n,)) triples."""
from __future__ import annotations

import bisect
import math

import numpy as np


def p3(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def _dist(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _norm(a):
    return math.sqrt(_dot(a, a))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _div(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


# ---- projecting.rs --------------------------------------------------------------------------------------------------
def branch_cum_arc(pts):
    """:123-130"""
    cum = [0.0]
    for i in range(1, len(pts)):
        cum.append(cum[-1] + _dist(pts[i - 1], pts[i]))
    return cum


def build_sample_positions(total, step):
    """:132-146 (repeated addition, not k * step)"""
    pos, s = [], 0.0
    while s <= total + 1e-9:
        pos.append(s)
        s += step
    if pos and pos[-1] > total + 1e-6:
        pos[-1] = total
    return pos


def interpolate_branch_at_s(pts, tans, cum, target):
    """:148-200 -> (position, tangent).  binary_search_by on a sorted cum == upper_bound - 1."""
    seg = max(bisect.bisect_right(cum, target) - 1, 0)
    if seg >= len(pts) - 1:
        return tuple(pts[-1]), tuple(tans[-1])
    p0, p1 = pts[seg], pts[seg + 1]
    s0, s1 = cum[seg], cum[seg + 1]
    t = 0.0 if abs(s1 - s0) < 1e-12 else (target - s0) / (s1 - s0)
    n0, n1 = tans[seg], tans[seg + 1]
    tg = tuple(n0[k] * (1.0 - t) + n1[k] * t for k in range(3))
    nn = _norm(tg)
    if nn > 1e-12:
        tg = _div(tg, nn)
    return (p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1]), p0[2] + t * (p1[2] - p0[2])), tg


def anchors(cl_xyz, cl_tan, cl_branch, branch_id, step):
    """The anchors of walk_centerline_slices (:19-39) as an (M, 6) array: position, tangent."""
    xyz, tan = p3(cl_xyz), p3(cl_tan)
    sel = [i for i in range(xyz.shape[0]) if int(cl_branch[i]) == branch_id]
    if not sel:
        return np.zeros((0, 6))
    pts = [tuple(float(v) for v in xyz[i]) for i in sel]
    tans = [tuple(float(v) for v in tan[i]) for i in sel]
    cum = branch_cum_arc(pts)
    out = [sum(interpolate_branch_at_s(pts, tans, cum, s), ()) for s in build_sample_positions(cum[-1], step)]
    return np.array(out, dtype=np.float64).reshape(-1, 6)


def nearest_project(pts, anc):
    """voronoi_partition (:62-104) with project_to_plane (:106-118): (anchor index, projected point) per point, the
    min_by fold in anchor order (anchor j replaces the best iff best > d_j).  No anchor: index -1, the point itself."""
    p, a = p3(pts), np.asarray(anc, dtype=np.float64).reshape(-1, 6)
    n = p.shape[0]
    if a.shape[0] == 0:
        return np.full(n, -1, dtype=np.int32), p.copy()
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        best = None
        idx = np.zeros(n, dtype=np.int32)
        for j in range(a.shape[0]):
            dx, dy, dz = px - a[j, 0], py - a[j, 1], pz - a[j, 2]
            d = (dx * dx + dy * dy) + dz * dz
            if best is None:
                best = d
                continue
            m = best > d
            best = np.where(m, d, best)
            idx = np.where(m, np.int32(j), idx)
        c, nrm = a[idx, 0:3], a[idx, 3:6]
        s = ((px - c[:, 0]) * nrm[:, 0] + (py - c[:, 1]) * nrm[:, 1]) + (pz - c[:, 2]) * nrm[:, 2]
        q = np.stack([px - nrm[:, 0] * s, py - nrm[:, 1] * s, pz - nrm[:, 2] * s], axis=1)
    return idx, q


def walk_centerline_slices(cl_xyz, cl_tan, cl_branch, pts, branch_id, step):
    """:13-60 -> (anchors (M, 6), buckets: M lists of projected points in input order)"""
    anc = anchors(cl_xyz, cl_tan, cl_branch, branch_id, step)
    idx, q = nearest_project(pts, anc)
    buckets = [[] for _ in range(anc.shape[0])]
    for i in range(idx.shape[0]):
        if idx[i] >= 0:
            buckets[idx[i]].append(tuple(float(v) for v in q[i]))
    return anc, buckets


# ---- resampling.rs --------------------------------------------------------------------------------------------------
class PanicError(RuntimeError):
    """Where the reference panics (a NaN angle in the stable sort's partial_cmp().unwrap())."""


def local_basis(points, c):
    """:188-214"""
    u = None
    for p in points:
        off = _sub(p, c)
        l = _norm(off)
        if l > 1e-10:
            u = _div(off, l)
            break
    if u is None:
        return None
    for p in points:
        cr = _cross(u, _sub(p, c))
        l = _norm(cr)
        if l > 1e-10:
            nrm = _div(cr, l)
            w = _cross(nrm, u)
            return u, _div(w, _norm(w))
    return None


def has_full_angular_coverage(points, c):
    """:40-66"""
    if len(points) < 4 or c is None:
        return False
    b = local_basis(points, c)
    if b is None:
        return False
    u, v = b
    q = [False] * 4
    for p in points:
        off = _sub(p, c)
        pu, pv = _dot(off, u) >= 0.0, _dot(off, v) >= 0.0
        q[0 if (pu and pv) else 1 if pv else 2 if not pu else 3] = True
    return all(q)


def _catmull_rom(P, C, N, A, t):
    """:216-229 in the written order, vectorised over (segments, samples)"""
    t2 = t * t
    t3 = t2 * t
    return 0.5 * ((((2.0 * C) + (-P + N) * t) + ((((2.0 * P) - (5.0 * C)) + (4.0 * N)) - A) * t2) +
                  ((((-P) + (3.0 * C)) - (3.0 * N)) + A) * t3)


def resample_spline(points, c, n_points):
    """:69-160 -> (n_points, 3) array or None"""
    if n_points < 2 or len(points) < 3 or c is None:
        return None
    b = local_basis(points, c)
    if b is None:
        return None
    u, v = b
    ang = []
    for p in points:
        off = _sub(p, c)
        a = math.atan2(_dot(off, v), _dot(off, u))
        if math.isnan(a):
            raise PanicError("NaN angle")
        ang.append(a)
    order = sorted(range(len(points)), key=lambda i: ang[i])           # stable
    ctrl = np.array([points[i] for i in order], dtype=np.float64)
    n = ctrl.shape[0]
    P = ctrl[(np.arange(n) + n - 1) % n][:, None, :]
    C = ctrl[:, None, :]
    N = ctrl[(np.arange(n) + 1) % n][:, None, :]
    A = ctrl[(np.arange(n) + 2) % n][:, None, :]
    t = (np.arange(32, dtype=np.float64) / 32.0)[None, :, None]
    with np.errstate(all="ignore"):
        curve = _catmull_rom(P, C, N, A, t).reshape(-1, 3)
        curve = np.concatenate([curve, curve[:1]])
        d = curve[1:] - curve[:-1]
        seg_len = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    arc = [0.0]
    for x in seg_len.tolist():
        arc.append(arc[-1] + x)
    total = arc[-1]
    if total < 1e-10:
        return None
    step = total / n_points
    out = np.empty((n_points, 3))
    m = curve.shape[0]
    for i in range(n_points):
        target = i * step
        seg = min(max(bisect.bisect_left(arc, target) - 1, 0), m - 2)
        s0, s1 = arc[seg], arc[seg + 1]
        f = 0.0 if abs(s1 - s0) < 1e-12 else (target - s0) / (s1 - s0)
        out[i] = curve[seg] * (1.0 - f) + curve[seg + 1] * f
    return out


def create_uniform_contours(contours, n_points):
    """:11-37 on (id, centroid, points) triples -> [(id, centroid, (n_points, 3) array)]"""
    ne = [c for c in contours if len(c[2]) > 0]
    cov = [has_full_angular_coverage(c[2], c[1]) for c in ne]
    start = cov.index(True) if True in cov else 0
    end = len(cov) - cov[::-1].index(True) if True in cov else len(ne)
    out = []
    for cid, cen, pts in ne[start:end]:
        r = resample_spline(pts, cen, n_points)
        if r is not None:
            out.append((cid, cen, r))
    return out


def discretize_vessel(cl_xyz, cl_tan, cl_branch, pts, branch_id, step, n_points):
    """discretize_vessel_rs (discretizing.rs:13-22) -> [(id, centroid, (n_points, 3) array)]"""
    anc, buckets = walk_centerline_slices(cl_xyz, cl_tan, cl_branch, pts, branch_id, step)
    raw = [(k, tuple(float(v) for v in anc[k, 0:3]), buckets[k]) for k in range(anc.shape[0])]
    return create_uniform_contours(raw, n_points)


# ---- discretized_tree.rs:95-326 -------------------------------------------------------------------------------------
def _try_normalize(v):
    n = _norm(v)
    return _div(v, n) if n > 1e-12 else (0.0, 0.0, 1.0)


def _argmin_first(vals):
    best, k = None, None
    for i, x in enumerate(vals):
        if best is None or x < best:
            best, k = x, i
    return k


def _assign_cc_clock(p1, p2, centroid, normal, up):
    """:295-313"""
    dn = _dot(up, normal)
    w = (up[0] - normal[0] * dn, up[1] - normal[1] * dn, up[2] - normal[2] * dn)
    n = _norm(w)
    up_perp = _div(w, n) if n > 1e-12 else (0.0, 0.0, 0.0)
    right = _cross(up_perp, normal)
    return (p1, p2) if _dot(_sub(p1, centroid), right) < 0.0 else (p2, p1)


def _farthest(pts):
    best, pair = 0.0, (0, 0)
    for i in range(len(pts)):
        for j in range(i + 1, len(pts)):
            d = _dist(pts[i], pts[j])
            if d > best:
                best, pair = d, (i, j)
    return pair


def _closest_opposite(pts):
    n = len(pts)
    half = n // 2
    best, pair = float.fromhex("0x1.fffffffffffffp+1023"), (0, half)
    for i in range(n):
        j = (i + half) % n
        d = _dist(pts[i], pts[j])
        if d < best:
            best, pair = d, (i, j)
    return pair


def _tuples(a):
    return [tuple(float(v) for v in p) for p in np.asarray(a).reshape(-1, 3)]


def vessel_references(ao, main, branches):
    """:148-185 on (id, centroid, points) contours -> [(main_ref, counter_clock_ref, clock_ref)]"""
    mc = [tuple(c[1]) for c in main]
    up = _try_normalize(_sub(mc[0], ao))
    tagged = []
    first = _tuples(main[0][2])
    if len(first) > 2:                                                     # ostium_reference (:187-235)
        normal = _try_normalize(_sub(mc[1], mc[0])) if len(main) > 1 else _try_normalize(_sub(mc[0], ao))
        i, j = _closest_opposite(first)
        pa, pb = first[i], first[j]
        main_ref = pa if _norm(_sub(pa, ao)) <= _norm(_sub(pb, ao)) else pb
        i, j = _farthest(first)
        cc, cl = _assign_cc_clock(first[i], first[j], mc[0], normal, up)
        tagged.append((0, (main_ref, cc, cl)))
    for br in branches:                                                    # sidebranch_reference (:237-293)
        if not br:
            continue
        side = tuple(br[0][1])
        k = _argmin_first([_norm(_sub(m, side)) for m in mc])
        bc = mc[k]
        if k + 1 < len(main):
            normal = _try_normalize(_sub(mc[k + 1], bc))
        elif k > 0:
            normal = _try_normalize(_sub(bc, mc[k - 1]))
        else:
            normal = _try_normalize(_sub(bc, ao))
        pts = _tuples(main[k][2])
        n = len(pts)
        if n < 4:
            continue
        ci = _argmin_first([_norm(_sub(p, side)) for p in pts])
        q = n // 4
        cc, cl = _assign_cc_clock(pts[(ci + q) % n], pts[(ci + n - q) % n], bc, normal, up)
        tagged.append((k, (side, cc, cl)))
    tagged.sort(key=lambda x: x[0])                                        # stable
    return [r for _, r in tagged]


def calculate_ref_pts(aorta, rca, lca, rca_branches, lca_branches):
    """:95-145 -> (ao_rca, ao_lca, rca_references, lca_references); contours are (id, centroid, points)"""
    ao_rca = ao_lca = (0.0, 0.0, 0.0)
    rr, lr = [], []
    if aorta:
        for main, brs, side in ((rca, rca_branches, "r"), (lca, lca_branches, "l")):
            if not main:
                continue
            c0 = tuple(main[0][1])
            k = _argmin_first([_norm(_sub(tuple(a[1]), c0)) for a in aorta])
            ao = tuple(aorta[k][1])
            refs = vessel_references(ao, main, brs)
            if side == "r":
                ao_rca, rr = ao, refs
            else:
                ao_lca, lr = ao, refs
    return ao_rca, ao_lca, rr, lr
