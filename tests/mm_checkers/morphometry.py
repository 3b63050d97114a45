"""Plain-Python restatement of the reference's lumen morphometry, the checker of mm_contour_measures and of the summaries
(multimoda_rs_amd/morphometry.py).  Scalar floats, math.sqrt (correctly rounded, like Rust's sqrt), math.atan2 (the C
library's, like Rust's f64::atan2; not np.arctan2) and sequential sums, in the order of:

  src/types/native.rs:27-39             distance_to, distance_2d_to
  src/types/native/contour.rs:227-361   find_farthest_points, find_closest_opposite, find_closest_opposite_3d,
                                        elliptic_ratio, area
  src/types/binding/py_geometry.rs:190-260       PyGeometry::get_summary
  src/types/binding/py_geometry_pair.rs:70-200   PyGeometryPair::get_summary / create_deformation_table

Where the reference panics these raise Panic.  `farthest_points_np` is the same fold vectorised (elementwise IEEE
products, sums and sqrt are exact in numpy as in Rust); the host suite checks it against the scalar loop.
"""
import math

import numpy as np

F64_MAX = 1.7976931348623157e308


class Panic(Exception):
    """Where the reference panics (an index out of bounds, an assert)."""


def fdiv(a, b):
    """IEEE 754 division, as in Rust (x / 0.0 is inf or NaN, not an exception)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _pts(p):
    return [tuple(float(v) for v in r) for r in np.asarray(p, dtype=np.float64).reshape(-1, 3)]


def dist3(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def dist2(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return math.sqrt(dx * dx + dy * dy)


def farthest_points(p):
    """contour.rs:227-242 -> ((i, j), distance)"""
    p = _pts(p)
    if not p:
        raise Panic("find_farthest_points: points[0] of an empty contour")
    best, pair = 0.0, (0, 0)
    for i in range(len(p)):
        for j in range(i + 1, len(p)):
            d = dist3(p[i], p[j])
            if d > best:
                best, pair = d, (i, j)
    return pair, best


def farthest_points_np(p):
    """farthest_points, vectorised: the first pair (i asc, j asc) of the largest distance above 0.0; NaN never wins."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        raise Panic("find_farthest_points: points[0] of an empty contour")
    i, j = np.triu_indices(n, 1)
    d = p[i] - p[j]
    s = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    with np.errstate(invalid="ignore"):
        ok = s > 0.0
    if not ok.any():
        return (0, 0), 0.0
    m = s[ok].max()
    k = int(np.argmax(s == m))
    return (int(i[k]), int(j[k])), float(m)


def closest_opposite_3d(p):
    """contour.rs:313-333 -> ((i, j), distance)"""
    p = _pts(p)
    n = len(p)
    if n <= 2:
        raise Panic("find_closest_opposite_3d: Need at least 3 points")
    half = n // 2
    best, pair = F64_MAX, (0, half)
    for i in range(n):
        j = (i + half) % n
        d = dist3(p[i], p[j])
        if d < best:
            best, pair = d, (i, j)
    return pair, best


def closest_opposite(p, centroid=None):
    """contour.rs:247-310 -> ((i, j), distance); the centre is `centroid` if given, else the mean of the points"""
    p = _pts(p)
    n = len(p)
    if n <= 2:
        raise Panic("find_closest_opposite: Need at least 3 points")
    if centroid is not None:
        cx, cy = float(centroid[0]), float(centroid[1])
    else:
        sx = sy = 0.0
        for q in p:
            sx += q[0]
            sy += q[1]
        cx, cy = fdiv(sx, float(n)), fdiv(sy, float(n))
    th = []
    for q in p:
        t = math.atan2(q[1] - cy, q[0] - cx)
        if t < 0.0:
            t += 2.0 * math.pi
        th.append(t)
    best, pair = F64_MAX, (0, 1)
    for i in range(n):
        bad, bj = F64_MAX, i
        for j in range(n):
            if j == i:
                continue
            delta = abs(th[j] - th[i])
            if delta > math.pi:
                delta = 2.0 * math.pi - delta
            diff = abs(delta - math.pi)
            if diff < bad:
                bad, bj = diff, j
        d = dist2(p[i], p[bj])
        if d < best:
            best, pair = d, (i, bj)
    return pair, best


def closest_opposite_np(p, centroid=None):
    """closest_opposite with the inner j loop vectorised (the angles still by math.atan2; |.|, subtraction and the
    strict first minimum are exact elementwise)."""
    q = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    if n <= 2:
        raise Panic("find_closest_opposite: Need at least 3 points")
    pts = _pts(q)
    if centroid is not None:
        cx, cy = float(centroid[0]), float(centroid[1])
    else:
        sx = sy = 0.0
        for r in pts:
            sx += r[0]
            sy += r[1]
        cx, cy = fdiv(sx, float(n)), fdiv(sy, float(n))
    th = []
    for r in pts:
        t = math.atan2(r[1] - cy, r[0] - cx)
        if t < 0.0:
            t += 2.0 * math.pi
        th.append(t)
    th = np.array(th)
    best, pair = F64_MAX, (0, 1)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            delta = np.abs(th - th[i])
            delta = np.where(delta > math.pi, 2.0 * math.pi - delta, delta)
            diff = np.abs(delta - math.pi)
            diff[i] = np.nan                                    # j == i is skipped
            ok = diff < F64_MAX
            bj = i
            if ok.any():
                m = diff[ok].min()
                bj = int(np.argmax(diff == m))
            d = dist2(pts[i], pts[bj])
            if d < best:
                best, pair = d, (i, bj)
    return pair, best


def elliptic_ratio(p, far=None):
    """contour.rs:335-343 (`far`: a farthest_points result to reuse)"""
    major = (far or farthest_points(p))[1]
    minor = closest_opposite_3d(p)[1]
    return fdiv(minor, major) if major < minor else fdiv(major, minor)


def area(p):
    """contour.rs:345-361"""
    p = _pts(p)
    n = len(p)
    if n < 3:
        return 0.0
    cx = cy = cz = 0.0
    for i in range(n):
        a, b = p[i], p[(i + 1) % n]
        cx += a[1] * b[2] - a[2] * b[1]
        cy += a[2] * b[0] - a[0] * b[2]
        cz += a[0] * b[1] - a[1] * b[0]
    return 0.5 * math.sqrt(cx * cx + cy * cy + cz * cz)


def _fmax(a, b):
    """f64::max: a NaN argument yields the other"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a <= b else b


def summary(areas, ratio_of, centroids):
    """PyGeometry::get_summary (py_geometry.rs:190-260).  ratio_of(k) -> the elliptic ratio of frame k, called in frame
    order only as far as Rust's all() gets (it may raise Panic)."""
    areas = [float(a) for a in areas]
    if not areas:
        return 0.0, 0.0, 0.0
    biggest = float("nan")
    for a in areas:
        biggest = _fmax(biggest, a)
    mla = float("inf")
    for a in areas:
        mla = _fmin(mla, a)
    max_stenosis = 1.0 - fdiv(mla, biggest) if biggest > 0.0 else 0.0
    all_elliptic = True
    for k in range(len(areas)):
        if not ratio_of(k) < 1.3:
            all_elliptic = False
            break
    threshold = 0.70 * biggest if all_elliptic else 0.50 * biggest
    cen = [tuple(float(v) for v in c) for c in centroids]
    longest, i = 0.0, 0
    while i < len(areas):
        if areas[i] < threshold:
            start = end = i
            while end + 1 < len(areas) and areas[end + 1] < threshold:
                end += 1
            run = 0.0
            for k in range(start, end):
                a, b = cen[k], cen[k + 1]
                dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
                run += math.sqrt(dx * dx + dy * dy + dz * dz)
            if run > longest:
                longest = run
            i = end + 1
        else:
            i += 1
    return mla, max_stenosis, longest


def _rust_f2(v):
    return "NaN" if v != v else "%.2f" % v


def deformation_table_text(ids, area_a, ellip_a, area_b, ellip_b, z,
                           headers=("id", "area_dia", "ellip_dia", "area_sys", "ellip_sys", "z")):
    """What create_deformation_table prints (py_geometry_pair.rs:127-196), print!/println! by print!/println!."""
    rows = [[str(int(ids[i]))] + [_rust_f2(float(c[i])) for c in (area_a, ellip_a, area_b, ellip_b, z)]
            for i in range(len(ids))]
    widths = [len(h) for h in headers]
    for row in rows:
        for k, cell in enumerate(row):
            widths[k] = max(widths[k], len(cell))
    out = []

    def border():
        out.append("+")
        for w in widths:
            out.append("-" * (w + 2) + "+")
        out.append("\n")

    border()
    out.append("|")
    for k, cell in enumerate(headers):
        total = widths[k] - len(cell)
        left = total // 2
        out.append(" " + " " * left + cell + " " * (total - left) + " |")
    out.append("\n")
    border()
    for row in rows:
        out.append("|")
        for k, cell in enumerate(row):
            out.append(" " + cell + " " * (widths[k] - len(cell)) + " |")
        out.append("\n")
    border()
    return "".join(out)


def geometry_summary(lumens, centroids, fast=True):
    """get_summary of a geometry given its lumen point arrays and frame centroids"""
    far = farthest_points_np if fast else farthest_points
    return summary([area(p) for p in lumens], lambda k: elliptic_ratio(lumens[k], far(lumens[k])), centroids)


def measures(p, centroid=None, closest_2d=True, fast=True):
    """Everything mm_contour_measures returns for one contour, with its NaN / (-1, -1) where the reference panics:
    dict(area, major, major_pair, minor_3d, minor_3d_pair, minor_2d, minor_2d_pair, elliptic_ratio)."""
    n = np.asarray(p).reshape(-1, 3).shape[0]
    nan = float("nan")
    out = {"area": area(p)}
    if n == 0:
        out["major"], out["major_pair"] = nan, (-1, -1)
    else:
        f = (farthest_points_np if fast else farthest_points)(p)
        out["major_pair"], out["major"] = f
    if n < 3:
        out.update(minor_3d=nan, minor_3d_pair=(-1, -1), minor_2d=nan, minor_2d_pair=(-1, -1), elliptic_ratio=nan)
        return out
    out["minor_3d_pair"], out["minor_3d"] = closest_opposite_3d(p)
    major, minor = out["major"], out["minor_3d"]
    out["elliptic_ratio"] = fdiv(minor, major) if major < minor else fdiv(major, minor)
    if closest_2d:
        out["minor_2d_pair"], out["minor_2d"] = (closest_opposite_np if fast else closest_opposite)(p, centroid)
    else:
        out["minor_2d"], out["minor_2d_pair"] = nan, (-1, -1)
    return out
