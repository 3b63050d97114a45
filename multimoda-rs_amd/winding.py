"""Winding numbers: which side of a surface a point lies on.

The generalized winding number (Jacobson et al. 2013) of a triangle mesh at query points, ``w(p) = (1 / 4 pi) sum_f
Omega_f(p)``: 1 inside and 0 outside a closed mesh of positive volume (as ``fix_mesh_winding`` leaves it), a smooth
fraction near the openings of an open mesh -- a CCTA aorta is open where the scan was cropped -- where ``w > 1/2`` stays a
sound "inside".  On it rest the point-in-mesh test, the signed surface distance, the mesh-in-mesh containment report and
the intramural course of a centerline, the reference's open roadmap items "write a more stable function to find
intramural points on aorta" and "intramural length etc. from the CCTA mesh".

The rule is include/mm_ccta.h, "winding number", restated in tests/mm_checkers/winding_number.py: every face is folded on
the device in exact-order f64 without atan2 (csrc/mm_winding_kernels.hip); ``w`` and its error bound ``err`` are
computed on the host from the device's quarter turns and complex remainder.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N
from .ccta import _engine, _p3
from .surface import PointMeshDistance, _finite, _mesh_arrays, _point_mesh, sample_mesh_surface

WINDING_REPORT_KEYS = ("n_staged_faces", "n_degenerate_faces", "chunk_faces", "chunks_per_group", "groups", "items",
                       "n_launches", "bytes_uploaded", "bytes_downloaded", "bytes_scratch")
MAX_COORDINATE = 2.0 ** 300

INSIDE, OUTSIDE, UNDECIDED = 1, 0, -1


@dataclass
class WindingNumber:
    """Per query: the winding number ``w``, the proven bound ``err`` on its distance from the exact value for these f64
    inputs (inf where the query touches a face or lies on an edge or vertex), ``inside`` (int8: 1 inside, 0 outside, -1
    undecided), and what the device returned: ``turns`` quarter turns, the complex remainder ``p`` (n, 2), ``rho`` (how
    far the query stays from every face's edges and corners, relative to the face) and ``touch``.
    ``report``: WINDING_REPORT_KEYS."""
    w: np.ndarray
    err: np.ndarray
    inside: np.ndarray
    turns: np.ndarray
    p: np.ndarray
    rho: np.ndarray
    touch: np.ndarray
    report: dict


@dataclass
class SignedPointMeshDistance(PointMeshDistance):
    """``PointMeshDistance`` plus ``sign`` (int8: -1 inside, +1 outside, 0 undecided), ``signed_distance`` = ``sign *
    distance`` (NaN where undecided) and the ``winding`` result the sign comes from."""
    sign: np.ndarray
    signed_distance: np.ndarray
    winding: WindingNumber


@dataclass
class ContainmentExtreme:
    """One sample of ``mesh_containment``: its index (-1: none), the face of the sampled mesh it lies on, its
    ``distance`` from the other mesh (NaN: none), the nearest ``face`` there and the ``closest`` point on it."""
    sample: int
    sample_face: int
    distance: float
    face: int
    closest: np.ndarray


@dataclass
class ContainmentReport:
    """``mesh_containment``: the samples of mesh_a ``n_inside``, ``n_outside`` and ``n_undecided`` of mesh_b;
    ``worst_outside`` the outside sample farthest from mesh_b, ``deepest_inside`` the inside sample farthest from it (the
    lowest sample index on ties); ``contained``: no sample outside and none undecided.  ``inside`` and ``distance`` are
    per sample."""
    n_samples: int
    n_inside: int
    n_outside: int
    n_undecided: int
    contained: bool
    worst_outside: ContainmentExtreme
    deepest_inside: ContainmentExtreme
    inside: np.ndarray
    distance: np.ndarray
    winding: WindingNumber


@dataclass
class IntramuralPoints:
    """``mask``: decided inside the wall surface and decided not inside the lumen surface; ``undecided``: either
    classification is -1; the two ``WindingNumber`` results."""
    mask: np.ndarray
    undecided: np.ndarray
    lumen: WindingNumber
    wall: WindingNumber


@dataclass
class IntramuralCourse:
    """``intramural`` per centerline point; ``start`` .. ``end`` (inclusive) the first maximal run of consecutive
    intramural points and ``length`` the sum of that run's segment lengths in index order; -1, -1 and 0.0 without one."""
    intramural: np.ndarray
    start: int
    end: int
    length: float
    points: IntramuralPoints


def _checked(points, mesh):
    v, f = _mesh_arrays(mesh)
    q = _p3(points)
    for a, what in ((v, "mesh vertices"), (q, "points")):
        _finite(a, what)
        if a.size and np.abs(a).max() > MAX_COORDINATE:
            raise ValueError(f"{what} must not exceed 2^300 in magnitude")
    return q, v, f


def _threshold(threshold) -> float:
    t = float(threshold)
    if not np.isfinite(t):
        raise ValueError("threshold must be finite")
    return t


def winding_plan(n_staged: int) -> dict:
    """TEST HOOK (``mm_winding_plan``; host only): the grouping for ``n_staged`` staged faces."""
    info = np.zeros(4, dtype=np.int64)
    N.check(N.lib().mm_winding_plan(int(n_staged), N._ptr(info)), "winding_plan")
    return {"chunk": int(info[0]), "chunks_per_group": int(info[1]), "groups": int(info[2]), "n_staged": int(info[3])}


def _raw_arrays(nq: int):
    return (np.zeros(nq, dtype=np.int32), np.zeros((nq, 2), dtype=np.float64), np.zeros(nq, dtype=np.float64),
            np.zeros(nq, dtype=np.uint8))


def winding_fold_host(points, mesh) -> dict:
    """TEST HOOK (``mm_winding_fold_host``; host only): ``turns``, ``p``, ``rho``, ``touch`` and ``n_staged`` by the
    arithmetic the kernels run, on the CPU."""
    q, v, f = _checked(points, mesh)
    n, p, rho, touch = _raw_arrays(q.shape[0])
    staged = np.zeros(1, dtype=np.int64)
    N.check(N.lib().mm_winding_fold_host(N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(q), q.shape[0], N._ptr(n),
                                         N._ptr(p), N._ptr(rho), N._ptr(touch), N._ptr(staged)), "winding_fold_host")
    return {"turns": n, "p": p, "rho": rho, "touch": touch.astype(bool), "n_staged": int(staged[0])}


def winding_result(turns, p, rho, touch, n_staged: int):
    """``(w, err)`` of rule 8 (``mm_winding_result``; host only)."""
    n = np.ascontiguousarray(turns, dtype=np.int32)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    touch = np.ascontiguousarray(touch, dtype=np.uint8)
    w, err = np.zeros(n.shape[0], dtype=np.float64), np.zeros(n.shape[0], dtype=np.float64)
    N.check(N.lib().mm_winding_result(N._ptr(n), N._ptr(p), N._ptr(rho), N._ptr(touch), n.shape[0], int(n_staged), N._ptr(w),
                                      N._ptr(err)), "winding_result")
    return w, err


def classify(w: np.ndarray, err: np.ndarray, threshold: float = 0.5, two_sided: bool = False) -> np.ndarray:
    """int8 per query: 1 where ``w - err > threshold``, 0 where ``w + err < threshold``, -1 otherwise; ``two_sided``
    classifies ``|w|``, for meshes whose orientation is unknown."""
    x = np.abs(w) if two_sided else w
    out = np.full(x.shape[0], UNDECIDED, dtype=np.int8)
    out[x - err > threshold] = INSIDE
    out[x + err < threshold] = OUTSIDE
    return out


def _winding(q: np.ndarray, v: np.ndarray, f: np.ndarray, threshold: float, two_sided: bool, engine) -> WindingNumber:
    nq = q.shape[0]
    n, p, rho, touch = _raw_arrays(nq)
    rep = N.MMWindingReport()
    N.check(N.lib().mm_mesh_winding(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(q), nq,
                                    N._ptr(n), N._ptr(p), N._ptr(rho), N._ptr(touch), C.byref(rep)), "mesh_winding_number")
    report = {k: int(getattr(rep, k)) for k in WINDING_REPORT_KEYS}
    w, err = winding_result(n, p, rho, touch, report["n_staged_faces"])
    return WindingNumber(w, err, classify(w, err, threshold, two_sided), n, p, rho, touch.astype(bool), report)


def mesh_winding_number(points, mesh, *, threshold: float = 0.5, two_sided: bool = False,
                        engine: Optional[N.Engine] = None) -> WindingNumber:
    """The generalized winding number of ``mesh`` -- a ``(vertices, faces)`` pair, an object with ``.vertices`` /
    ``.faces``, or a results dict with ``"mesh"`` -- at every one of ``points`` (n, 3): ``WindingNumber``.  On a closed
    mesh of positive volume ``w`` is 1 inside and 0 outside; an inward-oriented one gives -1 inside (``two_sided=True``
    classifies ``|w|``); on an open mesh ``w`` is a fraction and ``w > threshold`` the "inside".  ``inside`` is decided
    only where the proven ``err`` allows it.  Faces without area are ignored.  The result has one bit pattern whatever
    the scheduling and whichever other points share the call.  A mesh without a face gives ``w = 0``, ``err = 0``,
    outside.  Cost is points x faces.  Non-finite coordinates, coordinates above 2^300 and face indices out of range
    raise ValueError."""
    q, v, f = _checked(points, mesh)
    return _winding(q, v, f, _threshold(threshold), bool(two_sided), engine)


def points_in_mesh(points, mesh, *, threshold: float = 0.5, two_sided: bool = False,
                   engine: Optional[N.Engine] = None) -> np.ndarray:
    """``mesh_winding_number(...).inside``: int8 per point, 1 inside, 0 outside, -1 undecided (on the surface, or closer
    to an edge than the arithmetic can tell)."""
    return mesh_winding_number(points, mesh, threshold=threshold, two_sided=two_sided, engine=engine).inside


def _signed(q, v, f, threshold, two_sided, eng) -> SignedPointMeshDistance:
    d = _point_mesh(q, v, f, eng)
    wn = _winding(q, v, f, threshold, two_sided, eng)
    sign = np.where(wn.inside == INSIDE, -1, np.where(wn.inside == OUTSIDE, 1, 0)).astype(np.int8)
    signed = np.where(sign == 0, np.nan, sign * d.distance)
    return SignedPointMeshDistance(d.distance, d.sq_distance, d.face, d.closest, d.region, d.report, sign, signed, wn)


def signed_point_mesh_distance(points, mesh, *, threshold: float = 0.5, two_sided: bool = False,
                               engine: Optional[N.Engine] = None) -> SignedPointMeshDistance:
    """``point_mesh_distance`` and ``mesh_winding_number`` on one engine: the ``PointMeshDistance`` fields plus ``sign``
    (-1 inside, +1 outside, 0 undecided) and ``signed_distance`` = ``sign * distance`` (NaN where undecided)."""
    q, v, f = _checked(points, mesh)
    return _signed(q, v, f, _threshold(threshold), bool(two_sided), _engine(engine))


def _extreme(mask: np.ndarray, d: PointMeshDistance, owner: np.ndarray) -> ContainmentExtreme:
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return ContainmentExtreme(-1, -1, float("nan"), -1, np.full(3, np.nan))
    k = int(idx[np.argmax(d.sq_distance[idx])])             # the first of the largest
    return ContainmentExtreme(k, int(owner[k]), float(d.distance[k]), int(d.face[k]), d.closest[k].copy())


def mesh_containment(mesh_a, mesh_b, *, samples: int = 1, threshold: float = 0.5, two_sided: bool = False,
                     engine: Optional[N.Engine] = None) -> ContainmentReport:
    """Does ``mesh_b`` enclose ``mesh_a``, and if not, where and by how much: the ``sample_mesh_surface(mesh_a,
    samples)`` points tested against ``mesh_b`` -- ``ContainmentReport`` with the counts inside, outside and undecided,
    the outside sample farthest from ``mesh_b`` and the deepest inside sample, each with its face of ``mesh_a``, the
    nearest face of ``mesh_b`` and the closest point on it.  A lumen that lies wholly outside its wall has no crossing
    for ``mesh_intersections`` to find; here every sample of it is outside."""
    va, fa = _mesh_arrays(mesh_a)
    pts, owner = sample_mesh_surface((va, fa), samples)
    q, vb, fb = _checked(pts, mesh_b)
    s = _signed(q, vb, fb, _threshold(threshold), bool(two_sided), _engine(engine))
    inside, outside = s.winding.inside == INSIDE, s.winding.inside == OUTSIDE
    n_in, n_out = int(inside.sum()), int(outside.sum())
    n_und = q.shape[0] - n_in - n_out
    return ContainmentReport(q.shape[0], n_in, n_out, n_und, n_out == 0 and n_und == 0, _extreme(outside, s, owner),
                             _extreme(inside, s, owner), s.winding.inside, s.distance, s.winding)


def intramural_points(points, aortic_lumen_mesh, aortic_wall_mesh, *, threshold: float = 0.5, two_sided: bool = False,
                      engine: Optional[N.Engine] = None) -> IntramuralPoints:
    """Which of ``points`` (a coronary's centerline or vertices) lie inside the aortic wall: decided inside the wall's
    outer surface and decided not inside the lumen surface.  The two surfaces of a labelled result come from
    ``keep_labeled_points_from_mesh`` (the aortic vertices), ``manual_hole_fill`` (the ostia the cut leaves) and the
    aortic part of ``create_wall_mesh`` (the outer surface); they may stay open where the scan was cropped."""
    t = _threshold(threshold)
    q, vl, fl = _checked(points, aortic_lumen_mesh)
    _, vw, fw = _checked(q, aortic_wall_mesh)
    eng = _engine(engine)
    lumen = _winding(q, vl, fl, t, bool(two_sided), eng)
    wall = _winding(q, vw, fw, t, bool(two_sided), eng)
    return IntramuralPoints((wall.inside == INSIDE) & (lumen.inside == OUTSIDE),
                            (wall.inside == UNDECIDED) | (lumen.inside == UNDECIDED), lumen, wall)


def first_run(mask: np.ndarray, points: np.ndarray):
    """``(start, end, length)`` of the first maximal run of consecutive True entries (end inclusive) and the sum of its
    segment lengths ``sqrt((dx*dx + dy*dy) + dz*dz)``, added in index order; ``(-1, -1, 0.0)`` without one."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return -1, -1, 0.0
    start = end = int(idx[0])
    while end + 1 < mask.shape[0] and mask[end + 1]:
        end += 1
    length = 0.0
    for i in range(start, end):
        d = points[i + 1] - points[i]
        length += float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return start, end, length


def intramural_course(centerline_points, aortic_lumen_mesh, aortic_wall_mesh, *, threshold: float = 0.5,
                      two_sided: bool = False, engine: Optional[N.Engine] = None) -> IntramuralCourse:
    """The intramural course of a coronary centerline (points in order, (n, 3)): ``intramural_points`` per point, then
    the first maximal run of consecutive intramural points (``start`` .. ``end``) and its ``length``.  The meshes as for
    ``intramural_points``."""
    r = intramural_points(centerline_points, aortic_lumen_mesh, aortic_wall_mesh, threshold=threshold, two_sided=two_sided,
                          engine=engine)
    start, end, length = first_run(r.mask, _p3(centerline_points))
    return IntramuralCourse(r.mask, start, end, length, r)
