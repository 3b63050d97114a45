"""Surface distance: how far points, or the surface of one mesh, lie from the surface of another.

The reference bounds this quantity inside MeshLab while it remeshes (multimodars/ccta/fixing_functions.py:196-219,
``checksurfdist`` / ``maxsurfdist``); this project keeps those steps out and measures the distance instead.  Every
point-to-triangle distance is computed on the device in exact f64 by the rule of include/mm_ccta.h, "surface distance"
(csrc/mm_tri_kernels.hip); the lattice samples and the means are host numpy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N
from .ccta import _checked_faces, _engine, _mesh_parts, _p3

SURFACE_REPORT_KEYS = ("items_pass_a", "items_pass_b", "items_skipped", "n_launches", "bytes_uploaded", "bytes_downloaded")


@dataclass
class PointMeshDistance:
    """Per query: ``distance`` = sqrt(``sq_distance``), the winning ``face`` (-1: none), its ``closest`` point and the
    ``region`` of the face it lies in (0 interior; 1, 2, 3 corner a, b, c; 4, 5, 6 edge ab, bc, ca; -1: none).
    ``report``: SURFACE_REPORT_KEYS."""
    distance: np.ndarray
    sq_distance: np.ndarray
    face: np.ndarray
    closest: np.ndarray
    region: np.ndarray
    report: dict


@dataclass
class DirectedDistance:
    """One direction of ``surface_distance`` over ``n`` samples: ``max`` is the directed Hausdorff distance, reached at
    sample ``argmax`` (the lowest on ties) of face ``sample_face`` of the sampled mesh, nearest to ``closest`` on face
    ``face`` of the other mesh.  Without a sample, or without a face to measure to, see ``surface_distance``."""
    max: float
    mean: float
    rms: float
    argmax: int
    sample_face: int
    face: int
    closest: np.ndarray
    n: int
    report: dict


@dataclass
class SurfaceDistanceReport:
    a_to_b: DirectedDistance
    b_to_a: DirectedDistance
    hausdorff: float
    n_launches: int
    bytes_uploaded: int
    bytes_downloaded: int


def _mesh_arrays(mesh):
    """(vertices (nv, 3) f64, faces (nf, 3) int64) of a ``(vertices, faces)`` pair, an object with ``.vertices`` /
    ``.faces``, or a results dict that holds one of those under ``"mesh"``."""
    if isinstance(mesh, dict):
        if "mesh" not in mesh:
            raise ValueError('a results dict needs a "mesh" entry')
        mesh = mesh["mesh"]
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    return v, _checked_faces(faces, v.shape[0])


def _finite(a: np.ndarray, what: str) -> None:
    if a.size and not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite")


def tri_plan(points, mesh) -> dict:
    """TEST HOOK (``mm_tri_plan``; host only, no engine): the staging and the work items ``point_mesh_distance`` builds.
    ``face_order[j]`` / ``query_perm[j]``: the face / query staged at position j; ``a`` / ``b``: the items of pass A and
    pass B as (q0, c0) in staged positions, ``a_lb2`` / ``b_lb2`` their lower bounds; ``qpb`` queries a block, ``chunk``
    faces a chunk."""
    v, f = _mesh_arrays(mesh)
    q = _p3(points)
    nv, nf, nq = v.shape[0], f.shape[0], q.shape[0]
    order, perm = np.zeros(max(nf, 1), dtype=np.int32), np.zeros(max(nq, 1), dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    args = [N._ptr(v), nv, N._ptr(f), nf, N._ptr(q), nq, N._ptr(order), N._ptr(perm), N._ptr(info)]
    N.check(N.lib().mm_tri_plan(*args, None, None, 0), "tri_plan")
    cap = int(info[0] + info[1])
    items, lb2 = np.zeros((max(cap, 1), 3), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.float64)
    N.check(N.lib().mm_tri_plan(*args, N._ptr(items), N._ptr(lb2), cap), "tri_plan")
    na = int(info[0])
    assert (items[:na, 0] == 0).all() and (items[na:cap, 0] == 1).all()
    return {"face_order": order[:nf].copy(), "query_perm": perm[:nq].copy(), "qpb": int(info[2]), "chunk": int(info[3]),
            "a": items[:na, 1:].copy(), "a_lb2": lb2[:na].copy(), "b": items[na:cap, 1:].copy(), "b_lb2": lb2[na:cap].copy()}


def _point_mesh(q: np.ndarray, v: np.ndarray, f: np.ndarray, engine) -> PointMeshDistance:
    nq = q.shape[0]
    sq = np.zeros(nq, dtype=np.float64)
    face = np.zeros(nq, dtype=np.int64)
    closest = np.zeros((nq, 3), dtype=np.float64)
    region = np.zeros(nq, dtype=np.int32)
    rep = N.MMSurfaceReport()
    N.check(N.lib().mm_point_mesh_distance(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(q), nq,
                                           N._ptr(sq), N._ptr(face), N._ptr(closest), N._ptr(region), C.byref(rep)),
            "point_mesh_distance")
    return PointMeshDistance(np.sqrt(sq), sq, face, closest, region, {k: int(getattr(rep, k)) for k in SURFACE_REPORT_KEYS})


def point_mesh_distance(points, mesh, *, engine: Optional[N.Engine] = None) -> PointMeshDistance:
    """The distance from every one of ``points`` (n, 3) to the surface of ``mesh`` -- a ``(vertices, faces)`` pair, an
    object with ``.vertices`` / ``.faces``, or a results dict with ``"mesh"`` -- with the nearest face (the lowest index
    among equally near ones), the closest point on it and its region: ``PointMeshDistance``.  Exact f64 on the device;
    the result has one bit pattern whatever the scheduling.  Faces without area count as their three edges.  A mesh
    without a face gives ``inf``, face -1, a NaN closest point and region -1.  Non-finite coordinates and face indices
    out of range raise ValueError."""
    v, f = _mesh_arrays(mesh)
    q = _p3(points)
    _finite(v, "mesh vertices")
    _finite(q, "points")
    return _point_mesh(q, v, f, engine)


def sample_mesh_surface(mesh, n: int = 1):
    """``(points, face)``: the lattice samples ``((a*i + b*j) + c*k) / n`` with ``i + j + k == n`` of every face
    ``(a, b, c)`` of ``mesh``, face by face, in ascending ``(i, j)`` order -- ``(n + 1)(n + 2) / 2`` a face, the corners
    c, b, a for ``n == 1`` -- and the face every sample belongs to.  Host numpy, deterministic."""
    if int(n) != n or int(n) < 1:
        raise ValueError("n must be an integer of at least 1")
    n = int(n)
    v, f = _mesh_arrays(mesh)
    ij = np.array([(i, j) for i in range(n + 1) for j in range(n + 1 - i)], dtype=np.float64).reshape(-1, 2)
    wi, wj = ij[:, 0][None, :, None], ij[:, 1][None, :, None]
    wk = float(n) - wi - wj
    a, b, c = v[f[:, 0]][:, None, :], v[f[:, 1]][:, None, :], v[f[:, 2]][:, None, :]
    pts = ((a * wi + b * wj) + c * wk) / float(n)
    owner = np.repeat(np.arange(f.shape[0], dtype=np.int64), ij.shape[0])
    return np.ascontiguousarray(pts.reshape(-1, 3)), owner


def _directed(pts: np.ndarray, owner: np.ndarray, r: PointMeshDistance) -> DirectedDistance:
    n = pts.shape[0]
    if n == 0:
        nan = float("nan")
        return DirectedDistance(nan, nan, nan, -1, -1, -1, np.full(3, np.nan), 0, r.report)
    k = int(np.argmax(r.sq_distance))                       # the first of the largest: sqrt is monotone
    total = float(np.cumsum(r.distance)[-1])                # sequential, in index order
    total_sq = float(np.cumsum(r.sq_distance)[-1])
    return DirectedDistance(float(r.distance[k]), total / n, float(np.sqrt(total_sq / n)), k, int(owner[k]), int(r.face[k]),
                            r.closest[k].copy(), n, r.report)


def surface_distance(mesh_a, mesh_b, *, samples: int = 1, engine: Optional[N.Engine] = None) -> SurfaceDistanceReport:
    """The distance between two surfaces, measured from the ``sample_mesh_surface(mesh, samples)`` points of each to the
    triangles of the other: ``a_to_b`` and ``b_to_a`` (``DirectedDistance``: ``max`` is the directed Hausdorff distance
    of the samples, exact; ``mean`` and ``rms`` are summed on the host in index order) and ``hausdorff``, the larger of
    the two ``max``.  Both directions run on one engine, each mesh uploaded once as a mesh; the launch and byte counts
    are the sums of the two calls.  A direction without samples has NaN figures and ``argmax`` -1 and does not enter
    ``hausdorff``; one without a face to measure to has ``max`` inf."""
    va, fa = _mesh_arrays(mesh_a)
    vb, fb = _mesh_arrays(mesh_b)
    _finite(va, "mesh_a vertices")
    _finite(vb, "mesh_b vertices")
    eng = _engine(engine)
    pa, oa = sample_mesh_surface((va, fa), samples)
    pb, ob = sample_mesh_surface((vb, fb), samples)
    ab = _directed(pa, oa, _point_mesh(pa, vb, fb, eng))
    ba = _directed(pb, ob, _point_mesh(pb, va, fa, eng))
    tops = [d.max for d in (ab, ba) if d.n]
    return SurfaceDistanceReport(ab, ba, max(tops) if tops else float("nan"),
                                 *(ab.report[k] + ba.report[k] for k in ("n_launches", "bytes_uploaded", "bytes_downloaded")))
