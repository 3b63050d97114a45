"""Mesh cross-sections: the exact cut of a triangle mesh by a stack of planes, and the lumen profile along a centerline.

The reference has nothing of the kind: ``discretize_vessel`` gives every mesh *vertex* to its nearest slice anchor and
draws a spline through the flattened cloud, which is the input its tree wants and not a cross-section (its area follows
the vertex density and the step, and a short stenosis is smeared over a slice's thickness).  Its roadmap lists
"automatically assess lumen area, minor-, major axis, mla ... from the CCTA mesh" and "Discretize CCTA geometry in
layers following centerline" as open; ``vessel_profile`` is that item.

The rule is include/mm_ccta.h, "mesh cross-sections", restated in tests/mm_checkers/mesh_sections.py: every
(plane, face) pair is tested on the device (csrc/mm_section_kernels.hip), the host plans the (chunk, plane run) items
and chains, measures and selects (csrc/mm_section.cpp).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _native as N
from .ccta import MM_ERR_TOO_LARGE, _engine
from .centerline import Centerline
from .frames import Contour
from .morphometry import measure_csr, summary_from_measures
from .surface import _finite, _mesh_arrays

SECTION_REPORT_KEYS = ("n_planes", "n_faces", "n_skipped_faces", "n_segments", "n_contours", "n_closed", "n_open",
                       "n_branched", "items", "items_total", "face_tests", "n_launches", "bytes_uploaded",
                       "bytes_downloaded")
CLOSED, OPEN, BRANCHED = 0, 1, 2
# a segment record (MM_SECTION_SEGMENT_BYTES): plane << 32 | face, the two edge keys (lo, hi), the two points
SEGMENT_DTYPE = np.dtype([("key", "<u8"), ("e", "<i4", (4,)), ("p", "<f8", (6,))])
assert SEGMENT_DTYPE.itemsize == 72
PROFILE_HEADERS = ("index", "arc_length", "area", "equivalent_diameter", "major", "minor_3d", "elliptic_ratio", "perimeter")


@dataclass
class MeshCrossSections:
    """Contour ``i`` = ``points[contour_off[i]:contour_off[i + 1]]``; the contours of plane ``p`` are
    ``plane_off[p]:plane_off[p + 1]``, ordered by their smallest edge key.  ``point_edge``: the mesh edge (lo, hi) a point
    lies on; ``point_face``: the face of the segment that leaves the point (-1 at the far end of an open polyline and in
    a branched component).  ``contour_kind``: 0 closed, 1 open, 2 branched.  ``contour_area`` (NaN unless closed),
    ``contour_length``, ``contour_centroid`` by rule 6.  ``selected[p]``: the closed loop of plane ``p`` around its
    origin, the smallest of several, or -1.  ``report``: SECTION_REPORT_KEYS and ``attempts``."""
    contour_off: np.ndarray
    points: np.ndarray
    point_edge: np.ndarray
    point_face: np.ndarray
    contour_plane: np.ndarray
    contour_kind: np.ndarray
    contour_area: np.ndarray
    contour_length: np.ndarray
    contour_centroid: np.ndarray
    plane_off: np.ndarray
    selected: np.ndarray
    report: dict

    def __len__(self) -> int:
        return int(self.contour_off.shape[0]) - 1

    def contour(self, i: int) -> np.ndarray:
        """The (m, 3) points of contour ``i``."""
        if not 0 <= int(i) < len(self):
            raise IndexError("contour index out of range")
        return self.points[int(self.contour_off[i]):int(self.contour_off[i + 1])]


def _planes(origins, normals) -> Tuple[np.ndarray, np.ndarray]:
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float64))
    n = np.ascontiguousarray(np.asarray(normals, dtype=np.float64))
    if o.size == 0 and n.size == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    if o.ndim != 2 or o.shape[1] != 3 or n.shape != o.shape:
        raise ValueError("origins and normals must both be (P, 3)")
    _finite(o, "plane origins")
    if not np.isfinite(n).all():
        raise ValueError("plane normals must be finite")
    if (n == 0.0).all(axis=1).any():
        raise ValueError("a plane normal must not be zero")
    return o, n


def _checked(mesh, origins, normals):
    v, f = _mesh_arrays(mesh)
    _finite(v, "vertex coordinates")
    o, n = _planes(origins, normals)
    return v, f, o, n


class _Outputs:
    """The output arrays of mm_mesh_sections / mm_section_chain for `cap` segments and P planes."""

    def __init__(self, cap: int, P: int):
        c = max(cap, 1)
        self.contour_off = np.zeros(c + 1, dtype=np.int64)
        self.points = np.zeros((2 * c, 3))
        self.point_edge = np.zeros((2 * c, 2), dtype=np.int64)
        self.point_face = np.zeros(2 * c, dtype=np.int64)
        self.contour_plane = np.zeros(c, dtype=np.int64)
        self.contour_kind = np.zeros(c, dtype=np.int8)
        self.contour_area = np.zeros(c)
        self.contour_length = np.zeros(c)
        self.contour_centroid = np.zeros((c, 3))
        self.plane_off = np.zeros(P + 1, dtype=np.int64)
        self.selected = np.zeros(max(P, 1), dtype=np.int64)
        self.P = P

    def pointers(self):
        return [N._ptr(a) for a in (self.contour_off, self.points, self.point_edge, self.point_face, self.contour_plane,
                                    self.contour_kind, self.contour_area, self.contour_length, self.contour_centroid,
                                    self.plane_off, self.selected)]

    def result(self, n_contours: int, report: dict) -> MeshCrossSections:
        m = int(self.contour_off[n_contours])
        return MeshCrossSections(self.contour_off[:n_contours + 1].copy(), self.points[:m].copy(), self.point_edge[:m].copy(),
                                 self.point_face[:m].copy(), self.contour_plane[:n_contours].copy(),
                                 self.contour_kind[:n_contours].copy(), self.contour_area[:n_contours].copy(),
                                 self.contour_length[:n_contours].copy(), self.contour_centroid[:n_contours].copy(),
                                 self.plane_off.copy(), self.selected[:self.P].copy(), report)


def section_plan(mesh, origins, normals) -> dict:
    """TEST HOOK (``mm_section_plan``; host only, no engine): the staging and the items ``mesh_cross_sections`` builds.
    ``order[j]``: the face staged at position j; ``boxes``: (lo xyz, hi xyz) of every chunk; ``plane_list``: per chunk,
    ascending, the planes that pass rule 8; ``items``: (chunk, first entry in plane_list, planes, 0), one per workgroup;
    ``pairs`` / ``pairs_total``: the report's ``items`` / ``items_total``."""
    v, f, o, n = _checked(mesh, origins, normals)
    nf, P = f.shape[0], o.shape[0]
    order, info = np.zeros(max(nf, 1), dtype=np.int32), np.zeros(8, dtype=np.int64)
    head = [N._ptr(v), v.shape[0], N._ptr(f), nf, N._ptr(o), N._ptr(n), P, N._ptr(order), N._ptr(info)]
    N.check(N.lib().mm_section_plan(*head, None, None, 0, None, 0), "section_plan")
    pairs, nch, n_items = int(info[0]), int(info[3]), int(info[4])
    boxes, plist = np.zeros((max(nch, 1), 6)), np.zeros(max(pairs, 1), dtype=np.int32)
    items = np.zeros((max(n_items, 1), 4), dtype=np.int32)
    N.check(N.lib().mm_section_plan(*head, N._ptr(boxes), N._ptr(plist), pairs, N._ptr(items), n_items), "section_plan")
    return {"order": order[:nf].copy(), "boxes": boxes[:nch].copy(), "plane_list": plist[:pairs].copy(),
            "items": items[:n_items].copy(), "pairs": pairs, "pairs_total": int(info[1]), "chunk": int(info[2]),
            "run": int(info[5]), "face_tests": int(info[6]), "n_skipped_faces": int(info[7])}


def section_cut_host(mesh, origins, normals) -> np.ndarray:
    """TEST HOOK (``mm_section_cut_host``; host only): the segment records (SEGMENT_DTYPE) of the planned items, cut on
    the host by the arithmetic the kernel runs, sorted by (plane, face)."""
    v, f, o, n = _checked(mesh, origins, normals)
    head = [N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(o), N._ptr(n), o.shape[0]]
    count = np.zeros(1, dtype=np.int64)
    N.check(N.lib().mm_section_cut_host(*head, 0, None, N._ptr(count)), "section_cut_host")
    seg = np.zeros(max(int(count[0]), 1), dtype=SEGMENT_DTYPE)
    N.check(N.lib().mm_section_cut_host(*head, int(count[0]), N._ptr(seg), N._ptr(count)), "section_cut_host")
    return seg[:int(count[0])].copy()


def section_chain(segments, origins, normals) -> MeshCrossSections:
    """TEST HOOK (``mm_section_chain``; host only): rules 5 to 7 on segment records sorted by (plane, face) -- the code
    ``mesh_cross_sections`` runs on what the device returns."""
    seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
    o, n = _planes(origins, normals)
    out = _Outputs(seg.shape[0], o.shape[0])
    counts = np.zeros(5, dtype=np.int64)
    N.check(N.lib().mm_section_chain(N._ptr(seg) if seg.shape[0] else None, seg.shape[0], N._ptr(o), N._ptr(n), o.shape[0],
                                     *out.pointers(), N._ptr(counts)), "section_chain")
    report = {"n_segments": int(seg.shape[0]), "n_contours": int(counts[0]), "n_closed": int(counts[2]),
              "n_open": int(counts[3]), "n_branched": int(counts[4])}
    return out.result(int(counts[0]), report)


def _default_cap(nf: int, P: int) -> int:
    # a plane through a tube of nf faces crosses about sqrt(nf) of them; the retry covers everything else
    return min(nf * P, P * math.isqrt(nf) + 4096)


def mesh_cross_sections(mesh, origins, normals, *, max_segments: Optional[int] = None,
                        engine: Optional[N.Engine] = None) -> MeshCrossSections:
    """The exact intersection of ``mesh`` -- a ``(vertices, faces)`` pair, an object with ``.vertices`` / ``.faces``, or
    a results dict with ``"mesh"`` -- with the planes through ``origins`` (P, 3) with ``normals`` (P, 3; they need not be
    unit): ``MeshCrossSections``.  A vertex exactly on a plane counts as above it, so a plane through vertices, edges or
    whole faces needs no special case and every crossed face gives one segment.  Vertex identity is the index, not the
    coordinates: an unwelded seam cuts into open polylines -- ``repair_mesh`` welds it first.  Faces with a repeated
    index are skipped and counted.  The result has one bit pattern whatever the order of the faces (``point_face`` maps
    through the permutation).  ``max_segments`` sizes the segment buffer; where it is too small the call is repeated once
    with the count the first one returned.  A zero or non-finite normal, a shape mismatch, non-finite coordinates and a
    face index out of range raise ``ValueError`` before the engine is touched; an empty mesh and zero planes are valid."""
    v, f, o, n = _checked(mesh, origins, normals)
    nf, P = f.shape[0], o.shape[0]
    if max_segments is None:
        cap = _default_cap(nf, P)
    else:
        if int(max_segments) != max_segments or int(max_segments) < 0:
            raise ValueError("max_segments must be a non-negative integer")
        cap = min(int(max_segments), nf * P)
    rep = N.MMSectionReport()
    h = _engine(engine).handle
    for attempt in range(2):
        out = _Outputs(cap, P)
        rc = N.lib().mm_mesh_sections(h, N._ptr(v), v.shape[0], N._ptr(f), nf, N._ptr(o), N._ptr(n), P, cap, *out.pointers(),
                                      C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and rep.n_segments > cap:
            cap = int(rep.n_segments)
            continue
        N.check(rc, "mesh_cross_sections")
        break
    report = {k: int(getattr(rep, k)) for k in SECTION_REPORT_KEYS}
    report["attempts"] = attempt + 1
    return out.result(report["n_contours"], report)


def _stations(centerline: Centerline, branch_id, step_mm):
    if not isinstance(centerline, Centerline):
        raise TypeError("centerline must be a Centerline")
    cl = centerline.resample(float(step_mm)) if step_mm is not None else centerline
    idx = np.arange(len(cl), dtype=np.int64)
    if branch_id is not None:
        idx = idx[cl.points["branch_id"] == branch_id]
    p = cl.points[idx]
    origins = np.stack([p["x"], p["y"], p["z"]], axis=1) if len(idx) else np.zeros((0, 3))
    normals = np.stack([p["tx"], p["ty"], p["tz"]], axis=1) if len(idx) else np.zeros((0, 3))
    return idx, origins, normals


def centerline_cross_sections(mesh, centerline: Centerline, *, branch_id: Optional[int] = None,
                              step_mm: Optional[float] = None,
                              engine: Optional[N.Engine] = None) -> Tuple[List[Optional[Contour]], MeshCrossSections]:
    """``mesh_cross_sections`` with a plane at every point of ``centerline`` (after ``resample(step_mm)`` where
    ``step_mm`` is given; only the points of ``branch_id`` where it is given), the tangent as normal.  Returns
    ``(contours, sections)``: ``contours[k]`` is the selected loop of station k as a ``frames.Contour`` (kind
    ``"lumen"``, ``id`` = the point's index in the centerline used, ``centroid`` = the loop's area centroid), or ``None``
    where no closed loop goes around the point."""
    idx, origins, normals = _stations(centerline, branch_id, step_mm)
    sec = mesh_cross_sections(mesh, origins, normals, engine=engine)
    contours: List[Optional[Contour]] = []
    for k, c in enumerate(sec.selected):
        if c < 0:
            contours.append(None)
            continue
        cen = sec.contour_centroid[c]
        contours.append(Contour(int(idx[k]), int(idx[k]), sec.contour(int(c)).copy(), (float(cen[0]), float(cen[1]), float(cen[2])),
                                kind="lumen"))
    return contours, sec


@dataclass
class VesselProfile:
    """``table``: one row per station, PROFILE_HEADERS (NaN where no loop goes around the station's point);
    ``summary``: ``(mla, max_stenosis, stenosis_length_mm)`` by ``summary_from_measures`` on the stations that have a
    loop; ``contours`` and ``sections`` as ``centerline_cross_sections`` returns them; ``report``: the sections' report
    with ``n_stations`` and ``n_missing``."""
    table: np.ndarray
    summary: Tuple[float, float, float]
    contours: list
    sections: MeshCrossSections
    report: dict
    headers: tuple = PROFILE_HEADERS


def vessel_profile(mesh, centerline: Centerline, *, branch_id: Optional[int] = 0, step_mm: Optional[float] = None,
                   engine: Optional[N.Engine] = None) -> VesselProfile:
    """The lumen along a centerline, from the mesh itself (the reference's open roadmap item): per station the exact area
    and perimeter of the cross-section polygon (rule 6), the equivalent diameter ``2 sqrt(area / pi)`` and, from one
    launch of the contour measures over all selected loops, the major axis, the 3-D minor axis and the elliptic ratio;
    ``arc_length`` runs along the stations.  The summary is the reference's ``get_summary`` rule on the exact areas."""
    contours, sec = centerline_cross_sections(mesh, centerline, branch_id=branch_id, step_mm=step_mm, engine=engine)
    idx, origins, _ = _stations(centerline, branch_id, step_mm)
    S = len(contours)
    table = np.full((S, len(PROFILE_HEADERS)), np.nan)
    arc = 0.0
    for k in range(S):
        if k > 0:
            d = origins[k] - origins[k - 1]
            arc += math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        table[k, 0], table[k, 1] = float(idx[k]), arc
    have = [k for k in range(S) if contours[k] is not None]
    summary = (float("nan"), float("nan"), float("nan"))
    if have:
        sel = sec.selected[have]
        off = np.zeros(len(have) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(contours[k]) for k in have])
        xyz = np.concatenate([contours[k].points for k in have])
        m = measure_csr(off, xyz, np.ones(len(have), dtype=np.uint8), sec.contour_centroid[sel], False, engine)
        area = sec.contour_area[sel]
        table[have, 2] = area
        table[have, 3] = 2.0 * np.sqrt(area / math.pi)
        table[have, 4], table[have, 5], table[have, 6] = m.major, m.minor_3d, m.elliptic_ratio
        table[have, 7] = sec.contour_length[sel]
        summary = summary_from_measures(area, m.elliptic_ratio, m.n_points, sec.contour_centroid[sel])
    report = dict(sec.report)
    report["n_stations"], report["n_missing"] = S, S - len(have)
    return VesselProfile(table, summary, contours, sec, report)
