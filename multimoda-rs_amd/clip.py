"""Mesh clipping: a vessel cut open at planes, with flat, optionally capped and extended ends whose faces name their patch.

The reference's paper gives "patient-specific CFD and FSI simulations" as the first use of its surface; a flow solver wants
inlets and outlets perpendicular to the centerline.  Nothing in the reference cuts them (its users go through VMTK's
clipper and flow extensions, or MeshLab); ``clip_mesh`` and ``open_vessel_ends`` are that step.

The rule is include/mm_ccta.h, "mesh clipping", restated in tests/mm_checkers/mesh_clip.py: the sections of the planes
come from ``mesh_cross_sections``' engine, the host reads the cut sets off the loops and writes one record per cut face,
and connectivity, the pieces and the faces run on the device (csrc/mm_clip_kernels.hip, csrc/mm_clip.cpp).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .ccta import MM_ERR_TOO_LARGE, _engine
from .centerline import Centerline
from .section import _planes
from .surface import _finite, _mesh_arrays

CLIP_REPORT_KEYS = ("n_cuts", "n_applied", "n_vertices", "n_faces", "n_new_vertices", "n_dropped_vertices",
                    "n_dropped_faces", "n_cut_faces", "n_pieces", "n_null_pieces", "n_ext_faces", "n_cap_faces",
                    "n_closed_loops", "n_open_loops", "jump_rounds", "n_launches", "bytes_uploaded", "bytes_downloaded")
KEEP = {"below": 0, "above": 1}
SCOPE = {"loop": 0, "plane": 1}
OK, NO_LOOP, OVERLAP, NOT_SEPARATING, KEPT_SIDE_DROPPED = 0, 1, 2, 3, 4
STATUS_NAMES = ("ok", "no_loop", "overlap", "not_separating", "kept_side_dropped")
UNTOUCHED, PIECE, EXTENSION, CAP = 0, 1, 2, 3


class ClipError(RuntimeError):
    """A cut that cannot be applied; ``statuses`` holds every cut's status (OK, NO_LOOP, OVERLAP, NOT_SEPARATING,
    KEPT_SIDE_DROPPED)."""

    def __init__(self, statuses):
        self.statuses = [int(s) for s in statuses]
        names = ", ".join(f"cut {k}: {STATUS_NAMES[s]}" for k, s in enumerate(self.statuses) if s != OK)
        super().__init__(f"clip_mesh: nothing was cut ({names})")


@dataclass
class ClippedMesh:
    """``vertices`` / ``faces``: the result.  ``vertex_origin``: the input vertex, or -1 - k for a vertex made for cut k;
    ``face_origin``: the parent face, or -1 - k; ``face_kind``: 0 untouched, 1 piece of a cut face, 2 extension, 3 cap.
    ``rims[k]``: per closed loop of cut k the vertex indices of its outermost ring (the rim itself without an
    extension), in loop order.  ``cut_status`` (0 OK, 1 NO_LOOP, 2 OVERLAP, 3 NOT_SEPARATING, 4 KEPT_SIDE_DROPPED),
    ``cut_area``, ``cut_length``, ``cut_centroid``: per cut, of its first closed loop (NaN without one); ``cut_points``, ``cut_loops``,
    ``cut_faces``: its loop points, closed loops and cut faces.  ``report``: CLIP_REPORT_KEYS and ``attempts``."""
    vertices: np.ndarray
    faces: np.ndarray
    vertex_origin: np.ndarray
    face_origin: np.ndarray
    face_kind: np.ndarray
    rims: List[List[np.ndarray]]
    cut_status: np.ndarray
    cut_area: np.ndarray
    cut_length: np.ndarray
    cut_centroid: np.ndarray
    cut_points: np.ndarray
    cut_loops: np.ndarray
    cut_faces: np.ndarray
    report: dict

    @property
    def applied(self) -> bool:
        return bool((self.cut_status == OK).all())


def _per_cut(value, names: dict, K: int, what: str) -> np.ndarray:
    values = [value] * K if isinstance(value, str) else list(value)
    if len(values) != K:
        raise ValueError(f"{what} must be a string or one string per cut")
    for x in values:
        if x not in names:
            raise ValueError(f"{what} must be one of {sorted(names)}")
    return np.array([names[x] for x in values], dtype=np.int32)


def _extension(extension):
    if extension is None:
        return 0.0, 0
    try:
        length, layers = extension
    except (TypeError, ValueError):
        raise ValueError("extension must be (length_mm, layers)") from None
    if int(layers) != layers or not math.isfinite(length) or length <= 0.0 or int(layers) <= 0:
        raise ValueError("extension must be (length_mm > 0, layers > 0)")
    return float(length), int(layers)


def _checked(mesh, origins, normals, keep, scope, cap, extension):
    v, f = _mesh_arrays(mesh)
    _finite(v, "vertex coordinates")
    o, n = _planes(origins, normals)
    K = o.shape[0]
    length, layers = _extension(extension)
    return v, f, o, n, _per_cut(keep, KEEP, K, "keep"), _per_cut(scope, SCOPE, K, "scope"), int(bool(cap)), length, layers


def _call(fn, head, v, f, o, n, keep, scope, cap, length, layers, what) -> ClippedMesh:
    nv, nf, K = v.shape[0], f.shape[0], o.shape[0]
    # a loop through a tube of nf faces has about sqrt(nf) points; the retry covers everything else
    m = K * (math.isqrt(nf) + 64)
    vert_cap, face_cap = nv + m * (layers + 1) + K, nf + m * (2 * layers + 3)
    rep = N.MMClipReport()
    status, measures = np.zeros((max(K, 1), 4), dtype=np.int64), np.zeros((max(K, 1), 5))
    for attempt in range(2):
        ov, of = np.zeros((max(vert_cap, 1), 3)), np.zeros((max(face_cap, 1), 3), dtype=np.int64)
        vo, fo = np.zeros(max(vert_cap, 1), dtype=np.int64), np.zeros(max(face_cap, 1), dtype=np.int64)
        fk = np.zeros(max(face_cap, 1), dtype=np.int8)
        rim_off, rim_index = np.zeros(vert_cap + 1, dtype=np.int64), np.zeros(max(vert_cap, 1), dtype=np.int64)
        rc = fn(*head, N._ptr(v), nv, N._ptr(f), nf, N._ptr(o), N._ptr(n), N._ptr(keep), N._ptr(scope), K, cap, length, layers,
                vert_cap, face_cap, N._ptr(ov), N._ptr(of), N._ptr(vo), N._ptr(fo), N._ptr(fk), N._ptr(status), N._ptr(measures),
                N._ptr(rim_off), N._ptr(rim_index), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and (rep.n_vertices > vert_cap or rep.n_faces > face_cap):
            vert_cap, face_cap = max(vert_cap, int(rep.n_vertices)), max(face_cap, int(rep.n_faces))
            continue
        N.check(rc, what)
        break
    report = {k: int(getattr(rep, k)) for k in CLIP_REPORT_KEYS}
    report["attempts"] = attempt + 1
    V, F = report["n_vertices"], report["n_faces"]
    rims: List[List[np.ndarray]] = [[] for _ in range(K)]
    r = 0
    if report["n_applied"]:
        for k in range(K):
            for _ in range(int(status[k, 2])):
                rims[k].append(rim_index[int(rim_off[r]):int(rim_off[r + 1])].copy())
                r += 1
    return ClippedMesh(ov[:V].copy(), of[:F].copy(), vo[:V].copy(), fo[:F].copy(), fk[:F].copy(), rims, status[:K, 0].copy(),
                       measures[:K, 0].copy(), measures[:K, 1].copy(), measures[:K, 2:5].copy(), status[:K, 1].copy(),
                       status[:K, 2].copy(), status[:K, 3].copy(), report)


def clip_mesh_host(mesh, origins, normals, *, keep="below", scope="loop", cap=False, extension=None) -> ClippedMesh:
    """TEST HOOK (``mm_mesh_clip_host``; no engine, no device): the rule of ``clip_mesh`` in host C++; statuses are
    returned, never raised."""
    args = _checked(mesh, origins, normals, keep, scope, cap, extension)
    return _call(N.lib().mm_mesh_clip_host, [], *args, "clip_mesh_host")


def clip_mesh(mesh, origins, normals, *, keep="below", scope="loop", cap=False, extension=None, strict=True,
              engine: Optional[N.Engine] = None) -> ClippedMesh:
    """Cut ``mesh`` -- a ``(vertices, faces)`` pair, an object with ``.vertices`` / ``.faces``, or a results dict with
    ``"mesh"`` -- open at the K planes through ``origins`` (K, 3) with ``normals`` (K, 3; they need not be unit).  ``keep``
    ("below": the side the normal points away from stays; "above") and ``scope`` are each a string or one per cut.  A
    "loop" cut splits only the faces of the smallest closed section loop around its origin and throws away what hangs
    on the other side of that loop *by connectivity*, so a plane through a coronary outlet does not touch the aorta it
    also passes through; a "plane" cut splits every crossed face and drops every vertex on the other side.  ``cap`` closes
    every closed rim with a fan to the loop's area centroid; ``extension=(length_mm, layers)`` first extends it by a
    straight piece along the normal.  ``face_kind`` and ``face_origin`` name the patch of every face, ``rims`` the
    outermost ring of every end.  A vertex exactly on a plane counts as above it; pieces without area that this leaves
    are kept and counted (``n_null_pieces``; ``repair_mesh`` removes them).  All cuts are applied or none: with
    ``strict`` a status other than OK (no loop around an origin, two cuts through one face, a loop that does not separate
    the mesh, a cut whose kept side another cut throws away) raises ``ClipError`` carrying the statuses, otherwise the input comes back unchanged with them.  Bad
    arguments raise ``ValueError`` before the engine is touched; an empty mesh and zero cuts are valid; buffers that turn
    out too small are grown once."""
    args = _checked(mesh, origins, normals, keep, scope, cap, extension)
    got = _call(N.lib().mm_mesh_clip, [_engine(engine).handle], *args, "clip_mesh")
    if strict and not got.applied:
        raise ClipError(got.cut_status)
    return got


def vessel_end_stations(centerline: Centerline, *, outlet_mm: float, inlet_mm: Optional[float] = None,
                        branches: Optional[Sequence[int]] = None):
    """The cuts of ``open_vessel_ends``: ``(stations, origins, normals, keep)``.  Arc length is the sequential f64 sum of
    ``sqrt((dx dx + dy dy) + dz dz)`` inside a branch; an outlet sits at the last point of its branch with at least
    ``outlet_mm`` of arc left, the inlet at the first point of branch 0 whose arc length is at least ``inlet_mm``; a
    normal is the forward difference to the next point of the branch (at its last point, from the one before)."""
    if not isinstance(centerline, Centerline):
        raise TypeError("centerline must be a Centerline")
    if not math.isfinite(outlet_mm) or outlet_mm < 0.0 or (inlet_mm is not None and (not math.isfinite(inlet_mm) or inlet_mm < 0.0)):
        raise ValueError("outlet_mm and inlet_mm must be finite and >= 0")
    p = centerline.points
    ids = [int(b) for b in p["branch_id"]]
    every = sorted(set(ids))
    wanted = every if branches is None else [int(b) for b in branches]
    xyz = [(float(a), float(b), float(c)) for a, b, c in zip(p["x"], p["y"], p["z"])]

    def run(b):
        idx = [i for i, x in enumerate(ids) if x == b]
        if len(idx) < 2:
            raise ValueError(f"branch {b} needs at least two centerline points")
        arc = [0.0]
        for i, j in zip(idx, idx[1:]):
            dx, dy, dz = xyz[j][0] - xyz[i][0], xyz[j][1] - xyz[i][1], xyz[j][2] - xyz[i][2]
            arc.append(arc[-1] + math.sqrt((dx * dx + dy * dy) + dz * dz))
        return idx, arc

    def tangent(idx, at):
        i, j = (idx[at], idx[at + 1]) if at + 1 < len(idx) else (idx[at - 1], idx[at])
        return [xyz[j][0] - xyz[i][0], xyz[j][1] - xyz[i][1], xyz[j][2] - xyz[i][2]]

    stations, origins, normals, keep = [], [], [], []
    if inlet_mm is not None:
        idx, arc = run(0)
        at = [k for k in range(len(idx)) if arc[k] >= inlet_mm]
        if not at:
            raise ValueError("branch 0 is shorter than inlet_mm")
        stations.append(idx[at[0]]); origins.append(xyz[idx[at[0]]]); normals.append(tangent(idx, at[0])); keep.append("above")
    for b in wanted:
        idx, arc = run(b)
        at = [k for k in range(len(idx)) if arc[-1] - arc[k] >= outlet_mm]
        if not at:
            raise ValueError(f"branch {b} is shorter than outlet_mm")
        stations.append(idx[at[-1]]); origins.append(xyz[idx[at[-1]]]); normals.append(tangent(idx, at[-1])); keep.append("below")
    return (np.array(stations, dtype=np.int64), np.array(origins, dtype=np.float64).reshape(-1, 3),
            np.array(normals, dtype=np.float64).reshape(-1, 3), keep)


def open_vessel_ends(mesh, centerline: Centerline, *, outlet_mm: float, inlet_mm: Optional[float] = None,
                     branches: Optional[Sequence[int]] = None, cap=False, extension=None, strict=True,
                     engine: Optional[N.Engine] = None) -> ClippedMesh:
    """``clip_mesh`` with "loop" cuts perpendicular to ``centerline``: with ``inlet_mm`` one that keeps what lies
    downstream of the first point of branch 0 at that arc length, then one per branch in ``branches`` (default: all)
    that keeps what lies upstream of the last point with at least ``outlet_mm`` of arc left
    (``vessel_end_stations``).  ``report["stations"]`` lists the centerline indices chosen, in cut order."""
    stations, origins, normals, keep = vessel_end_stations(centerline, outlet_mm=outlet_mm, inlet_mm=inlet_mm, branches=branches)
    got = clip_mesh(mesh, origins, normals, keep=keep, scope="loop", cap=cap, extension=extension, strict=strict, engine=engine)
    got.report["stations"] = stations.tolist()
    return got
