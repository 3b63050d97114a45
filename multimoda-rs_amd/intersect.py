"""Mesh intersection check: which faces of a mesh pass through other faces of it, or through faces of another mesh.

The reference leaves this to MeshLab and switches it off (multimodars/ccta/fixing_functions.py:182-185, 234:
``meshing_close_holes(selfintersection=False)``); here it is a report of its own.  Every pair of faces is *disjoint*,
*intersecting* or *undecided* by the rule of include/mm_ccta.h, "mesh intersections": filtered exact predicates in
unfused f64 whose verdicts, where they give one, hold in exact arithmetic on the inputs.  The pairs are tested on the
device (csrc/mm_intersect_kernels.hip); the host plans the chunk pairs and sorts the list.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N
from .ccta import _engine
from .surface import _mesh_arrays

INTERSECT_REPORT_KEYS = ("n_intersecting_pairs", "n_undecided_pairs", "n_degenerate_faces", "n_coincident_pairs", "items",
                         "items_total", "pair_box_tests", "narrow_tests", "n_launches", "bytes_uploaded",
                         "bytes_downloaded", "pairs_complete")


@dataclass
class MeshIntersections:
    """``face_state``: uint8 per face, bit 0 = the face is in a proved intersecting pair, bit 1 = in an undecided one
    (touching or coplanar within rounding); the two-mesh call holds a tuple, one array per mesh.  ``pairs``: (n, 2) int64
    original face indices, sorted by row, ``i < j`` in the self form, (face of a, face of b) in the two-mesh form;
    ``pair_state``: int8 per pair, 1 intersecting, 2 undecided.  Both are None where there are more pairs than
    ``max_pairs``; the flags and counts are complete all the same.  ``report``: INTERSECT_REPORT_KEYS."""
    face_state: object
    pairs: Optional[np.ndarray]
    pair_state: Optional[np.ndarray]
    report: dict


def _check_cap(max_pairs) -> int:
    if int(max_pairs) != max_pairs or int(max_pairs) < 0:
        raise ValueError("max_pairs must be a non-negative integer")
    return int(max_pairs)


def isect_plan(mesh_a, mesh_b=None) -> dict:
    """TEST HOOK (``mm_isect_plan``; host only, no engine): the staging and the items the intersection check builds.
    ``order_a[j]`` / ``order_b[j]``: the face staged at position j; ``boxes_a`` / ``boxes_b``: (lo xyz, hi xyz) of every
    chunk; ``items``: the chunk pairs (I, J) that run; ``items_total``: the chunk pairs before culling; ``chunk`` faces a
    chunk.  Without ``mesh_b`` the self form: ``I <= J`` over the chunks of ``mesh_a``."""
    va, fa = _mesh_arrays(mesh_a)
    vb, fb = (None, None) if mesh_b is None else _mesh_arrays(mesh_b)
    nfa, nfb = fa.shape[0], 0 if fb is None else fb.shape[0]
    order_a, order_b = np.zeros(max(nfa, 1), dtype=np.int32), np.zeros(max(nfb, 1), dtype=np.int32)
    info = np.zeros(5, dtype=np.int64)
    # a mesh b without a vertex still selects the two-mesh form
    pb = None if vb is None else (N._ptr(vb) if vb.shape[0] else N._ptr(np.zeros((1, 3))))
    head = [N._ptr(va), va.shape[0], N._ptr(fa), nfa, pb, 0 if vb is None else vb.shape[0],
            None if fb is None else N._ptr(fb), nfb, N._ptr(order_a), N._ptr(order_b), N._ptr(info)]
    N.check(N.lib().mm_isect_plan(*head, None, None, 0), "isect_plan")
    n, nca, ncb = int(info[0]), int(info[3]), int(info[4])
    boxes, items = np.zeros((max(nca + ncb, 1), 6)), np.zeros((max(n, 1), 2), dtype=np.int32)
    N.check(N.lib().mm_isect_plan(*head, N._ptr(boxes), N._ptr(items), n), "isect_plan")
    return {"order_a": order_a[:nfa].copy(), "order_b": order_b[:nfb].copy(), "boxes_a": boxes[:nca].copy(),
            "boxes_b": boxes[nca:nca + ncb].copy(), "items": items[:n].copy(), "items_total": int(info[1]),
            "chunk": int(info[2])}


def _run(va, fa, vb, fb, max_pairs: int, engine) -> MeshIntersections:
    self_form = vb is None
    nfa, nfb = fa.shape[0], 0 if self_form else fb.shape[0]
    bound = nfa * (nfa - 1) // 2 if self_form else nfa * nfb             # no call finds more pairs than there are
    cap = min(max_pairs, bound)
    state_a, state_b = np.zeros(nfa, dtype=np.uint8), np.zeros(nfb, dtype=np.uint8)
    pairs, pair_state = np.zeros((max(cap, 1), 2), dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int8)
    rep = N.MMIntersectReport()
    pb = None if self_form else (N._ptr(vb) if vb.shape[0] else N._ptr(np.zeros((1, 3))))
    N.check(N.lib().mm_mesh_intersections(_engine(engine).handle, N._ptr(va), va.shape[0], N._ptr(fa), nfa, pb,
                                          0 if self_form else vb.shape[0], None if self_form else N._ptr(fb), nfb, cap,
                                          N._ptr(state_a), N._ptr(state_b), N._ptr(pairs), N._ptr(pair_state), C.byref(rep)),
            "mesh_intersections")
    report = {k: int(getattr(rep, k)) for k in INTERSECT_REPORT_KEYS}
    report["pairs_complete"] = bool(report["pairs_complete"])
    n = report["n_intersecting_pairs"] + report["n_undecided_pairs"]
    complete = report["pairs_complete"]
    return MeshIntersections(state_a if self_form else (state_a, state_b), pairs[:n].copy() if complete else None,
                             pair_state[:n].copy() if complete else None, report)


def mesh_self_intersections(mesh, *, max_pairs: int = 1 << 20, engine: Optional[N.Engine] = None) -> MeshIntersections:
    """Every pair of faces of ``mesh`` -- a ``(vertices, faces)`` pair, an object with ``.vertices`` / ``.faces``, or a
    results dict with ``"mesh"`` -- that is not proved disjoint: ``MeshIntersections``.  Vertices with equal coordinates
    (``+0.0 == -0.0``) count as one, so an unwelded seam reads as adjacent, not as touching; faces that share vertices
    are reported only where they meet beyond them.  Faces without area are counted (``n_degenerate_faces``) and tested
    against nothing; two faces on the same three vertices count as intersecting (``n_coincident_pairs``).  The result
    has one bit pattern whatever the chunking or the order of the faces.  Non-finite coordinates and face indices out of
    range raise."""
    va, fa = _mesh_arrays(mesh)
    return _run(va, fa, None, None, _check_cap(max_pairs), engine)


def mesh_intersections(mesh_a, mesh_b, *, max_pairs: int = 1 << 20,
                       engine: Optional[N.Engine] = None) -> MeshIntersections:
    """Every face of ``mesh_a`` against every face of ``mesh_b`` -- a lumen against a wall, the intravascular lumen
    against the cut CCTA mesh before a stitch -- by the same rule, without vertex identities: faces that only touch are
    undecided.  ``face_state`` is ``(state_a, state_b)``; ``pairs`` holds (face of a, face of b)."""
    va, fa = _mesh_arrays(mesh_a)
    vb, fb = _mesh_arrays(mesh_b)
    return _run(va, fa, vb, fb, _check_cap(max_pairs), engine)
