"""A centerline from a mesh: the geodesic distance field over the edge graph, the band (level-set) skeleton after
Lazarus and Verroust, and its tree of branches (include/mm_centerline.h, rules G, S and T).  The reference
has no such function ("Create Centerline directly from mesh" is an open item of its roadmap); the rules are this
project's own, restated in tests/mm_checkers/mesh_skeleton.py.  Field and skeleton run on the device, the tree is host
C++ over the few thousand nodes; there is no host fall-back for the device part.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N
from .ccta import MM_ERR_TOO_LARGE, _checked_faces, _engine, _mesh_parts, _p3, order_boundary_rings
from .centerline import CL_DTYPE, Centerline

GEODESIC_REPORT_KEYS = ("n_vertices", "n_faces", "n_edges", "n_skipped_edges", "n_reached", "rounds", "n_batches",
                        "n_launches", "bytes_uploaded", "bytes_downloaded", "max_dist", "max_edge")


def _mesh_arrays(mesh):
    """The checked arrays of a mesh: ValueError before the engine is touched.  Coordinates may be anything."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    return v, _checked_faces(faces, v.shape[0])


def _seed_vertices(seeds, v: np.ndarray) -> np.ndarray:
    """Seeds as vertex indices: an integer array as it is (repeats allowed), or one ``(x, y, z)`` point, which stands
    for the vertex nearest to it by (dx dx + dy dy) + dz dz, the lowest index among equals."""
    a = np.asarray(seeds)
    nv = v.shape[0]
    if a.size == 0:
        raise ValueError("seeds must not be empty")
    if np.issubdtype(a.dtype, np.integer):
        s = np.ascontiguousarray(a.astype(np.int64).reshape(-1))
        if s.min() < 0 or s.max() >= nv:
            raise ValueError(f"seed out of range [0, {nv})")
        return s
    if not np.issubdtype(a.dtype, np.floating) or a.shape != (3,):
        raise ValueError("seeds must be an integer array of vertex indices or one (x, y, z) point")
    if nv == 0:
        raise ValueError("a seed point needs a vertex")
    d = v - a.astype(np.float64)
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    if not np.isfinite(q).any():
        raise ValueError("no vertex at a finite distance from the seed point")
    q = np.where(np.isnan(q), np.inf, q)
    return np.array([int(np.argmin(q))], dtype=np.int64)                  # argmin: the first of equal minima


def _geodesic(v: np.ndarray, f: np.ndarray, s: np.ndarray, engine):
    nv = v.shape[0]
    dist = np.zeros(nv, dtype=np.float64)
    pred = np.zeros(nv, dtype=np.int64)
    rep = N.MMGeodesicReport()
    N.check(N.lib().mm_mesh_geodesic(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), f.shape[0], N._ptr(s), s.shape[0],
                                     N._ptr(dist), N._ptr(pred), C.byref(rep)), "mesh_geodesic_distance")
    return dist, pred, {k: getattr(rep, k) for k in GEODESIC_REPORT_KEYS}


def mesh_geodesic_distance(mesh, seeds, *, engine: Optional[N.Engine] = None):
    """The distance along the edges of ``mesh`` (``(vertices, faces)`` or anything with ``.vertices`` / ``.faces``) from
    the nearest of ``seeds``, on the device: ``(dist, pred, report)``, ``dist`` f64[nv], ``pred`` int64[nv].

    ``seeds`` is an integer array of vertex indices (repeats allowed), or a single ``(x, y, z)`` point of floats, which
    means the vertex nearest to it, the lowest index on ties.

    The graph is the distinct edges of the faces between different vertices, each weighing its Euclidean length in
    unfused f64; an edge whose length is not finite is left out (``report["n_skipped_edges"]``).  ``dist`` is +0.0 at a
    seed, the smallest left-to-right rounded sum of weights over the paths from any seed elsewhere, and ``+inf`` where
    no path arrives: exactly what Dijkstra's algorithm returns, and, because rounded addition of a non-negative number
    is monotone, the one fixpoint the relaxation can reach -- the result has one bit pattern whatever the schedule
    (include/mm_centerline.h, "Rule G").  ``pred[v]`` is the smallest neighbour ``u`` with ``dist[u] + w(u, v) ==
    dist[v]``, -1 at seeds and unreached vertices.  This is a distance along edges, not the exact polyhedral geodesic:
    on a regular mesh it overestimates by the usual few per cent.

    ``report``: GEODESIC_REPORT_KEYS.  ``rounds``, ``n_batches`` and ``n_launches`` describe the schedule (a round
    relaxes every flagged block of 256 consecutive vertices to its local fixpoint) and may differ from run to run."""
    v, f = _mesh_arrays(mesh)
    return _geodesic(v, f, _seed_vertices(seeds, v), engine)


# ---- the band skeleton -------------------------------------------------------------------------------------------------

NODE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("radius", "<f8"), ("radius_min", "<f8"), ("weight", "<f8"),
                       ("band", "<i8"), ("first_vertex", "<i8"), ("n_vertices", "<i8"), ("flags", "<i8")])
assert NODE_DTYPE.itemsize == 80
TERMINAL_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("radius", "<f8"), ("node", "<i8")])
NODE_OPEN, NODE_PLAIN_MEAN, NODE_SEED = 1, 2, 4
SKELETON_REPORT_KEYS = ("n_nodes", "n_node_edges", "union_rounds", "n_launches", "bytes_uploaded", "bytes_downloaded",
                        "band_mm")
TREE_REPORT_KEYS = ("n_points", "n_branches", "n_roots", "n_components", "n_loops", "n_dropped_open", "n_pruned",
                    "n_terminals")


@dataclass
class SkeletonGraph:
    """``mesh_skeleton``'s result: ``vertex_node`` int64[nv] (-1: unreached), ``nodes`` (NODE_DTYPE records: x, y, z,
    radius, radius_min, weight, band, first_vertex, n_vertices, flags -- NODE_OPEN, NODE_PLAIN_MEAN, NODE_SEED), ``edges``
    int64[m, 2] (lo node < hi node, sorted), the field ``dist`` and ``pred``, and ``report``."""
    vertex_node: np.ndarray
    nodes: np.ndarray
    edges: np.ndarray
    dist: np.ndarray
    pred: np.ndarray
    report: dict


def longest_edge(v: np.ndarray, f: np.ndarray) -> float:
    """The longest finite edge of the faces, with the weight's own arithmetic (lo to hi, unfused)."""
    if f.shape[0] == 0:
        return 0.0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    lo, hi = e.min(axis=1), e.max(axis=1)
    with np.errstate(all="ignore"):
        d = v[hi] - v[lo]
        w = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    w = w[np.isfinite(w)]
    return float(w.max()) if w.size else 0.0


def _band(band_mm, v: np.ndarray, f: np.ndarray) -> float:
    if band_mm is None:
        band_mm = 2.0 * longest_edge(v, f)
        if not band_mm > 0.0:
            raise ValueError("the mesh has no edge of finite positive length: give band_mm")
    band_mm = float(band_mm)
    if not np.isfinite(band_mm) or not band_mm > 0.0:
        raise ValueError("band_mm must be finite and positive")
    return band_mm


def _skeleton(v: np.ndarray, f: np.ndarray, s: np.ndarray, band_mm: float, engine) -> SkeletonGraph:
    """mm_mesh_skeleton on checked arrays: capacities guessed first and, where they do not fit, once more with the sizes
    the first call reports (the protocol of ``mesh_adjacency_csr``)."""
    nv, nf = v.shape[0], f.shape[0]
    h = _engine(engine).handle
    dist, pred, vnode = np.zeros(nv, dtype=np.float64), np.zeros(nv, dtype=np.int64), np.zeros(nv, dtype=np.int64)
    rep = N.MMSkeletonReport()
    node_cap, edge_cap = max(min(nv, 1 << 16), 1), max(min(3 * nf, 1 << 18), 1)   # all but crumbled skeletons fit
    for attempt in (0, 1):
        nodes = np.zeros(node_cap, dtype=NODE_DTYPE)
        edges = np.zeros((edge_cap, 2), dtype=np.int64)
        rc = N.lib().mm_mesh_skeleton(h, N._ptr(v), nv, N._ptr(f), nf, N._ptr(s), s.shape[0], band_mm, node_cap, edge_cap,
                                      N._ptr(dist), N._ptr(pred), N._ptr(vnode), N._ptr(nodes), N._ptr(edges), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and (rep.n_nodes > node_cap or rep.n_node_edges > edge_cap):
            node_cap, edge_cap = max(int(rep.n_nodes), 1), max(int(rep.n_node_edges), 1)
            continue
        N.check(rc, "mesh_skeleton")
        break
    report = {k: getattr(rep, k) for k in SKELETON_REPORT_KEYS}
    report["field"] = {k: getattr(rep.field, k) for k in GEODESIC_REPORT_KEYS}
    return SkeletonGraph(vnode, nodes[:int(rep.n_nodes)].copy(), edges[:int(rep.n_node_edges)].copy(), dist, pred, report)


def mesh_skeleton(mesh, seeds, *, band_mm: Optional[float] = None, engine: Optional[N.Engine] = None) -> SkeletonGraph:
    """The level-set skeleton of ``mesh`` from ``seeds`` (as in ``mesh_geodesic_distance``), on the device, mesh and field
    resident: the geodesic field is cut into bands ``int(dist / band_mm)``, every connected component of a band is one
    node, placed at the area-weighted centroid of its vertices (each corner of a face carries a third of the face's
    area; vertex-count means are biased by vertex density), and nodes that touch across an edge are joined
    (include/mm_centerline.h, "Rule S").  Nodes are numbered by (band, smallest vertex).

    ``band_mm=None`` takes twice the longest finite edge of the mesh.  A band narrower than the edges breaks the rings
    of a vessel into crumbs, so a mesh with very uneven edges wants ``mm.isotropic_remesh`` first, or a band chosen by
    hand.  ``radius`` is the weighted mean distance of the node's vertices from its centre and ``radius_min`` the
    smallest, not an inscribed-sphere radius: ``mm.point_mesh_distance`` from the node centres gives those."""
    v, f = _mesh_arrays(mesh)
    return _skeleton(v, f, _seed_vertices(seeds, v), _band(band_mm, v, f), engine)


# ---- terminals, tree, branches -----------------------------------------------------------------------------------------

def _norm(dx: float, dy: float, dz: float) -> float:
    return float(np.sqrt((dx * dx + dy * dy) + dz * dz))


def rim_terminal(v: np.ndarray, ring) -> tuple:
    """``(start, x, y, z, radius)`` of one rim loop: the loop is walked from its smallest vertex ``start`` towards the
    smaller of that vertex's two ring neighbours; the point is the mean of the loop's vertices, each weighted by half
    the sum of its two rim edges, summed in that order, the radius the same weighted mean distance from the point."""
    ring = [int(i) for i in ring]
    m = len(ring)
    k = ring.index(min(ring))
    ring = ring[k:] + ring[:k]
    if m > 2 and ring[-1] < ring[1]:
        ring = [ring[0]] + ring[:0:-1]
    p = [v[i].tolist() for i in ring]
    length = [_norm(p[(i + 1) % m][0] - p[i][0], p[(i + 1) % m][1] - p[i][1], p[(i + 1) % m][2] - p[i][2]) for i in range(m)]
    wt = [0.5 * (length[i - 1] + length[i]) for i in range(m)]
    W, S = 0.0, [0.0, 0.0, 0.0]
    for i in range(m):
        W = W + wt[i]
        for c in range(3):
            S[c] = S[c] + wt[i] * p[i][c]
    with np.errstate(all="ignore"):
        centre = [float(np.float64(S[c]) / np.float64(W)) for c in range(3)]
        R = 0.0
        for i in range(m):
            R = R + wt[i] * _norm(p[i][0] - centre[0], p[i][1] - centre[1], p[i][2] - centre[2])
        return ring[0], centre[0], centre[1], centre[2], float(np.float64(R) / np.float64(W))


def skeleton_terminals(v: np.ndarray, rings, seeds, vertex_node: np.ndarray) -> np.ndarray:
    """TERMINAL_DTYPE records of the rim loops that hold no seed and whose smallest vertex the field reached, in ascending
    order of that vertex."""
    seed_set = set(int(i) for i in np.asarray(seeds).reshape(-1))
    found = []
    for ring in rings:
        if len(ring) == 0 or seed_set.intersection(int(i) for i in ring):
            continue
        start, x, y, z, r = rim_terminal(v, ring)
        if vertex_node[start] >= 0:
            found.append((start, x, y, z, r, int(vertex_node[start])))
    out = np.zeros(len(found), dtype=TERMINAL_DTYPE)
    for j, t in enumerate(sorted(found)):
        out[j] = t[1:]
    return out


def skeleton_centerline(nodes: np.ndarray, edges: np.ndarray, terminals: Optional[np.ndarray] = None,
                        min_branch_mm: Optional[float] = None):
    """``mm_skeleton_centerline`` (host C++; include/mm_centerline.h, "Rule T") on node records, node edges and
    terminals: ``(Centerline, report)``.  ``report``: TREE_REPORT_KEYS, ``point_node`` (the node of every point,
    ``len(nodes) + j`` for terminal j) and ``branches``, one dict per branch with ``parent_branch``, ``parent_index``
    (the junction's index in the centerline; -1 for a root's first branch), ``ends_at_rim`` and ``n_points``."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    term = np.zeros(0, dtype=TERMINAL_DTYPE) if terminals is None else np.ascontiguousarray(terminals, dtype=TERMINAL_DTYPE)
    cap = max(len(nodes) + len(term), 1)
    out = np.zeros(cap, dtype=CL_DTYPE)
    point_node, info = np.zeros(cap, dtype=np.int64), np.zeros((cap, 4), dtype=np.int64)
    rep = N.MMTreeReport()
    n = N.lib().mm_skeleton_centerline(N._ptr(nodes), len(nodes), N._ptr(edges), edges.shape[0], N._ptr(term), len(term),
                                       -1.0 if min_branch_mm is None else float(min_branch_mm), N._ptr(out),
                                       N._ptr(point_node), N._ptr(info), cap, C.byref(rep))
    if n < 0:
        N.check(int(n), "skeleton_centerline")
    report = {k: getattr(rep, k) for k in TREE_REPORT_KEYS}
    report["point_node"] = point_node[:int(n)].copy()
    report["branches"] = [{"parent_branch": int(a), "parent_index": int(b), "ends_at_rim": bool(c), "n_points": int(d)}
                          for a, b, c, d in info[:int(rep.n_branches)].tolist()]
    return Centerline(out[:int(n)].copy()), report


def centerline_from_mesh(mesh, seeds, *, band_mm: Optional[float] = None, min_branch_mm: Optional[float] = None,
                         spacing_mm: Optional[float] = None, smooth_sigma: Optional[float] = None,
                         engine: Optional[N.Engine] = None):
    """A centerline straight from a vessel mesh: ``(Centerline, report)``.  The composite of ``mesh_skeleton`` (``seeds``
    and ``band_mm`` as there: seed the inlet rim, or a point near it), the terminals of the open rims
    (``order_boundary_rings``; a rim that holds a seed gets none) and ``skeleton_centerline``, which orders the nodes
    into a tree, drops the partial rings before an open outlet (their centroids walk off to the wall; the rim's own
    centroid ends the branch instead), and cuts the tree into branches: branch 0 is the longest path from the inlet,
    the main vessel; every other branch is a contiguous run that starts at its first point off its parent, as
    ``prepare_centerline`` and the labelling expect.  A side path shorter than ``min_branch_mm`` (default: twice the
    radius at its junction) that does not end at an open rim is dropped.  ``radius`` is the node's mean vertex distance
    (``mm.point_mesh_distance`` from the points gives inscribed radii); tangents are forward differences.

    ``spacing_mm`` and ``smooth_sigma``, where given, run ``Centerline.resample`` and ``Centerline.smooth`` on the
    result, in that order; ``report["point_node"]`` and ``parent_index`` refer to the points before them.  On a closed
    mesh seeded by a point the first nodes sit in the seed-side cap: ``Centerline.trim_start`` removes them.  A mesh
    with handles gives ``report["n_loops"] > 0``; the tree is not healed.

    ``report``: the tree's (``skeleton_centerline``), ``skeleton`` (the skeleton's report), ``terminals`` and
    ``graph``, the ``SkeletonGraph``."""
    v, f = _mesh_arrays(mesh)
    s = _seed_vertices(seeds, v)
    band = _band(band_mm, v, f)
    if min_branch_mm is not None and not float(min_branch_mm) >= 0.0:
        raise ValueError("min_branch_mm must not be negative")
    graph = _skeleton(v, f, s, band, engine)
    rings = order_boundary_rings(f, v, engine=engine) if f.shape[0] else []
    terminals = skeleton_terminals(v, rings, s, graph.vertex_node)
    cl, report = skeleton_centerline(graph.nodes, graph.edges, terminals, min_branch_mm)
    report.update(skeleton=graph.report, terminals=terminals, graph=graph)
    if spacing_mm is not None:
        cl = cl.resample(float(spacing_mm))
    if smooth_sigma is not None:
        cl = cl.smooth(float(smooth_sigma))
    return cl, report
