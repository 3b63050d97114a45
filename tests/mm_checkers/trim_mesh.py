"""Plain numpy / Python restatement of the CCTA mesh trimming (multimodars/ccta/boundary.py:26-325,
multimodars/ccta/stitching.py:18-352, multimodars/ccta/__init__.py:341-429, build_adjacency_map of
src/ccta/binding/ccta_py.rs:507-525), with the reference's set-order walk replaced by the package's fixed rule:

- rings are discovered in increasing order of their smallest remaining vertex, and each starts at it;
- from every vertex the walk goes to the smallest neighbour that is not the previous vertex and still remains;
- length ties keep discovery order (a stable sort); _join_rings keeps its loop order and strict <.

Distances and cosines are summed as (x*x + y*y) + z*z in f64.  Points are compared by value through dicts of tuples:
-0.0 equals 0.0, a row with a NaN equals nothing and the last of duplicated vertices wins.  The face and edge stages
are vectorised (a million faces is fine); the rim logic is plain Python."""
from __future__ import annotations

import math

import numpy as np

TRIM_KEYS = ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "lca_removed_points", "proximal_points",
             "distal_points")


def _p3(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64).reshape(-1, 3)


def open_boundary_edges(faces) -> np.ndarray:
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.empty((0, 2), dtype=np.int64)
    edges = np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    return uniq[counts == 1]


def build_adjacency_map(faces) -> dict:
    adj: dict = {}
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            adj.setdefault(u, set()).add(w)
            adj.setdefault(w, set()).add(u)
    return adj


def boundary_graph(edges) -> dict:
    g: dict = {}
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        g.setdefault(a, set()).add(b)
        g.setdefault(b, set()).add(a)
    return g


def rims_touching(graph: dict, seeds: set) -> dict:
    if not seeds:
        return {v: set(ns) for v, ns in graph.items()}
    keep: set = set()
    unvisited = set(graph)
    while unvisited:
        stack = [unvisited.pop()]
        comp = set(stack)
        while stack:
            v = stack.pop()
            for w in graph.get(v, set()):
                if w not in comp:
                    comp.add(w)
                    unvisited.discard(w)
                    stack.append(w)
        if comp & seeds:
            keep |= comp
    return {v: set(graph[v]) & keep for v in keep}


def walk_rings(graph: dict) -> list:
    nbrs = {v: sorted(ns) for v, ns in graph.items()}
    remaining = set(graph)
    rings = []
    for start in sorted(graph):
        if start not in remaining:
            continue
        ring = [start]
        remaining.discard(start)
        prev, cur = -1, start
        while True:
            nxt = next((n for n in nbrs[cur] if n != prev and n in remaining), None)
            if nxt is None:
                break
            ring.append(nxt)
            remaining.discard(nxt)
            prev, cur = cur, nxt
        rings.append(ring)
    return rings


def _norm(d) -> float:
    return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def despike_ring(ring: list, V: list, cos_thresh: float) -> list:
    pts = list(ring)
    changed = True
    while changed and len(pts) > 3:
        changed = False
        m = len(pts)
        for i in range(m):
            d1 = _sub(V[pts[i - 1]], V[pts[i]])
            d2 = _sub(V[pts[(i + 1) % m]], V[pts[i]])
            n1, n2 = _norm(d1), _norm(d2)
            if n1 == 0.0 or n2 == 0.0:
                continue
            if (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) / (n1 * n2) > cos_thresh:
                del pts[i]
                changed = True
                break
    return pts


def join_rings(rings: list, V: list, target_n: int) -> list:
    comps = [list(r) for r in rings]
    while len(comps) > target_n:
        best_dist = float("inf")
        best = (0, 1, False, False)
        for a in range(len(comps)):
            for b in range(a + 1, len(comps)):
                for pa, flip_a in ((comps[a][0], True), (comps[a][-1], False)):
                    for pb, flip_b in ((comps[b][0], False), (comps[b][-1], True)):
                        d = _norm(_sub(V[pa], V[pb]))
                        if d < best_dist:
                            best_dist, best = d, (a, b, flip_a, flip_b)
        a, b, flip_a, flip_b = best
        ca = comps[a][::-1] if flip_a else comps[a]
        cb = comps[b][::-1] if flip_b else comps[b]
        comps = [c for k, c in enumerate(comps) if k not in (a, b)] + [ca + cb]
    return comps


def reduce_rings(rings: list, V: list, target_n) -> list:
    rings = sorted((r for r in rings if r), key=len, reverse=True)
    if target_n is None or len(rings) <= target_n:
        return rings
    return sorted(join_rings(rings, V, target_n), key=len, reverse=True)[:target_n]


def _vlist(vertices) -> list:
    return [tuple(r) for r in _p3(vertices).tolist()]


def order_boundary_rings(faces, vertices, seeds=None, target_n=None) -> list:
    graph = rims_touching(boundary_graph(open_boundary_edges(faces)), set(seeds or ()))
    return reduce_rings(walk_rings(graph), _vlist(vertices), target_n)


def _surviving(faces: np.ndarray, drop: set) -> np.ndarray:
    if not drop:
        return faces
    return faces[~np.any(np.isin(faces, np.fromiter(drop, dtype=np.int64, count=len(drop))), axis=1)]


def clean_open_boundary(faces, vertices, seeds, target_n=1, despike_cos=0.0, max_rounds=64):
    """(drop as a sorted list, rings)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = _vlist(vertices)
    drop: set = set()
    seed_set = set(seeds)
    for _ in range(max_rounds):
        graph = rims_touching(boundary_graph(open_boundary_edges(_surviving(f, drop))), seed_set)
        if not graph:
            return sorted(drop), []
        seed_set |= set(graph)
        bad = {v for v, ns in graph.items() if len(ns) != 2}
        if bad:
            drop |= bad
            continue
        rings = walk_rings(graph)
        spikes = {v for ring in rings for v in set(ring) - set(despike_ring(ring, V, despike_cos))}
        if not spikes:
            return sorted(drop), reduce_rings(rings, V, target_n)
        drop |= spikes
    graph = rims_touching(boundary_graph(open_boundary_edges(_surviving(f, drop))), seed_set)
    return sorted(drop), reduce_rings(walk_rings(graph), V, target_n)


# ---- remove / keep / export --------------------------------------------------------------------------------------------

def coord_to_idx(vertices) -> dict:
    return {t: i for i, t in enumerate(_vlist(vertices))}


def _filter(points, vertices) -> np.ndarray:
    s = set(_vlist(vertices))
    p = _p3(points)
    keep = [i for i, t in enumerate(_vlist(p)) if t in s]
    return p[keep]


def _store_boundary_rings(updated: dict, vertices: np.ndarray, rings: list) -> None:
    for key in [k for k in updated if k.startswith("boundary_points_")]:
        del updated[key]
    per_ring = [vertices[np.asarray(r, dtype=np.int64)] for r in rings]
    for n, pts in enumerate(per_ring, start=1):
        updated[f"boundary_points_{n}"] = pts
    updated["boundary_points"] = np.concatenate(per_ring) if per_ring else np.zeros((0, 3))


def _trim(results: dict, keys: list, keep_region: bool, target_boundaries: int):
    pts = [t for k in keys for t in _vlist(results.get(k, ()))]
    if not pts:
        return None
    v, f = results["mesh"]
    v = _p3(v)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    idx = coord_to_idx(v)
    hit = {idx[t] for t in pts if t in idx}
    if not hit:
        return None
    region = np.zeros(len(v), dtype=bool)
    region[list(hit)] = True
    keep_mask = region.copy() if keep_region else ~region
    face_keep = np.all(keep_mask[f], axis=1)
    # kept vertices sharing a face with a dropped one (the reference's adjacency test)
    mixed = f[~face_keep & np.any(keep_mask[f], axis=1)]
    seeds = set(mixed[keep_mask[mixed]].tolist())
    extra, rings = clean_open_boundary(f[face_keep], v, seeds, target_n=target_boundaries)
    if extra:
        keep_mask[np.asarray(extra, dtype=np.int64)] = False
        face_keep = np.all(keep_mask[f], axis=1)
    new_index = np.full(len(v), -1, dtype=np.int64)
    new_index[keep_mask] = np.arange(keep_mask.sum(), dtype=np.int64)
    new_v = v[keep_mask]
    updated = dict(results)
    updated["mesh"] = (new_v, new_index[f[face_keep]])
    _store_boundary_rings(updated, v, rings)
    return updated


def remove_labeled_points_from_mesh(results: dict, region_keys="anomalous_points", target_boundaries=1) -> dict:
    keys = [region_keys] if isinstance(region_keys, str) else list(region_keys)
    updated = _trim(results, keys, False, target_boundaries)
    if updated is None:
        return results
    for key in keys:
        updated[key] = np.zeros((0, 3))
    for key in TRIM_KEYS:
        if key in updated and key not in keys:
            updated[key] = _filter(updated[key], updated["mesh"][0])
    return updated


def keep_labeled_points_from_mesh(results: dict, region_key, target_boundaries=1) -> dict:
    keys = [region_key] if isinstance(region_key, str) else list(region_key)
    updated = _trim(results, keys, True, target_boundaries)
    if updated is None:
        return results
    for key in TRIM_KEYS + tuple(keys):
        if key in updated:
            updated[key] = _filter(updated[key], updated["mesh"][0])
    return updated


def extract_region_with_border_faces(mesh, region_points):
    v, f = mesh
    v = _p3(v)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    idx = coord_to_idx(v)
    keep = np.array([idx[t] for t in _vlist(region_points) if t in idx], dtype=np.int64)
    if keep.size == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    sel = f[np.isin(f, keep).any(axis=1)]
    used = np.unique(sel)
    remap = np.full(len(v), -1, dtype=np.int64)
    remap[used] = np.arange(len(used), dtype=np.int64)
    return v[used], remap[sel]


def section_mesh(results: dict, type: str):
    """The mesh export_section_stl writes for ``type``."""
    if type == "all":
        return results["mesh"]
    if type == "aorta":
        return keep_labeled_points_from_mesh(results, ["aorta_points", "rca_removed_points",
                                                       "lca_removed_points"])["mesh"]
    return extract_region_with_border_faces(results["mesh"], results.get(f"{type}_points", ()))


def read_stl(path):
    """(normals (F, 3) f32, triangles (F, 3, 3) f32) of a binary STL."""
    with open(path, "rb") as fh:
        data = fh.read()
    n = int(np.frombuffer(data, dtype="<u4", count=1, offset=80)[0])
    assert len(data) == 84 + 50 * n
    rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=n,
                        offset=84)
    return rec["n"].copy(), rec["v"].copy()
