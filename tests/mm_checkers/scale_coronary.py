"""Plain Python / numpy restatement of the reference's mesh morphing: centerline_based_diameter_morphing
(src/ccta/adjust_mesh/scale_coronary.rs:218-260), keep_largest_connected_component (src/ccta/binding/ccta_py.rs:541-580
with connected_components, label_coronary.rs:428-455), label_anomalous_region (multimodars/ccta/labeling.py:283-389),
scale_region_centerline_morphing / sync_results_to_mesh (multimodars/ccta/scaling.py:16-80, 301-351) and scale
(multimodars/ccta/__init__.py:171-258).  The parity reference of the morphing tests; nothing here touches the device or
the native library.

Point lists are lists of tuples of Python floats, so set membership and dict lookups compare by value exactly as the
reference's Python does (-0.0 equals 0.0; a NaN coordinate equals nothing, the floats being distinct objects).  Float
arithmetic is Python's IEEE f64 in the reference's operation order (no fused multiply-add), so the results are bit-exact
restatements."""
from __future__ import annotations

import math
import sys

import numpy as np

DBL_MAX = sys.float_info.max


def tuples(a) -> list:
    """(n, 3) rows as a list of tuples of fresh Python floats."""
    return [tuple(float(c) for c in r) for r in np.asarray(a, dtype=np.float64).reshape(-1, 3)]


# ---- centerline_based_diameter_morphing (scale_coronary.rs:218-260) ----------------------------------------------

def closest_index(cl, p) -> int:
    """find_closest_centerline_point_optimized (:245-260): best = f64::MAX, index 0; c_j replaces it iff d_j < best."""
    best, k = DBL_MAX, 0
    for j, c in enumerate(cl):
        dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
        d = dx * dx + dy * dy + dz * dz
        if d < best:
            best, k = d, j
    return k


def nearest_indices(cl, pts) -> np.ndarray:
    """closest_index for many points at once (elementwise numpy f64, same operations): the first index of the smallest
    d_j among those below f64::MAX, else 0."""
    c, p = np.asarray(cl, dtype=np.float64).reshape(-1, 3), np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(p.shape[0], dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(0, p.shape[0], 1024):
            q = p[s:s + 1024]
            dx, dy, dz = q[:, None, 0] - c[None, :, 0], q[:, None, 1] - c[None, :, 1], q[:, None, 2] - c[None, :, 2]
            d = dx * dx + dy * dy + dz * dz
            d = np.where(d < DBL_MAX, d, np.inf)
            k = np.argmin(d, axis=1)
            out[s:s + 1024] = np.where(np.isfinite(d[np.arange(q.shape[0]), k]), k, 0)
    return out


def move(p, c, adj):
    """:226-239 with try_normalize(0.0): v = p - c, n = |v|; p + (v / n) * adj if n > 0, else p.  A NaN n keeps p (the
    rule of the package's host and device paths; nalgebra's `n <= 0` test would give NaN there)."""
    vx, vy, vz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    n = math.sqrt(vx * vx + vy * vy + vz * vz)
    if n > 0.0:
        return (p[0] + (vx / n) * adj, p[1] + (vy / n) * adj, p[2] + (vz / n) * adj)
    return tuple(p)


def diameter_morphing(cl, points, adj, nearest=None):
    """centerline_based_diameter_morphing -> (moved points, nearest indices).  ``nearest``: precomputed indices."""
    cl = tuples(cl)
    pts = [tuple(float(c) for c in p) for p in points]
    idx = [closest_index(cl, p) for p in pts] if nearest is None else [int(k) for k in nearest]
    return [move(p, cl[k], float(adj)) for p, k in zip(pts, idx)], idx


# ---- keep_largest_connected_component (ccta_py.rs:541-580) --------------------------------------------------------

def bits(p):
    """bits_key (label_coronary.rs:293): the bit patterns of the three coordinates."""
    return tuple(int(x) for x in np.asarray(p, dtype=np.float64).view(np.uint64))


def adjacency(faces):
    """build_adjacency_map (ccta_py.rs:507-525)."""
    adj = {}
    for a, b, c in faces:
        for u, v in ((a, b), (b, c), (c, a)):
            adj.setdefault(u, set()).add(v)
            adj.setdefault(v, set()).add(u)
    return adj


def connected_components(adj, subset):
    """label_coronary.rs:428-455, walked from the smallest vertex upwards (the reference walks in hash order)."""
    remaining, comps = set(subset), []
    for s in sorted(subset):
        if s not in remaining:
            continue
        comp, stack = set(), [s]
        while stack:
            i = stack.pop()
            if i in comp:
                continue
            comp.add(i)
            stack.extend(n for n in adj.get(i, ()) if n in remaining and n not in comp)
        remaining -= comp
        comps.append(comp)
    return comps


def keep_largest_connected_component(vertices, faces, points):
    """Fewer than 2 points or none matching a vertex (bit for bit): the points unchanged.  Else the vertices of the
    largest component, ascending; of equally large ones the one holding the smallest vertex index."""
    points = [tuple(float(c) for c in p) for p in points]
    if len(points) < 2:
        return points
    vertices = tuples(vertices)
    idx = {bits(v): i for i, v in enumerate(vertices)}
    sub = {idx[bits(p)] for p in points if bits(p) in idx}
    if not sub:
        return points
    comps = connected_components(adjacency([tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]), sub)
    best = comps[0]
    for c in comps[1:]:
        if len(c) > len(best):
            best = c
    return [vertices[i] for i in sorted(best)]


# ---- labeling.py:283-389, scaling.py:16-80 / 301-351, __init__.py:171-258 ----------------------------------------

def label_anomalous_region(split, vertices, faces, results, results_key="rca_points"):
    """labeling.py:283-389 from the (proximal, distal, anomalous) split of find_points_by_cl_region (checked on its
    own elsewhere).  Mutates and returns ``results`` (lists of tuples)."""
    raw = [tuples(x) for x in split]
    kept = [keep_largest_connected_component(vertices, faces, r) for r in raw]
    dropped = set()
    for r, k in zip(raw, kept):
        dropped |= set(r) - set(k)
    if dropped:
        results[results_key] = [p for p in results[results_key] if p not in dropped]
    results["proximal_points"], results["distal_points"], results["anomalous_points"] = kept
    all_coronary = (set(results.get("rca_points", [])) | set(results.get("lca_points", [])) | set(kept[0]) |
                    set(kept[1]) | set(kept[2]))
    results["aorta_points"] = [v for v in tuples(vertices) if v not in all_coronary]
    return results


def scale_region_centerline_morphing(vertices, region_points, cl, adj):
    """scaling.py:16-80 on a vertex list -> the new vertex list."""
    out = tuples(vertices)
    region = set(region_points)
    sel = [i for i, v in enumerate(out) if v in region]
    if not sel:
        return out
    cl = tuples(cl)
    for i in sel:
        out[i] = move(out[i], cl[closest_index(cl, out[i])], float(adj))
    return out


def sync_results_to_mesh(results, old_vertices, new_vertices):
    """scaling.py:301-351 on vertex lists; "mesh" is set to the new vertex list."""
    old_coord_to_idx = {v: i for i, v in enumerate(tuples(old_vertices))}
    new = tuples(new_vertices)
    updated = dict(results)
    updated["mesh"] = new
    for key in ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "lca_removed_points",
                "proximal_points", "distal_points", "anomalous_points", "boundary_points",
                *sorted(k for k in updated if k.startswith("boundary_points_"))):
        if key not in updated or not updated[key]:
            continue
        indices = [old_coord_to_idx.get(tuple(p)) for p in updated[key]]
        updated[key] = [new[i] for i in indices if i is not None]
    return updated


def scale_rounds(results, cl_vessel, cl_aorta, prox_scaling, distal_scaling, aortic_scaling):
    """The three morph + sync rounds of __init__.py:227-256 given the three scalings; results["mesh"] is a vertex list."""
    new = scale_region_centerline_morphing(results["mesh"], results["distal_points"], cl_vessel, distal_scaling)
    results = sync_results_to_mesh(results, results["mesh"], new)
    region = list(results["aorta_points"]) + list(results["rca_removed_points"])
    new = scale_region_centerline_morphing(results["mesh"], region, cl_aorta, aortic_scaling)
    results = sync_results_to_mesh(results, results["mesh"], new)
    new = scale_region_centerline_morphing(results["mesh"], results["proximal_points"], cl_vessel, prox_scaling)
    return sync_results_to_mesh(results, results["mesh"], new)
