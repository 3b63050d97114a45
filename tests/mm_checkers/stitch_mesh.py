"""Numpy / plain-Python restatement of the CCTA stitching (multimodars/ccta/stitching.py:69-107, 355-481, 1148-1334,
multimodars/_converters.py:1018-1085, src/ccta/binding/ccta_py.rs:596-700): the yardstick for csrc/mm_weld_kernels.hip
and csrc/mm_stitch.cpp.  trimesh is not available, so merge_vertices / unique_faces / fix_inversion are restated from
their documented behaviour; the rules below are this package's definition (include/mm_ccta.h states the same).

Assembly of concatenated parts (face indices local to their part):

* weld: only vertices some face names take part, the others are dropped.  key = rint(c * 10^digits) per coordinate, one
  f64 multiply, half to even, as an integer triple (-0.0 and 0.0 share a key).  A vertex with a non-finite coordinate
  or a scaled magnitude at or above 2^62 matches nothing.  Equal keys become the vertex with the smallest index in
  concatenated order, its coordinates bit for bit; survivors keep concatenated order.
* faces: remapped through the weld; a face with a repeated index is dropped; of faces with the same vertex set the one
  with the smallest index stays with its own corner order; survivors keep input order.
* winding: two faces are adjacent when they share an undirected edge that exactly two faces own.  A plain BFS from the
  smallest unvisited face index: the start keeps its corner order, a neighbour first reached over an edge that both
  traverse in the same direction (after the current face's own flip) is reversed (a, b, c) -> (c, b, a).  For an
  orientable component the result does not depend on the visiting order.  conflicts = the edges owned twice whose two
  faces still traverse them in the same direction (0 for orientable input).
* inversion: t_f = (p0x cx + p0y cy) + p0z cz with c = p1 x p2 = (p1y p2z - p1z p2y, p1z p2x - p1x p2z,
  p1x p2y - p1y p2x), every operation rounded on its own; the sum is the adjacent-pair tree over the faces in output
  order padded with +0.0 to a power of two; volume = sum / 6; volume < 0 reverses every face.

The seam: sums run in index order, norms are sqrt((x x + y y) + z z), minima are first minima (strict <).
"""
from collections import deque

import numpy as np


# ---- assembly -----------------------------------------------------------------------------------------------------------

def pair_tree_sum(a) -> float:
    a = np.asarray(a, dtype=np.float64)
    n = 1
    while n < a.shape[0]:
        n *= 2
    a = np.concatenate([a, np.zeros(n - a.shape[0])])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


def weld(v, f, digits=3):
    """(rep, n_unreferenced): rep[i] = the vertex i is welded into, -1 for an unreferenced vertex."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    nv = v.shape[0]
    ref = np.zeros(nv, dtype=bool)
    ref[np.asarray(f, dtype=np.int64).ravel()] = True
    s = v * float(10 ** digits)
    with np.errstate(invalid="ignore"):
        has_key = ref & (np.abs(s) < 2.0 ** 62).all(axis=1)
    rep = np.where(ref, np.arange(nv), -1)
    idx = np.nonzero(has_key)[0]
    if idx.size:
        keys = np.rint(s[idx]).astype(np.int64)
        _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        rep[idx] = idx[first[np.asarray(inv).ravel()]]
    return rep, int((~ref).sum())


def face_adjacency(f):
    """The edges owned by exactly two faces as (fa, da, fb, db) rows (d = 1: traversed from the smaller to the larger
    index), and the numbers of edges owned once and more than twice."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nf = f.shape[0]
    u = f.ravel()
    w = f[:, [1, 2, 0]].ravel()
    key = (np.minimum(u, w) << 32) | np.maximum(u, w)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0] if ks.size else np.zeros(0, dtype=np.int64)
    count = np.diff(np.concatenate([start, [ks.size]]))
    two = start[count == 2]
    ea, eb = order[two], order[two + 1]
    d = (u < w).astype(np.int64)
    pairs = np.stack([ea // 3, d[ea], eb // 3, d[eb]], axis=1) if two.size else np.zeros((0, 4), dtype=np.int64)
    del nf
    return pairs, int((count == 1).sum()), int((count > 2).sum())


def fix_winding(f):
    """(faces, flipped, conflicts): the BFS of the module docstring."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3).copy()
    nf = f.shape[0]
    pairs, _, _ = face_adjacency(f)
    nbr = [[] for _ in range(nf)]
    for fa, da, fb, db in pairs.tolist():
        same = 1 if da == db else 0
        nbr[fa].append((fb, same))
        nbr[fb].append((fa, same))
    flip = [0] * nf
    seen = [False] * nf
    for start in range(nf):
        if seen[start]:
            continue
        seen[start] = True
        q = deque([start])
        while q:
            cur = q.popleft()
            for nb, same in nbr[cur]:
                if seen[nb]:
                    continue
                seen[nb] = True
                flip[nb] = flip[cur] ^ same
                q.append(nb)
    flip = np.asarray(flip, dtype=np.int64).reshape(-1)
    conflicts = 0
    if pairs.shape[0]:
        conflicts = int(((pairs[:, 1] ^ flip[pairs[:, 0]]) == (pairs[:, 3] ^ flip[pairs[:, 2]])).sum())
    m = flip.astype(bool)
    f[m] = f[m][:, ::-1]
    return f, m, conflicts


def volume_terms(v, f):
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cx = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    cy = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    cz = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    return (p0[:, 0] * cx + p0[:, 1] * cy) + p0[:, 2] * cz


def assemble(parts, digits=3, fix_wind=True, fix_inv=True):
    """(vertices, faces, report) of the module docstring's assembly; winding_rounds is not restated."""
    vs = [np.asarray(p[0], dtype=np.float64).reshape(-1, 3) for p in parts]
    fs = [np.asarray(p[1], dtype=np.int64).reshape(-1, 3) for p in parts]
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in vs])]).astype(np.int64)
    v = np.concatenate(vs) if vs else np.zeros((0, 3))
    f = np.concatenate([a + o for a, o in zip(fs, off[:-1])]) if fs else np.zeros((0, 3), dtype=np.int64)
    report = dict.fromkeys(("n_vertices", "n_faces", "n_welded_vertices", "n_unreferenced_vertices",
                            "n_degenerate_faces", "n_duplicate_faces", "n_flipped_faces", "n_winding_conflicts",
                            "n_open_edges", "n_nonmanifold_edges", "inverted"), 0)
    report["volume"] = 0.0
    if f.shape[0] == 0:
        report["n_unreferenced_vertices"] = v.shape[0]
        report["watertight"] = True
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), report
    rep, n_unref = weld(v, f, digits)
    keep = rep == np.arange(v.shape[0])
    new = np.cumsum(keep) - 1
    g = new[rep[f]]
    degenerate = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    idx = np.nonzero(~degenerate)[0]
    _, first = np.unique(np.sort(g[idx], axis=1), axis=0, return_index=True)
    kept = np.sort(idx[first])
    out_v, out_f = v[keep], g[kept]
    report.update(n_vertices=int(keep.sum()), n_faces=int(kept.size), n_unreferenced_vertices=n_unref,
                  n_welded_vertices=int(v.shape[0] - n_unref - keep.sum()), n_degenerate_faces=int(degenerate.sum()),
                  n_duplicate_faces=int(idx.size - kept.size))
    if fix_wind:
        out_f, flipped, conflicts = fix_winding(out_f)
        report.update(n_flipped_faces=int(flipped.sum()), n_winding_conflicts=conflicts)
    else:
        pairs, _, _ = face_adjacency(out_f)
        report["n_winding_conflicts"] = int((pairs[:, 1] == pairs[:, 3]).sum())
    _, n_open, n_nonmanifold = face_adjacency(out_f)
    report.update(n_open_edges=n_open, n_nonmanifold_edges=n_nonmanifold)
    if fix_inv:
        with np.errstate(all="ignore"):
            volume = pair_tree_sum(volume_terms(out_v, out_f)) / 6.0
        report["volume"] = volume
        if volume < 0.0:
            report["inverted"] = 1
            out_f = out_f[:, ::-1]
    report["watertight"] = n_open == 0 and n_nonmanifold == 0
    return out_v, np.ascontiguousarray(out_f), report


# ---- the seam -----------------------------------------------------------------------------------------------------------

def _norm(d):
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def _centroid(ring):
    s = np.zeros(3)
    for p in np.asarray(ring, dtype=np.float64).reshape(-1, 3):
        s = s + p
    return s / float(len(ring))


def assign_rings_to_ends(rings, prox, dist):
    cs = [_centroid(r) for r in rings]
    prox, dist = np.asarray(prox, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    best_cost, best = float("inf"), (0, 1)
    for i in range(len(rings)):
        for j in range(len(rings)):
            if i == j:
                continue
            cost = _norm(cs[i] - prox) + _norm(cs[j] - dist)
            if cost < best_cost:
                best_cost, best = cost, (i, j)
    return best[0], best[1], [k for k in range(len(rings)) if k not in best]


def ring_start(ring, mode, iv_pt=None):
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 3)
    if mode == "highest_z":
        return int(np.argmax(ring[:, 2]))
    q = np.asarray(iv_pt, dtype=np.float64).reshape(3)
    return int(np.argmin([_norm(p - q) for p in ring]))


def rotate(ring, k):
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([ring[k:], ring[:k]])


def reversed_ring(ring):
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([ring[:1], ring[:0:-1]])


def direction_by_distance(ring, iv, step):
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 3)
    sub = np.asarray(iv, dtype=np.float64).reshape(-1, 3)[0::step][:len(ring)]

    def total(b):
        s = 0.0
        for i in range(min(len(b), len(sub))):
            s += _norm(b[i] - sub[i])
        return s

    rev = reversed_ring(ring)
    return rev if total(rev) < total(ring) else ring


def newell_normal(pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    nx = ny = nz = 0.0
    for i in range(n):
        c, x = pts[i], pts[(i + 1) % n]
        nx += (c[1] - x[1]) * (c[2] + x[2])
        ny += (c[2] - x[2]) * (c[0] + x[0])
        nz += (c[0] - x[0]) * (c[1] + x[1])
    length = _norm((nx, ny, nz))
    return np.array([nx / length, ny / length, nz / length]) if length > 1e-10 else np.array([0.0, 0.0, 1.0])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot(a, b):
    return float((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def signed_area_projected(pts, normal):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    ref = np.array([1.0, 0.0, 0.0]) if abs(normal[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = _cross(normal, ref)
    u = u / _norm(u)
    w = _cross(normal, u)
    n = len(pts)
    s = 0.0
    for i in range(n):
        a, b = pts[i], pts[(i + 1) % n]
        s += _dot(a, u) * _dot(b, w) - _dot(b, u) * _dot(a, w)
    return 0.5 * s


def direction_by_winding(ring, iv):
    return reversed_ring(ring) if signed_area_projected(ring, newell_normal(iv)) < 0 else \
        np.asarray(ring, dtype=np.float64).reshape(-1, 3)


def stitch_rings(boundary, iv, outward=None):
    b = np.asarray(boundary, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(iv, dtype=np.float64).reshape(-1, 3)
    n_b, n_iv = len(b), len(q)
    if n_b < 3 or n_iv < 3:
        raise ValueError("Need at least 3 points per ring to stitch")
    v = np.concatenate([b, q])
    faces = []
    i = j = 0
    while i < n_b or j < n_iv:
        if j >= n_iv or (i < n_b and (i + 1) / n_b <= (j + 1) / n_iv):
            faces.append((i % n_b, (i + 1) % n_b, n_b + j % n_iv))
            i += 1
        else:
            faces.append((i % n_b, n_b + (j + 1) % n_iv, n_b + j % n_iv))
            j += 1
    faces = np.asarray(faces, dtype=np.int64)
    if outward is not None:
        s, valid = np.zeros(3), 0
        with np.errstate(all="ignore"):
            for a, c, d in faces:
                n = _cross(v[c] - v[a], v[d] - v[a])
                u = n / _norm(n)
                if np.isfinite(u).all():
                    s = s + u
                    valid += 1
        if valid and _dot(s / float(valid), np.asarray(outward, dtype=np.float64)) < 0:
            faces = faces[:, ::-1]
    return v, np.ascontiguousarray(faces)


def tube(contours, centroid0):
    cs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in contours]
    n = len(cs[0])
    v = np.concatenate(cs)
    faces = []
    for i in range(len(cs) - 1):
        for j in range(n):
            j1 = (j + 1) % n
            a, b, c, d = i * n + j, i * n + j1, (i + 1) * n + j1, (i + 1) * n + j
            faces.append((a, b, d))
            faces.append((b, c, d))
    faces = np.asarray(faces, dtype=np.int64)
    p0, p1, p2 = v[faces[0]]
    centre = np.array([((p0[k] + p1[k]) + p2[k]) / 3.0 for k in range(3)])
    if _dot(_cross(p1 - p0, p2 - p0), centre - np.asarray(centroid0, dtype=np.float64)) < 0:
        faces = faces[:, ::-1]
    return v, np.ascontiguousarray(faces)


def downsample(pts, n):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if len(pts) <= n:
        return pts
    step = len(pts) / float(n)
    return pts[[int(i * step) for i in range(n)]]


def stitch_parts(frames, centroids, lumen_centroid0, rings, mesh, n_points=100, prox_mode="nearest_iv",
                 dist_mode="nearest_iv"):
    """stitch_ccta_to_intravascular without the rim conditioning, up to the four parts that are assembled: returns
    (parts, prox_ring, dist_ring)."""
    frames = [downsample(f, n_points) for f in frames]
    prox_c, dist_c = np.asarray(centroids[0], dtype=np.float64), np.asarray(centroids[-1], dtype=np.float64)
    i, j, _ = assign_rings_to_ends(rings, prox_c, dist_c)
    prox_b, dist_b = np.asarray(rings[i], dtype=np.float64), np.asarray(rings[j], dtype=np.float64)
    prox_step = max(1, len(frames[0]) // len(prox_b))
    dist_step = max(1, len(frames[-1]) // len(dist_b))
    if "highest_z" in (prox_mode, dist_mode):
        z = frames[0][:, 2]
        shift = max(k for k in range(len(z)) if z[k] == z.max())
        frames = [rotate(f, shift % len(f)) for f in frames]
    out = []
    for ring, iv, mode, step in ((prox_b, frames[0], prox_mode, prox_step), (dist_b, frames[-1], dist_mode, dist_step)):
        ring = rotate(ring, ring_start(ring, mode, iv[0]))
        out.append(direction_by_winding(ring, iv) if mode == "highest_z" else direction_by_distance(ring, iv, step))
    prox_b, dist_b = out
    parts = [mesh, stitch_rings(prox_b, frames[0], prox_c - dist_c), stitch_rings(dist_b, frames[-1], dist_c - prox_c),
             tube(frames, lumen_centroid0)]
    return parts, prox_b, dist_b
