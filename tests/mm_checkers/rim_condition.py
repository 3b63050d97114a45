"""Checker for the rim conditioning in front of the CCTA stitch: a plain numpy / Python restatement of
multimodars/ccta/stitching.py:484-1064, written from the behaviour.  A mesh is ``(vertices (V, 3) f64, faces (F, 3)
int)``, a ring a list of ``(x, y, z)`` tuples or an ``(n, 3)`` array.

Ring stages use numpy as the reference does (np.linalg.svd, np.median, np.searchsorted, np.linspace).  The three
mesh-wide stages -- locating points (the ``{tuple(v): i}`` dicts of :826 and :873), the layer push (:1014-1064) and the
fans of the densification (:894-962) -- spell their arithmetic out as scalar f64 operations in a fixed order (no np.dot,
no np.linalg.norm, whose summation order belongs to BLAS), so that the device can be compared with them bit for bit.

Where the reference leaves an order to CPython it is fixed here, and the product follows the same rule:
  * _densify_boundary walks a Python ``set`` of touched faces (:927): here in ascending face index.  Output faces are the
    untouched faces in input order, then the fans in ascending source-face order, each fan in the reference's own order
    (:938-950).  Appended vertices are the inserted rim points in ring-edge order (:897-905), then one centroid per
    apex-less face in ascending face order.
  * ``coord_to_idx`` is a dict: the last vertex with a coordinate wins, keys compare by value (-0.0 == 0.0), a row with a
    NaN equals nothing.
  * a ring that names one mesh vertex twice raises ValueError (the reference would overwrite ``inserted[(a, b)]``); so
    does a ring that gives one vertex two different targets in write_ring_to_mesh (the reference keeps the last).
  * the reference's printed warnings are fields of the report; nothing prints.
"""
import math

import numpy as np


def _arr(points):
    return np.asarray(points, dtype=np.float64).reshape(-1, 3)


# ---- ring stages (numpy, as the reference) ------------------------------------------------------------------------------

def plane_normal_svd(pts):
    """:965-969."""
    pts = _arr(pts)
    _, _, vt = np.linalg.svd(pts - pts.mean(axis=0), full_matrices=False)
    return vt[-1]


def singular_gap(pts):
    """(s2 - s3) / s1 of the centred ring: how well its plane is defined."""
    pts = _arr(pts)
    s = np.linalg.svd(pts - pts.mean(axis=0), compute_uv=False)
    return float((s[1] - s[2]) / s[0]) if s[0] > 0 else 0.0


def project_to_best_fit_plane(points):
    """:648-665."""
    pts = _arr(points)
    if len(pts) < 3:
        return pts.copy()
    centroid = pts.mean(axis=0)
    normal = plane_normal_svd(pts)
    distances = (pts - centroid) @ normal
    return pts - np.outer(distances, normal)


def smooth_ring_laplacian(points, iterations=5, alpha=0.5):
    """:668-693."""
    pts = _arr(points).copy()
    if len(pts) < 3:
        return pts
    for _ in range(iterations):
        prev = pts.copy()
        neighbor_avg = (np.roll(prev, 1, axis=0) + np.roll(prev, -1, axis=0)) / 2.0
        pts = alpha * prev + (1.0 - alpha) * neighbor_avg
    return pts


def ring_calibre(pts):
    """:696-703."""
    pts = _arr(pts)
    return float(np.linalg.norm(pts - pts.mean(axis=0), axis=1).mean())


def smooth_ring_preserving_size(points, iterations=5, alpha=0.5):
    """:706-739."""
    pts = _arr(points)
    if len(pts) < 3:
        return pts.copy()
    before = ring_calibre(pts)
    smoothed = smooth_ring_laplacian(pts, iterations, alpha)
    after = ring_calibre(smoothed)
    if before <= 0.0 or after <= 0.0:
        return smoothed
    centroid = smoothed.mean(axis=0)
    return centroid + (smoothed - centroid) * (before / after)


def redistribute_ring_evenly(points, n_out=None):
    """:742-772."""
    pts = _arr(points)
    count = len(pts) if n_out is None else n_out
    if len(pts) < 3 or count < 3:
        return pts.copy()
    loop = np.vstack([pts, pts[:1]])
    seg_len = np.linalg.norm(np.diff(loop, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg_len)])
    perimeter = float(cum[-1])
    if perimeter <= 0.0:
        return pts.copy()
    out = []
    for target in np.linspace(0.0, perimeter, count, endpoint=False):
        k = min(int(np.searchsorted(cum, target, side="right") - 1), len(seg_len) - 1)
        span = float(seg_len[k])
        frac = 0.0 if span <= 0.0 else (float(target) - float(cum[k])) / span
        out.append(loop[k] + frac * (loop[k + 1] - loop[k]))
    return np.array(out)


def project_onto_plane(points, origin, normal):
    """:775-782."""
    pts = _arr(points)
    origin, normal = np.asarray(origin, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    return pts - np.outer((pts - origin) @ normal, normal)


def shift_plane_clear_of(origin, normal, points, outward, overshoot):
    """:785-813: (shifted origin, oriented unit normal, distance moved)."""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    if float(np.dot(n, np.asarray(outward, dtype=np.float64))) < 0.0:
        n = -n
    o = np.asarray(origin, dtype=np.float64)
    signed = (_arr(points) - o) @ n
    worst = float(signed.max())
    if worst <= -overshoot:
        return o, n, 0.0
    shift = worst + overshoot
    return o + shift * n, n, shift


def angle_between_planes_deg(n1, n2):
    """:972-975."""
    cos = np.clip(np.abs(np.dot(n1, n2)), 0.0, 1.0)
    return float(np.degrees(np.arccos(cos)))


def clamp_to_plane(points, plane_origin, plane_normal, overshoot=0.0):
    """:978-1011."""
    pts = _arr(points).copy()
    plane_origin = np.asarray(plane_origin, dtype=np.float64)
    plane_normal = np.asarray(plane_normal, dtype=np.float64)
    dists = (pts - plane_origin) @ plane_normal
    correct_sign = np.sign(np.median(dists))
    wrong = (np.sign(dists) != correct_sign) & (dists != 0.0)
    pts[wrong] -= np.outer(dists[wrong], plane_normal)
    if overshoot > 0.0:
        dists2 = (pts - plane_origin) @ plane_normal
        signed_dist = correct_sign * dists2
        too_close = signed_dist < overshoot
        deficit = overshoot - signed_dist[too_close]
        pts[too_close] += np.outer(deficit * correct_sign, plane_normal)
    return pts


def densify_plan(ring, target_n):
    """The insert counts of :862-892 and how clear the cut of the length sort is: ``(counts, status, gap)`` with status
    0 nothing to insert, 1 a plan, 2 the ring is above the target, and gap the difference between the shortest length
    that gets one more point and the longest that does not (inf where the remainder is 0)."""
    pts = _arr(ring)
    n = len(pts)
    extra = target_n - n
    if n < 3 or extra <= 0:
        return [0] * n, (2 if extra < 0 else 0), math.inf
    lengths = [float(np.linalg.norm(pts[(i + 1) % n] - pts[i])) for i in range(n)]
    counts = [extra // n] * n
    order = sorted(range(n), key=lambda k: lengths[k], reverse=True)
    cut = extra % n
    for e in order[:cut]:
        counts[e] += 1
    gap = lengths[order[cut - 1]] - lengths[order[cut]] if 0 < cut < n else math.inf
    return counts, 1, gap


# ---- mesh-wide stages (scalar f64, fixed order) --------------------------------------------------------------------------

def _key(p):
    """A dict key that compares as the reference's ``tuple(v)`` does; None for a row with a NaN (equal to nothing)."""
    t = tuple(float(x) for x in p)
    if any(x != x for x in t):
        return None
    return tuple(0.0 if x == 0.0 else x for x in t)


def locate_points(vertices, points):
    """:826-830, :873-874: for every point the index of the last vertex equal to it by value, -1 without one."""
    coord_to_idx = {}
    for i, v in enumerate(_arr(vertices)):
        k = _key(v)
        if k is not None:
            coord_to_idx[k] = i
    out = []
    for p in _arr(points):
        k = _key(p)
        out.append(coord_to_idx.get(k, -1) if k is not None else -1)
    return np.array(out, dtype=np.int64)


def write_ring_to_mesh(mesh, old_pts, new_pts):
    """:816-834: ``((vertices, faces), moved)``, moved the sorted distinct vertex indices written."""
    v, f = mesh
    verts = np.array(v, dtype=np.float64)
    idx = locate_points(verts, old_pts)
    new = _arr(new_pts)
    target = {}
    for k, i in enumerate(idx.tolist()):
        if i < 0:
            continue
        if i in target and target[i].tobytes() != new[k].tobytes():
            raise ValueError("two ring points with different targets sit on one mesh vertex")
        target[i] = new[k]
    for i, p in target.items():
        verts[i] = p
    return (verts, f), sorted(target)


def vertex_layers(faces, nv, seeds, n_rings):
    """The breadth-first layers of :1034-1062 over build_adjacency_map's graph: ``(layer, rings_run)``; layer[v] = 0 for
    a seed, k for a vertex first reached in ring k, -1 otherwise; rings_run counts the rings entered (the run ends
    behind one that finds nothing)."""
    adj = {}
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            adj.setdefault(x, set()).add(y)
            adj.setdefault(y, set()).add(x)
    layer = np.full(nv, -1, dtype=np.int32)
    frontier = set(int(s) for s in seeds)
    for s in frontier:
        layer[s] = 0
    rings_run = 0
    if not frontier:
        return layer, 0
    for ring in range(1, n_rings + 1):
        rings_run += 1
        nxt = set()
        for vi in frontier:
            for nb in adj.get(vi, ()):
                if layer[nb] == -1:
                    nxt.add(nb)
        for vi in nxt:
            layer[vi] = ring
        frontier = nxt
        if not frontier:
            break
    return layer, rings_run


def push_vertex(p, layer, origin, normal, step):
    """:1049-1057 for one vertex, in the order the header states; None where the vertex stays."""
    px, py, pz = (float(x) for x in p)
    ox, oy, oz = (float(x) for x in origin)
    nx, ny, nz = (float(x) for x in normal)
    d = ((px - ox) * nx + (py - oy) * ny) + (pz - oz) * nz
    rx, ry, rz = (px - d * nx) - ox, (py - d * ny) - oy, (pz - d * nz) - oz
    rn = math.sqrt((rx * rx + ry * ry) + rz * rz)
    if rn < 1e-10:
        return None, rn
    s = (float(layer) * float(step)) / rn
    return (px + s * rx, py + s * ry, pz + s * rz), rn


def enforce_layer_gap_from_plane(mesh, seeds, plane_origin, plane_normal, layer_step_mm=0.1, n_rings=2):
    """:1014-1064: ``((vertices, faces), layer, rings_run, r_norms)``."""
    v, f = mesh
    verts = np.array(v, dtype=np.float64)
    layer, rings_run = vertex_layers(f, len(verts), seeds, n_rings)
    r_norms = []
    for vi in np.nonzero(layer >= 1)[0].tolist():
        q, rn = push_vertex(verts[vi], int(layer[vi]), plane_origin, plane_normal, layer_step_mm)
        r_norms.append(rn)
        if q is not None:
            verts[vi] = q
    return (verts, f), layer, rings_run, r_norms


def split_rim_edges(mesh, ring_idx, counts):
    """The mesh side of :894-962 for a ring given as vertex indices: ``((vertices, faces), dense ring indices, info)``
    with info = {n_inserted, n_fanned_faces, n_centroid_fans}."""
    v, f = mesh
    verts = np.array(v, dtype=np.float64)
    faces = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    idx = [int(i) for i in ring_idx]
    n = len(idx)
    if len(set(idx)) != n:
        raise ValueError("the ring names one mesh vertex twice")
    nv = len(verts)
    edges = [(idx[i], idx[(i + 1) % n]) for i in range(n)]
    new_pts, inserted, next_idx = [], {}, nv
    for (a, b), count in zip(edges, counts):
        ids = []
        for j in range(1, int(count) + 1):
            t = j / (count + 1)
            new_pts.append([float(verts[a][c]) + t * (float(verts[b][c]) - float(verts[a][c])) for c in range(3)])
            ids.append(next_idx)
            next_idx += 1
        inserted[(a, b)] = ids
    all_v = [list(map(float, p)) for p in verts] + new_pts

    def points_on(a, b):
        if inserted.get((a, b)):
            return inserted[(a, b)]
        if inserted.get((b, a)):
            return list(reversed(inserted[(b, a)]))
        return []

    split = {frozenset(e) for e, ids in inserted.items() if ids}
    touched = [fi for fi, (a, b, c) in enumerate(faces.tolist())
               if frozenset((a, b)) in split or frozenset((b, c)) in split or frozenset((c, a)) in split]
    touched_set = set(touched)
    out_faces = [tuple(t) for fi, t in enumerate(faces.tolist()) if fi not in touched_set]
    n_centroid = 0
    for fi in touched:                                                   # ascending: the fixed order
        a0, b0, c0 = faces[fi].tolist()
        poly, on_sub = [], set()
        for a, b in ((a0, b0), (b0, c0), (c0, a0)):
            poly.append(a)
            mids = points_on(a, b)
            poly.extend(mids)
            if mids:
                on_sub.update((a, b))
        apex = next((x for x in (a0, b0, c0) if x not in on_sub), None)
        if apex is not None:
            r = poly.index(apex)
            rot = poly[r:] + poly[:r]
            out_faces.extend((rot[0], rot[i], rot[i + 1]) for i in range(1, len(rot) - 1))
        else:
            s = [0.0, 0.0, 0.0]
            for p in poly:                                               # mean(axis=0): row after row
                for c in range(3):
                    s[c] += all_v[p][c]
            all_v.append([s[c] / len(poly) for c in range(3)])
            ci = len(all_v) - 1
            n_centroid += 1
            out_faces.extend((ci, poly[i], poly[(i + 1) % len(poly)]) for i in range(len(poly)))
    dense = []
    for a, b in edges:
        dense.append(a)
        dense.extend(inserted[(a, b)])
    info = {"n_inserted": len(new_pts), "n_fanned_faces": len(touched), "n_centroid_fans": n_centroid}
    return (np.array(all_v, dtype=np.float64).reshape(-1, 3), np.array(out_faces, dtype=np.int64).reshape(-1, 3)), dense, info


def densify_boundary(mesh, ring, target_n):
    """:837-962: ``((vertices, faces), dense ring (m, 3), info)``; info adds ``over_target``, ``off_mesh`` and the plan's
    ``gap``."""
    ring = _arr(ring)
    info = {"n_inserted": 0, "n_fanned_faces": 0, "n_centroid_fans": 0, "over_target": 0, "off_mesh": 0, "gap": math.inf}
    counts, status, gap = densify_plan(ring, target_n)
    info["over_target"] = int(status == 2)
    if status != 1:
        return mesh, ring.copy(), info
    info["gap"] = gap
    idx = locate_points(mesh[0], ring)
    if (idx < 0).any():
        info["off_mesh"] = 1
        return mesh, ring.copy(), info
    new_mesh, dense, sinfo = split_rim_edges(mesh, idx, counts)
    info.update(sinfo)
    return new_mesh, new_mesh[0][dense], info


# ---- the whole stage ------------------------------------------------------------------------------------------------------

def toward_aorta(ring_centroid, aorta_pts, fallback):
    """:559-579 (only the direction is returned)."""
    if aorta_pts is not None and len(aorta_pts) > 0:
        direction = _arr(aorta_pts).mean(axis=0) - ring_centroid
        if np.any(direction):
            return direction
    if fallback is not None and np.any(fallback):
        return np.asarray(fallback, dtype=np.float64)
    return None


def condition_ostium_ring(mesh, ring, prox_centroid, iv_frame_pts, outward, angle_threshold_deg, overshoot, aorta_pts,
                          report, layer_step_mm=0.1, n_rings=2):
    """:582-645; fills the report's plane_shift_mm, plane_angle_deg, clamped, n_moved_ostium, n_layer_vertices and the
    intermediates the tests put conditions on (``worst_plus_overshoot``, ``r_norms``, ``gaps``)."""
    ring = _arr(ring)
    if iv_frame_pts is None or len(iv_frame_pts) == 0 or len(ring) < 3:
        return ring, mesh
    iv_arr = _arr(iv_frame_pts)
    original = ring.copy()
    report["gaps"].append(singular_gap(ring))
    aorta_dir = toward_aorta(ring.mean(axis=0), aorta_pts, outward)
    if aorta_dir is not None:
        n0 = plane_normal_svd(ring)
        so, sn, moved = shift_plane_clear_of(ring.mean(axis=0), n0, iv_arr, aorta_dir, overshoot)
        report["worst_plus_overshoot"] = float(((iv_arr - ring.mean(axis=0)) @ sn).max() + overshoot)
        if moved > 0.0:
            report["plane_shift_mm"] = moved
            ring = project_onto_plane(ring, so, sn)
    report["gaps"].append(singular_gap(iv_arr))
    report["gaps"].append(singular_gap(ring))
    iv_normal = plane_normal_svd(iv_arr)
    iv_origin = np.asarray(prox_centroid, dtype=np.float64)
    report["plane_angle_deg"] = angle_between_planes_deg(plane_normal_svd(ring), iv_normal)
    if report["plane_angle_deg"] >= angle_threshold_deg:
        ring = clamp_to_plane(ring, iv_origin, iv_normal, overshoot=overshoot)
        report["clamped"] = 1
    mesh, moved_idx = write_ring_to_mesh(mesh, original, ring)
    report["n_moved_ostium"] = len(moved_idx)
    if report["clamped"] and moved_idx:
        mesh, layer, _, r_norms = enforce_layer_gap_from_plane(mesh, moved_idx, iv_origin, iv_normal, layer_step_mm, n_rings)
        report["r_norms"] = r_norms
        report["n_layer_vertices"] = [int((layer == 1).sum()), int((layer == 2).sum())]
    return ring, mesh


def prepare_prox_dist_boundary_pts(mesh, prox_ring, dist_ring, prox_centroid, proximal_is_ostium=True,
                                   proximal_iv_frame_pts=None, ostium_angle_threshold_deg=45.0, clamp_overshoot=1.0,
                                   target_n=None, prox_outward=None, aorta_pts=None):
    """:505-556 for the two rings already assigned to the ends (:505-521 are checked with the stitch):
    ``(prox_pts, dist_pts, (vertices, faces), report)``."""
    report = {"n_moved_prox": 0, "n_moved_dist": 0, "n_moved_ostium": 0, "plane_shift_mm": 0.0, "plane_angle_deg": 0.0,
              "clamped": 0, "n_layer_vertices": [0, 0], "n_inserted_prox": 0, "n_inserted_dist": 0, "n_fanned_faces": 0,
              "n_centroid_fans": 0, "ring_over_target": [0, 0], "ring_off_mesh": [0, 0],
              "gaps": [], "plan_gaps": [], "worst_plus_overshoot": None, "r_norms": []}
    mesh = (np.array(mesh[0], dtype=np.float64), np.asarray(mesh[1], dtype=np.int64))
    prox_ring, dist_ring = _arr(prox_ring), _arr(dist_ring)
    for r in (prox_ring, dist_ring):
        if len(r) >= 3:
            report["gaps"].append(singular_gap(r))
    prox_pts = redistribute_ring_evenly(smooth_ring_preserving_size(project_to_best_fit_plane(prox_ring)))
    mesh, moved = write_ring_to_mesh(mesh, prox_ring, prox_pts)
    report["n_moved_prox"] = len(moved)
    dist_pts = redistribute_ring_evenly(smooth_ring_preserving_size(project_to_best_fit_plane(dist_ring)))
    mesh, moved = write_ring_to_mesh(mesh, dist_ring, dist_pts)
    report["n_moved_dist"] = len(moved)
    if proximal_is_ostium:
        prox_pts, mesh = condition_ostium_ring(mesh, prox_pts, prox_centroid, proximal_iv_frame_pts, prox_outward,
                                               ostium_angle_threshold_deg, clamp_overshoot, aorta_pts, report)
    if target_n:
        for s, key in ((0, "n_inserted_prox"), (1, "n_inserted_dist")):
            mesh, pts, info = densify_boundary(mesh, prox_pts if s == 0 else dist_pts, target_n)
            report[key] = info["n_inserted"]
            report["n_fanned_faces"] += info["n_fanned_faces"]
            report["n_centroid_fans"] += info["n_centroid_fans"]
            report["ring_over_target"][s] = info["over_target"]
            report["ring_off_mesh"][s] = info["off_mesh"]
            report["plan_gaps"].append(info["gap"])
            if s == 0:
                prox_pts = pts
            else:
                dist_pts = pts
    report["n_vertices"], report["n_faces"] = len(mesh[0]), len(mesh[1])
    return prox_pts, dist_pts, mesh, report
