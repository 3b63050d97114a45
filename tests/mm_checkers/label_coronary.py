"""Plain numpy / Python restatement of the reference's mesh labelling (src/ccta/adjust_mesh/label_coronary.rs:29-640 and
multimodars/ccta/labeling.py:23-280), the parity reference of the labelling tests.  Nothing here touches the device or
the native library.  Float arithmetic is elementwise numpy f64 in the reference's operation order (numpy never fuses a
multiply and an add), so the results are bit-exact restatements, not approximations."""
from __future__ import annotations

import math

import numpy as np


def p3(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


# ---- ray-triangle test (:29-68), vectorised over faces ------------------------------------------------------------
def ray_hits(o, d, tris):
    """(hit mask, t) of one ray (origin o, direction d) against (F, 9) triangles v0 v1 v2."""
    t9 = np.asarray(tris, dtype=np.float64).reshape(-1, 9)
    v0 = t9[:, 0:3]
    e1 = t9[:, 3:6] - v0
    e2 = t9[:, 6:9] - v0
    dx, dy, dz = d
    hx = dy * e2[:, 2] - dz * e2[:, 1]
    hy = dz * e2[:, 0] - dx * e2[:, 2]
    hz = dx * e2[:, 1] - dy * e2[:, 0]
    with np.errstate(all="ignore"):
        a = (e1[:, 0] * hx + e1[:, 1] * hy) + e1[:, 2] * hz
        ok = ~(np.abs(a) < 1e-8)
        f = 1.0 / a
        sx, sy, sz = o[0] - v0[:, 0], o[1] - v0[:, 1], o[2] - v0[:, 2]
        u = f * ((sx * hx + sy * hy) + sz * hz)
        ok &= (u >= 0.0) & (u <= 1.0)
        qx = sy * e1[:, 2] - sz * e1[:, 1]
        qy = sz * e1[:, 0] - sx * e1[:, 2]
        qz = sx * e1[:, 1] - sy * e1[:, 0]
        v = f * ((dx * qx + dy * qy) + dz * qz)
        ok &= ~((v < 0.0) | (u + v > 1.0))
        t = f * ((e2[:, 0] * qx + e2[:, 1] * qy) + e2[:, 2] * qz)
        ok &= t > 1e-8
    return ok, t


def mean_spacing(xyz, branch=None) -> float:
    """Centerline::mean_spacing (centerline.rs:304-320): the first branch run, sequential sum, 1.0 below two points."""
    xyz = p3(xyz)
    n = xyz.shape[0]
    end = n
    if branch is not None and n:
        b = np.asarray(branch)
        ch = np.nonzero(b[1:] != b[:-1])[0]
        end = int(ch[0]) + 1 if ch.size else n
    if end < 2:
        return 1.0
    s = 0.0
    for i in range(1, end):
        dx, dy, dz = xyz[i - 1] - xyz[i]
        s += math.sqrt(dx * dx + dy * dy + dz * dz)
    return s / float(end - 1)


def sat_usize(x: float) -> int:
    """Rust's saturating ``x as usize``."""
    if not (x > 0.0):
        return 0
    if x >= 2.0 ** 64:
        return 2 ** 64 - 1
    return int(x)


def ray_list(cl_coronary, cl_aorta, range_mm, step_size_mm, branch_coronary=None, branch_aorta=None):
    """(origins, directions) of :92-117, or None when step_by(0) would panic."""
    cc, ca = p3(cl_coronary), p3(cl_aorta)
    spacing = (mean_spacing(ca, branch_aorta) + mean_spacing(cc, branch_coronary)) / 2.0
    step = sat_usize(float(np.ceil(step_size_mm / spacing)))
    rng = sat_usize(float(np.ceil(range_mm / spacing)))
    if step == 0:
        return None
    idx = list(range(0, min(rng, cc.shape[0]), step))
    o = np.repeat(ca, len(idx), axis=0)
    d = np.concatenate([cc[idx] - a for a in ca], axis=0) if len(idx) else np.zeros((0, 3))
    return o, d


def excluded_faces(origins, directions, tris):
    """:98-139: per ray, with >= 3 hits, the face of the smallest t (stable sort: lowest index on ties)."""
    out = set()
    for o, d in zip(p3(origins), p3(directions)):
        ok, t = ray_hits(o, d, tris)
        idx = np.nonzero(ok)[0]
        if idx.size >= 3:
            tt = t[idx]
            out.add(int(idx[np.argmin(tt)]))        # argmin: first of equal minima, i.e. the lowest index
    return out


def within_any(q, p, r2):
    """mask over q: some p within squared distance <= r2 (dx*dx + dy*dy + dz*dz)."""
    q, p = p3(q), p3(p)
    m = np.zeros(q.shape[0], dtype=bool)
    if p.shape[0] == 0:
        return m
    for s in range(0, p.shape[0], 256):
        b = p[s:s + 256]
        with np.errstate(invalid="ignore"):
            dx = q[:, None, 0] - b[None, :, 0]
            dy = q[:, None, 1] - b[None, :, 1]
            dz = q[:, None, 2] - b[None, :, 2]
            m |= ((dx * dx + dy * dy + dz * dz) <= r2).any(axis=1)
    return m


def occluded(cl_coronary, cl_aorta, range_mm, points, tris, step_size_mm=1.0):
    """remove_occluded_points_ray_triangle_rust: (removed mask, excluded face set); None when step_by(0) panics."""
    pts = p3(points)
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 9)
    if pts.shape[0] == 0 or tris.shape[0] == 0 or p3(cl_aorta).shape[0] == 0:
        return np.zeros(pts.shape[0], dtype=bool), set()
    rays = ray_list(cl_coronary, cl_aorta, range_mm, step_size_mm)
    if rays is None:
        return None
    ex = excluded_faces(rays[0], rays[1], tris)
    if not ex:
        return np.zeros(pts.shape[0], dtype=bool), ex
    ev = np.concatenate([tris[sorted(ex)].reshape(-1, 3)], axis=0)
    return within_any(pts, ev, 0.5), ex


def bounded(cl, points, radius):
    """find_centerline_bounded_points (:201-235) as a mask over points."""
    return within_any(points, cl, radius * radius)


def faces_near(vertices, faces, points, tol=1e-6):
    """find_faces_near_points (:242-289) as a mask over faces."""
    v, f = p3(vertices), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if p3(points).shape[0] == 0 or v.shape[0] == 0 or f.shape[0] == 0:
        return np.zeros(f.shape[0], dtype=bool)
    matched = within_any(v, points, tol * tol)
    return matched[f].any(axis=1)


def key(p):
    return tuple(np.asarray(p, dtype=np.float64).view(np.uint64).tolist())


def aortic_mask(vertices, a, b):
    """find_aortic_points (:296-313) as a mask over vertices."""
    ex = {key(p) for p in p3(a)} | {key(p) for p in p3(b)}
    return np.array([key(v) not in ex for v in p3(vertices)], dtype=bool)


def adjacency(faces):
    adj = {}
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            adj.setdefault(x, set()).add(y)
            adj.setdefault(y, set()).add(x)
    return adj


def _components(adj, subset):
    comps, seen = [], set()
    for s in sorted(subset):
        if s in seen:
            continue
        comp, stack = set(), [s]
        while stack:
            i = stack.pop()
            if i in comp:
                continue
            comp.add(i)
            stack.extend(n for n in adj.get(i, ()) if n in subset and n not in comp)
        seen |= comp
        comps.append(comp)
    return comps                       # in order of their smallest vertex


def _minority(adj, labels, new, subject, targets):
    subset = {i for i, l in enumerate(labels) if l == subject}
    if not subset:
        return
    comps = _components(adj, subset)
    largest = max(range(len(comps)), key=lambda c: (len(comps[c]), -min(comps[c])))
    for c, comp in enumerate(comps):
        if c == largest:
            continue
        boundary = {n for i in comp for n in adj.get(i, ()) if n not in comp}
        if not boundary:
            continue
        for t in targets:
            if float(sum(labels[n] == t for n in boundary)) > float(len(boundary)) * 0.7:
                for i in comp:
                    new[i] = t
                break


def _restore(adj, labels, new, removed, target):
    subset = {i for i, l in enumerate(labels) if l == removed}
    tc, oc, decided = {}, {}, {}
    for v in subset:
        nb = [n for n in adj.get(v, ()) if n not in subset]
        tc[v] = sum(labels[n] == target for n in nb)
        oc[v] = len(nb) - tc[v]
    frontier = [v for v in subset if tc[v] != oc[v]]
    for v in frontier:
        decided[v] = tc[v] > oc[v]
    while frontier:
        inc = {}
        for v in frontier:
            for n in adj.get(v, ()):
                if n not in subset or n in decided:
                    continue
                e = inc.setdefault(n, [0, 0])
                e[0 if decided[v] else 1] += 1
        nxt = []
        for v, (dt, do) in inc.items():
            tc[v] += dt
            oc[v] += do
            if tc[v] != oc[v]:
                decided[v] = tc[v] > oc[v]
                nxt.append(v)
        frontier = nxt
    for v, is_t in decided.items():
        if is_t:
            new[v] = target


def reclassify(vertices, faces, rca, lca, rca_rm, lca_rm):
    """final_reclassification (:337-640): labels 0..4 per vertex."""
    v = p3(vertices)
    idx = {}
    for i, p in enumerate(v):
        idx[key(p)] = i                      # the last duplicate wins
    labels = [0] * v.shape[0]
    for pts, lab in ((rca, 1), (lca, 2), (rca_rm, 3), (lca_rm, 4)):
        for p in p3(pts):
            i = idx.get(key(p))
            if i is not None:
                labels[i] = lab
    adj = adjacency(faces)
    new = list(labels)
    _minority(adj, labels, new, 0, (1, 2))
    _minority(adj, labels, new, 1, (0,))
    _minority(adj, labels, new, 2, (0,))
    _restore(adj, labels, new, 3, 1)
    _restore(adj, labels, new, 4, 2)
    return np.array(new, dtype=np.uint8)


def clean_outliers(cleanup, reference, radius, ratio):
    """clean_up_non_section_points (scale_coronary.rs:342-409): mask of the cleanup points that join the reference."""
    c, r = p3(cleanup), p3(reference)
    out = np.zeros(c.shape[0], dtype=bool)
    r2 = radius * radius
    for i in range(c.shape[0]):
        d = c[i] - r
        ref_n = int(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) <= r2).sum())
        e = c[i] - c
        self_n = max(int(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) <= r2).sum()) - 1, 0)
        tot = ref_n + self_n
        if tot > 0:
            out[i] = ref_n / tot >= ratio
    return out


def label_geometry(vertices, faces, cl_aorta, cl_rca, cl_lca, acute_rca=False, acute_lca=False, range_rca=60.0,
                   range_lca=60.0, step=1.0, r_rca=3.0, r_lca=3.0, tol=1e-6):
    """labeling.py:23-280 composed from the functions above; centerlines as (N, 3) single-branch arrays.  Returns the
    per-vertex labels 0..4."""
    v, f = p3(vertices), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    empty = np.zeros((0, 3))

    def occl(cl, found, rng):
        tris = v[f[faces_near(v, f, found, tol)]].reshape(-1, 9)
        rm, _ = occluded(cl, cl_aorta, rng, found, tris, step)
        gone = rm | np.isnan(found).any(axis=1)
        return found[gone], found[~rm]

    rca_found = v[bounded(cl_rca, v, r_rca)]
    lca_found = v[bounded(cl_lca, v, r_lca)]
    rca_rm, rca_kept = occl(cl_rca, rca_found, range_rca) if acute_rca else (empty, rca_found)
    lca_rm, lca_kept = occl(cl_lca, lca_found, range_lca) if acute_lca else (empty, lca_found)
    aortic = v[aortic_mask(v, rca_kept, lca_kept)]
    mv = clean_outliers(lca_kept, aortic, 2.0, 0.4)
    lca_pts, aortic2 = lca_kept[~mv], np.concatenate([aortic, lca_kept[mv]])
    rca_pts = rca_kept[~clean_outliers(rca_kept, aortic2, 2.0, 0.4)]
    return reclassify(v, f, rca_pts, lca_pts, rca_rm, lca_rm)
