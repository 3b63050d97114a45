"""The executable form of "mesh cross-sections" (include/mm_ccta.h): the exact cut of a triangle mesh by a stack of
planes, in plain Python floats (IEEE f64, nothing fused), every plane against every face, no cull.  The product
(csrc/mm_section_device.h, csrc/mm_section.cpp, csrc/mm_section_kernels.hip) must equal it bit for bit.

``scan`` returns what ``mm.mesh_cross_sections`` returns, as a dict of arrays; ``segments`` the records of rule 4;
``box_pairs`` / ``crossed_pairs`` the two sides of rule 8 for a given staging order; ``predict_report`` the report
integers that are a function of the sizes alone."""
import math

import numpy as np

NAN = float("nan")
CLOSED, OPEN, BRANCHED = 0, 1, 2
CHUNK, RUN, SEGMENT_BYTES = 256, 64, 72
SEGMENT_DTYPE = np.dtype([("key", "<u8"), ("e", "<i4", (4,)), ("p", "<f8", (6,))])


# ---- rules 1 to 4 ---------------------------------------------------------------------------------------------------

def height(o, n, x):
    return (n[0] * (x[0] - o[0]) + n[1] * (x[1] - o[1])) + n[2] * (x[2] - o[2])


def side(h):
    return 0 if h < 0.0 else 1


def crossing(v, ia, ha, ib, hb):
    """rule 3: ((lo, hi), point) of the crossed edge between vertices ia and ib"""
    lo, hi, h_lo, h_hi = (ia, ib, ha, hb) if ia < ib else (ib, ia, hb, ha)
    t = h_lo / (h_lo - h_hi)
    assert 0.0 <= t <= 1.0
    a, b = v[lo], v[hi]
    return (lo, hi), tuple(a[k] + t * (b[k] - a[k]) for k in range(3))


def _lists(v, f, origins, normals):
    return (np.asarray(v, dtype=np.float64).reshape(-1, 3).tolist(), np.asarray(f, dtype=np.int64).reshape(-1, 3).tolist(),
            np.asarray(origins, dtype=np.float64).reshape(-1, 3).tolist(), np.asarray(normals, dtype=np.float64).reshape(-1, 3).tolist())


def segments(v, f, origins, normals):
    """rule 4: [(plane, face, key0, key1, p0, p1)] sorted by (plane, face), and the number of skipped faces"""
    v, f, origins, normals = _lists(v, f, origins, normals)
    live = [(i, t) for i, t in enumerate(f) if len(set(t)) == 3]
    out = []
    for p, (o, n) in enumerate(zip(origins, normals)):
        hv = [height(o, n, x) for x in v]                     # the side is a function of the vertex alone
        for i, t in live:
            h = [hv[t[0]], hv[t[1]], hv[t[2]]]
            s = [side(x) for x in h]
            if s[0] == s[1] == s[2]:
                continue
            k = 2 if s[0] == s[1] else (1 if s[0] == s[2] else 0)      # the corner alone on its side
            ends = [crossing(v, t[k], h[k], t[(k + j) % 3], h[(k + j) % 3]) for j in (1, 2)]
            ends.sort(key=lambda e: e[0])
            out.append((p, i, ends[0][0], ends[1][0], ends[0][1], ends[1][1]))
    return out, len(f) - len(live)


def to_records(segs):
    rec = np.zeros(len(segs), dtype=SEGMENT_DTYPE)
    for r, (p, i, k0, k1, p0, p1) in zip(rec, segs):
        r["key"] = (p << 32) | i
        r["e"] = [k0[0], k0[1], k1[0], k1[1]]
        r["p"] = list(p0) + list(p1)
    return rec


# ---- rule 6 ---------------------------------------------------------------------------------------------------------

def _dist(a, b):
    ex, ey, ez = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    return math.sqrt((ex * ex + ey * ey) + ez * ez)


def curve_mean(pts, closed):
    L, M = 0.0, [0.0, 0.0, 0.0]
    m = len(pts)
    for i in range(m if closed else m - 1):
        a, b = pts[i], pts[(i + 1) % m]
        ln = _dist(a, b)
        L += ln
        for k in range(3):
            M[k] += ln * (0.5 * (a[k] + b[k]))
    return L, [pts[0][k] if L == 0.0 else M[k] / L for k in range(3)]


EPS = 2.0 ** -52


def loop_signed(pts, n):
    """s, W, B, G of a closed loop in its listed order, about its own first point"""
    A, G, W, B = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0, 0.0
    m = len(pts)
    o = pts[0]
    for i in range(m):
        a, b = pts[i], pts[(i + 1) % m]
        d = [a[k] - o[k] for k in range(3)]
        e = [b[k] - o[k] for k in range(3)]
        c = [d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]]
        for k in range(3):
            A[k] += c[k]
        w = (c[0] * n[0] + c[1] * n[1]) + c[2] * n[2]
        W += w
        q = [abs(d[1] * e[2]) + abs(d[2] * e[1]), abs(d[2] * e[0]) + abs(d[0] * e[2]), abs(d[0] * e[1]) + abs(d[1] * e[0])]
        B += (q[0] * abs(n[0]) + q[1] * abs(n[1])) + q[2] * abs(n[2])
        for k in range(3):
            G[k] += w * (d[k] + e[k])
    return (A[0] * n[0] + A[1] * n[1]) + A[2] * n[2], W, B, G


def loop_flat(m, W, B):
    return not abs(W) > (float(m + 6) * EPS) * B


# ---- rule 7 ---------------------------------------------------------------------------------------------------------

def origin_inside(pts, o, n):
    an = [abs(x) for x in n]
    drop = 0
    for a in (1, 2):
        if an[a] > an[drop]:
            drop = a
    iu, iv = (1 if drop == 0 else 0), (1 if drop == 2 else 2)
    inside = False
    m = len(pts)
    for i in range(m):
        a, b = pts[i], pts[(i + 1) % m]
        if (a[iv] > o[iv]) == (b[iv] > o[iv]):
            continue
        t = ((o[iv] - a[iv]) * (b[iu] - a[iu])) / (b[iv] - a[iv])
        if o[iu] < a[iu] + t:
            inside = not inside
    return inside


# ---- rule 5 ---------------------------------------------------------------------------------------------------------

def chain_plane(segs, o, n):
    """The contours of one plane from its segments in ascending face order: a list of dicts (kind, keys, faces, points,
    area, length, centroid), ordered by their smallest edge key; and the selected one's position or -1."""
    at = {}                                                   # edge key -> [(segment, end)]
    for s, (_p, _i, k0, k1, _p0, _p1) in enumerate(segs):
        at.setdefault(k0, []).append((s, 0))
        at.setdefault(k1, []).append((s, 1))
    point = {k: segs[e[0][0]][4 + e[0][1]] for k, e in at.items()}
    other = lambda s, k: segs[s][3] if segs[s][2] == k else segs[s][2]              # noqa: E731
    seen, contours = set(), []
    for k0 in sorted(at):
        if k0 in seen:
            continue
        comp, stack = {k0}, [k0]                              # the component of k0, its smallest key
        while stack:
            k = stack.pop()
            for s, _e in at[k]:
                k2 = other(s, k)
                if k2 not in comp:
                    comp.add(k2)
                    stack.append(k2)
        seen |= comp
        keys = sorted(comp)
        ends = [k for k in keys if len(at[k]) == 1]
        if max(len(at[k]) for k in keys) > 2:
            mine = [s for s in range(len(segs)) if segs[s][2] in comp]
            L = 0.0
            for s in mine:
                L += _dist(segs[s][4], segs[s][5])
            contours.append(dict(kind=BRANCHED, keys=keys, faces=[-1] * len(keys), points=[point[k] for k in keys], area=NAN,
                                 length=L, centroid=[NAN, NAN, NAN]))
            continue
        is_open = len(ends) == 2
        assert is_open or not ends
        start = ends[0] if is_open else keys[0]
        s = at[start][0][0]
        if not is_open:
            s2 = at[start][1][0]
            if other(s2, start) < other(s, start):
                s = s2
        wk, ws, k = [], [], start
        while True:
            wk.append(k)
            nxt = other(s, k)
            ws.append(s)
            if nxt == start:
                break
            k = nxt
            if len(at[k]) == 1:
                wk.append(k)
                break
            e0, e1 = at[k][0][0], at[k][1][0]
            s = e1 if e0 == s else e0
        pts = [point[k] for k in wk]
        if is_open:
            L, mean = curve_mean(pts, False)
            contours.append(dict(kind=OPEN, keys=wk, faces=[segs[x][1] for x in ws] + [-1], points=pts, area=NAN, length=L,
                                 centroid=mean))
            continue
        sgn, W, B, G = loop_signed(pts, n)
        if sgn < 0.0:
            wk = wk[:1] + wk[1:][::-1]
            ws = ws[::-1]
            pts = [point[k] for k in wk]
            sgn, W, B, G = loop_signed(pts, n)
        L, mean = curve_mean(pts, True)
        flat = loop_flat(len(pts), W, B)
        cen = [mean[k] if flat else pts[0][k] + G[k] / (3.0 * W) for k in range(3)]
        area = (0.5 * sgn) / math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        contours.append(dict(kind=CLOSED, keys=wk, faces=[segs[x][1] for x in ws], points=pts, area=area, length=L, centroid=cen))
    best = -1
    for c, ct in enumerate(contours):
        if ct["kind"] != CLOSED or not origin_inside(ct["points"], o, n):
            continue
        if best < 0 or ct["area"] < contours[best]["area"]:
            best = c
    return contours, best


def scan(v, f, origins, normals):
    """Everything ``mm.mesh_cross_sections`` returns, as a dict of arrays, plus the report's counts."""
    segs, n_skipped = segments(v, f, origins, normals)
    _v, _f, origins, normals = _lists(v, f, origins, normals)
    P = len(origins)
    per_plane = [[] for _ in range(P)]
    for s in segs:
        per_plane[s[0]].append(s)
    off, pts, edge, face, plane, kind, area, length, cen, plane_off, selected = [0], [], [], [], [], [], [], [], [], [0], []
    for p in range(P):
        contours, best = chain_plane(per_plane[p], origins[p], normals[p])
        selected.append(-1 if best < 0 else len(kind) + best)
        for ct in contours:
            pts += ct["points"]; edge += ct["keys"]; face += ct["faces"]
            off.append(len(pts)); plane.append(p); kind.append(ct["kind"]); area.append(ct["area"])
            length.append(ct["length"]); cen.append(ct["centroid"])
        plane_off.append(len(kind))
    i64 = lambda a, shape: np.array(a, dtype=np.int64).reshape(shape)                # noqa: E731
    return {"contour_off": i64(off, -1), "points": np.array(pts, dtype=np.float64).reshape(-1, 3), "point_edge": i64(edge, (-1, 2)),
            "point_face": i64(face, -1), "contour_plane": i64(plane, -1), "contour_kind": np.array(kind, dtype=np.int8),
            "contour_area": np.array(area, dtype=np.float64), "contour_length": np.array(length, dtype=np.float64),
            "contour_centroid": np.array(cen, dtype=np.float64).reshape(-1, 3), "plane_off": i64(plane_off, -1),
            "selected": i64(selected, -1), "segments": segs,
            "counts": {"n_planes": P, "n_faces": len(_f), "n_skipped_faces": n_skipped, "n_segments": len(segs),
                       "n_contours": len(kind), "n_closed": kind.count(CLOSED), "n_open": kind.count(OPEN),
                       "n_branched": kind.count(BRANCHED)}}


ARRAYS = ("contour_off", "points", "point_edge", "point_face", "contour_plane", "contour_kind", "contour_area",
          "contour_length", "contour_centroid", "plane_off", "selected")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- rule 8 ---------------------------------------------------------------------------------------------------------

def box_pairs(order, v, f, origins, normals, chunk=CHUNK):
    """The (plane, chunk) pairs that pass rule 8 for the staging ``order``, as a sorted list, and the chunk boxes."""
    v, f, origins, normals = _lists(v, f, origins, normals)
    boxes = []
    for c0 in range(0, len(order), chunk):
        corners = [v[i] for j in order[c0:c0 + chunk] for i in f[j]]
        boxes.append(([min(x[k] for x in corners) for k in range(3)], [max(x[k] for x in corners) for k in range(3)]))
    pairs = []
    for p, (o, n) in enumerate(zip(origins, normals)):
        for c, (lo, hi) in enumerate(boxes):
            pos = [not (n[k] < 0.0) for k in range(3)]
            h_min = height(o, n, [lo[k] if pos[k] else hi[k] for k in range(3)])
            h_max = height(o, n, [hi[k] if pos[k] else lo[k] for k in range(3)])
            if h_min < 0.0 and not (h_max < 0.0):
                pairs.append((p, c))
    return pairs, boxes


def crossed_pairs(order, segs, chunk=CHUNK):
    """The (plane, chunk) pairs that hold a crossed face, by brute force from the segments."""
    pos = {int(face): j for j, face in enumerate(order)}
    return sorted({(s[0], pos[s[1]] // chunk) for s in segs})


def up256(n):
    return (n + 255) // 256 * 256


def predict_report(nf, n_planes, pairs, n_items, n_segments):
    """The report integers that follow from the sizes: nothing is launched, uploaded or downloaded without an item."""
    if n_items == 0:
        return {"n_launches": 0, "bytes_uploaded": 0, "bytes_downloaded": 0}
    return {"n_launches": 2,
            "bytes_uploaded": up256(nf * 96) + up256(n_planes * 48) + up256(pairs * 4) + up256(n_items * 16),
            "bytes_downloaded": 64 + n_segments * SEGMENT_BYTES}
