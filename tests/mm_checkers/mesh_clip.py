"""The executable form of "mesh clipping" (include/mm_ccta.h): a triangle mesh cut open along plane sections, in plain
Python floats (IEEE f64, nothing fused).  The sections are those of mesh_sections.py (rules 1 to 7), unchanged.  The
product (csrc/mm_clip_device.h, csrc/mm_clip.cpp, csrc/mm_clip_kernels.hip) must equal ``clip`` array for array and bit
for bit, and its report integer for integer (``COUNT_KEYS``; ``predict_report`` restates the launch and byte counts of
the device pass as closed forms of the sizes and the measured jump rounds)."""
import math

import numpy as np

from . import mesh_sections as X

BELOW, ABOVE = 0, 1                  # keep: the side of rule 1 that stays (h < 0: below)
LOOP, PLANE = 0, 1
OK, NO_LOOP, OVERLAP, NOT_SEPARATING, KEPT_SIDE_DROPPED = 0, 1, 2, 3, 4
UNTOUCHED, PIECE, EXTENSION, CAP = 0, 1, 2, 3
RECORD_BYTES, CUT_BYTES = 48, 64

COUNT_KEYS = ("n_cuts", "n_applied", "n_vertices", "n_faces", "n_new_vertices", "n_dropped_vertices", "n_dropped_faces",
              "n_cut_faces", "n_pieces", "n_null_pieces", "n_ext_faces", "n_cap_faces", "n_closed_loops", "n_open_loops")
ARRAYS = ("vertices", "faces", "vertex_origin", "face_origin", "face_kind", "cut_status", "cut_measures", "rim_off",
          "rim_index")


def sq_dist(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def face_pieces(tri, apex, m_ab, m_ca, xyz):
    """C4 for one cut face: [(corners, old vertices)] of the apex piece and the two pieces of the quad.  ``tri`` holds the
    face's three vertex names, ``m_ab`` / ``m_ca`` the names of its two loop points, ``xyz`` maps a name to its point."""
    a, b, c = tri[apex], tri[(apex + 1) % 3], tri[(apex + 2) % 3]
    out = [((a, m_ab, m_ca), (a,))]
    if sq_dist(xyz(m_ab), xyz(c)) < sq_dist(xyz(b), xyz(m_ca)):
        out += [((m_ab, b, c), (b, c)), ((m_ab, c, m_ca), (c,))]
    else:
        out += [((m_ab, b, m_ca), (b,)), ((b, c, m_ca), (b, c))]
    return out


def is_null(corners, xyz):
    p = [tuple(xyz(x)) for x in corners]
    return p[0] == p[1] or p[1] == p[2] or p[0] == p[2]


def _find(root, x):
    while root[x] != x:
        root[x] = root[root[x]]
        x = root[x]
    return x


def clip(v, f, origins, normals, keep, scope, cap=0, ext_length=0.0, ext_layers=0):
    """Everything ``mm.clip_mesh`` returns, as a dict of arrays, and the report's counts."""
    sec = X.scan(v, f, origins, normals)
    v, f, origins, normals = X._lists(v, f, origins, normals)
    K, nv, nf, L = len(origins), len(v), len(f), int(ext_layers)
    keep, scope = [int(x) for x in keep], [int(x) for x in scope]
    off, pface, pedge, kind = sec["contour_off"].tolist(), sec["point_face"].tolist(), sec["point_edge"].tolist(), sec["contour_kind"].tolist()
    pts = sec["points"].tolist()

    # ---- C1
    status, contours, cut_faces, owner = [OK] * K, [], [], {}
    measures = [[X.NAN] * 5 for _ in range(K)]
    for k in range(K):
        if scope[k] == LOOP:
            c = int(sec["selected"][k])
            cs = [c] if c >= 0 and off[c + 1] - off[c] >= 3 else []
            if not cs:
                status[k] = NO_LOOP
            faces = [pface[i] for c in cs for i in range(off[c], off[c + 1])]
        else:
            cs = list(range(int(sec["plane_off"][k]), int(sec["plane_off"][k + 1])))
            faces = [s[1] for s in sec["segments"] if s[0] == k]
        contours.append(cs)
        cut_faces.append(sorted(faces))
        first = [c for c in cs if kind[c] == X.CLOSED][:1]
        if first:
            c = first[0]
            measures[k] = [float(sec["contour_area"][c]), float(sec["contour_length"][c])] + sec["contour_centroid"][c].tolist()
        for face in faces:
            if face in owner and owner[face] != k:
                status[k] = status[owner[face]] = OVERLAP
            owner.setdefault(face, k)
    n_points = [sum(off[c + 1] - off[c] for c in cs) for cs in contours]
    n_closed = [sum(kind[c] == X.CLOSED for c in cs) for cs in contours]
    info = [[status[k], n_points[k], n_closed[k], len(cut_faces[k])] for k in range(K)]

    # the apex and the kept side of every cut face
    side_of = [[X.side(X.height(origins[k], normals[k], x)) for x in v] if K else [] for k in range(K)]
    apex_of = {}
    for face, k in owner.items():
        s = [side_of[k][i] for i in f[face]]
        apex_of[face] = 2 if s[0] == s[1] else (1 if s[0] == s[2] else 0)

    # ---- C2
    dropped = [False] * nv
    if all(s == OK for s in status):
        root = list(range(nv))

        def unite(a, b):
            a, b = _find(root, a), _find(root, b)
            if a != b:
                root[max(a, b)] = min(a, b)
        for i, t in enumerate(f):
            if i in owner:
                a = apex_of[i]
                unite(t[(a + 1) % 3], t[(a + 2) % 3])
            else:
                unite(t[0], t[1]); unite(t[1], t[2])
        marked = set()
        for k in range(K):
            if scope[k] != LOOP:
                continue
            for face in cut_faces[k]:
                a, b = f[face][apex_of[face]], f[face][(apex_of[face] + 1) % 3]
                kept, drop = (a, b) if side_of[k][a] == keep[k] else (b, a)
                if _find(root, kept) == _find(root, drop):
                    status[k] = NOT_SEPARATING
                else:
                    marked.add(_find(root, drop))
        for x in range(nv):
            dropped[x] = _find(root, x) in marked or any(scope[k] == PLANE and side_of[k][x] != keep[k] for k in range(K))
        if all(s == OK for s in status):                   # the orphan check: the marks are complete
            for face, k in owner.items():
                a = apex_of[face]
                t = f[face]
                kept_side = [t[a]] if side_of[k][t[a]] == keep[k] else [t[(a + 1) % 3], t[(a + 2) % 3]]
                if any(dropped[x] for x in kept_side):
                    status[k] = KEPT_SIDE_DROPPED
        for k in range(K):
            info[k][0] = status[k]

    counts = dict.fromkeys(COUNT_KEYS, 0)
    counts["n_cuts"] = K
    out = {"cut_status": np.array(info, dtype=np.int64).reshape(K, 4), "cut_measures": np.array(measures, dtype=np.float64).reshape(K, 5)}
    # ---- C3
    if any(s != OK for s in status):
        counts["n_vertices"], counts["n_faces"] = nv, nf
        out.update(vertices=np.array(v, dtype=np.float64).reshape(-1, 3), faces=np.array(f, dtype=np.int64).reshape(-1, 3),
                   vertex_origin=np.arange(nv, dtype=np.int64), face_origin=np.arange(nf, dtype=np.int64),
                   face_kind=np.zeros(nf, dtype=np.int8), rim_off=np.zeros(1, dtype=np.int64), rim_index=np.zeros(0, dtype=np.int64),
                   counts=counts, applied=False, n_records=0, n_plane_cuts=0)
        return out

    # ---- C5: the vertices
    new_name = [-1] * nv
    V, VO = [], []
    for x in range(nv):
        if not dropped[x]:
            new_name[x] = len(V)
            V.append(v[x]); VO.append(x)
    kv = len(V)
    name_of_edge = [dict() for _ in range(K)]              # per cut: edge key -> vertex of its loop point
    ring_name = {}                                         # (cut, closed loop, point, ring) -> vertex
    centre_name = {}
    for k in range(K):
        o, n = origins[k], normals[k]
        for c in contours[k]:
            for i in range(off[c], off[c + 1]):
                name_of_edge[k][tuple(pedge[i])] = len(V)
                if kind[c] == X.CLOSED:
                    ring_name[(k, c, i - off[c], 0)] = len(V)
                V.append(pts[i]); VO.append(-1 - k)
        nn = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        u = [n[0] / nn, n[1] / nn, n[2] / nn]
        sgn = 1.0 if keep[k] == BELOW else -1.0
        step = ext_length / L if L else 0.0
        for j in range(1, L + 1):
            for c in contours[k]:
                if kind[c] != X.CLOSED:
                    continue
                for i in range(off[c], off[c + 1]):
                    ring_name[(k, c, i - off[c], j)] = len(V)
                    V.append([pts[i][a] + (sgn * (float(j) * step)) * u[a] for a in range(3)]); VO.append(-1 - k)
        if cap:
            for c in contours[k]:
                if kind[c] != X.CLOSED:
                    continue
                centre_name[(k, c)] = len(V)
                cen = sec["contour_centroid"][c].tolist()
                V.append([cen[a] + (sgn * (float(L) * step)) * u[a] for a in range(3)] if L else cen); VO.append(-1 - k)
    xyz = lambda name: V[name]                             # noqa: E731

    # ---- C4, C7.1
    F, FO, FK = [], [], []
    kept_edge = {}                                         # cut face -> (x, y): its kept side runs x -> y along the rim
    for i, t in enumerate(f):
        if i not in owner:
            if not (dropped[t[0]] or dropped[t[1]] or dropped[t[2]]):
                F.append([new_name[x] for x in t]); FO.append(i); FK.append(UNTOUCHED)
            else:
                counts["n_dropped_faces"] += 1
            continue
        k, a = owner[i], apex_of[i]
        key = lambda p, q: (min(p, q), max(p, q))          # noqa: E731
        m_ab = name_of_edge[k][key(t[a], t[(a + 1) % 3])]
        m_ca = name_of_edge[k][key(t[(a + 2) % 3], t[a])]
        tri = [new_name[x] if not dropped[x] else -2 - x for x in t]       # a dropped vertex keeps a name of its own
        coords = lambda name: V[name] if name >= 0 else v[-2 - name]       # noqa: E731
        n_kept = 0
        for corners, old in face_pieces(tri, a, m_ab, m_ca, coords):
            if any(x < 0 for x in old):
                continue
            F.append(list(corners)); FO.append(i); FK.append(PIECE)
            n_kept += 1
            counts["n_null_pieces"] += is_null(corners, coords)
        counts["n_pieces"] += n_kept
        counts["n_dropped_faces"] += n_kept == 0
        kept_edge[i] = (m_ab, m_ca) if side_of[k][t[a]] == keep[k] else (m_ca, m_ab)
    # ---- C6, C7.2 and C7.3
    rim_off, rim_index = [0], []
    for k in range(K):
        for j in range(L):
            for c in contours[k]:
                if kind[c] != X.CLOSED:
                    continue
                m = off[c + 1] - off[c]
                local = {ring_name[(k, c, i, 0)]: i for i in range(m)}
                for i in range(m):
                    x, y = (local[w] for w in kept_edge[pface[off[c] + i]])
                    assert {x, y} == {i, (i + 1) % m}
                    xj, yj, xj1, yj1 = ring_name[(k, c, x, j)], ring_name[(k, c, y, j)], ring_name[(k, c, x, j + 1)], ring_name[(k, c, y, j + 1)]
                    F += [[yj, xj, xj1], [yj, xj1, yj1]]; FO += [-1 - k] * 2; FK += [EXTENSION] * 2
    for k in range(K):
        for c in contours[k]:
            if kind[c] != X.CLOSED:
                counts["n_open_loops"] += 1
                continue
            m = off[c + 1] - off[c]
            counts["n_closed_loops"] += 1
            rim_index += [ring_name[(k, c, i, L)] for i in range(m)]
            rim_off.append(len(rim_index))
            if not cap:
                continue
            local = {ring_name[(k, c, i, 0)]: i for i in range(m)}
            for i in range(m):
                x, y = (local[w] for w in kept_edge[pface[off[c] + i]])
                F.append([ring_name[(k, c, y, L)], ring_name[(k, c, x, L)], centre_name[(k, c)]]); FO.append(-1 - k); FK.append(CAP)
    counts.update(n_applied=K, n_vertices=len(V), n_faces=len(F), n_new_vertices=len(V) - kv, n_dropped_vertices=nv - kv,
                  n_cut_faces=len(owner), n_ext_faces=FK.count(EXTENSION), n_cap_faces=FK.count(CAP))
    out.update(vertices=np.array(V, dtype=np.float64).reshape(-1, 3), faces=np.array(F, dtype=np.int64).reshape(-1, 3),
               vertex_origin=np.array(VO, dtype=np.int64), face_origin=np.array(FO, dtype=np.int64),
               face_kind=np.array(FK, dtype=np.int8), rim_off=np.array(rim_off, dtype=np.int64),
               rim_index=np.array(rim_index, dtype=np.int64), counts=counts, applied=True, n_records=len(owner),
               n_plane_cuts=sum(s == PLANE for s in scope))
    return out


def up256(n):
    return (n + 255) // 256 * 256


def predict_report(nv, nf, n_cuts, want, jump_rounds):
    """The launches and the bytes of the clip's own device pass (the section pass before it reports its own) from the
    sizes, the checker's result ``want`` and the measured jump rounds R.  Nothing runs on the device without a cut,
    without a vertex or where C1 leaves a status other than OK.  Otherwise 5 + R launches (initialise, scatter, sides,
    unions, R jumps, verdict), 1 more (the orphan check, whose K status words are read a second time) where no cut is
    NOT_SEPARATING and, where the cuts are applied, 11 more (keep flags, 3 of their scan, piece counts, 3 of
    their scan -- none on a mesh without faces --, vertices, faces, rim faces).  bytes_uploaded is restated where the
    cuts are applied (the new vertices of a call that is NOT_SEPARATING are not part of its result)."""
    status = want["cut_status"][:, 0].tolist()
    if n_cuts == 0 or nv == 0 or NO_LOOP in status or OVERLAP in status:
        return {"n_launches": 0, "bytes_uploaded": 0, "bytes_downloaded": 0, "jump_rounds": 0}
    checked = NOT_SEPARATING not in status
    out = {"n_launches": 5 + jump_rounds + checked, "bytes_downloaded": 4 * jump_rounds + 4 * n_cuts * (1 + checked),
           "jump_rounds": jump_rounds}
    if want["applied"]:
        c = want["counts"]
        out["n_launches"] += 11 if nf > 0 else 8
        out["bytes_downloaded"] += 16 + 64 + c["n_vertices"] * 28 + c["n_faces"] * 17
        out["bytes_uploaded"] = (up256(nv * 24) + up256(nf * 12) + up256(want["n_records"] * RECORD_BYTES) + up256(c["n_new_vertices"] * 24) +
                                 up256(c["n_new_vertices"] * 4) + up256(n_cuts * CUT_BYTES))
    return out
