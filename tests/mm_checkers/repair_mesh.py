"""Plain sequential Python / numpy restatement of the mesh repair (include/mm_ccta.h, "mesh repair"): the yardstick for
csrc/mm_repair_kernels.hip and csrc/mm_repair.cpp.  Neither MeshLab nor vcglib is available, so the rules are this
package's own; DESIGN 4.25 says where they knowingly differ from MeshLab's filters.  No device, no hash table: dicts,
sorts and a union-find over corners.

* `weld`: stage (a), duplicate vertices by `==` on the coordinates (+0.0 equals -0.0), the smallest index survives.
* `cross_q`: the unfused cross product of stage (b) and the squared double area q of stage (d).
* `remove_walk` / `remove_closed`: stage (d) as the literal sequential walk and as the closed form the device uses.
* `corner_components`: stage (e), the components of the corners at every vertex.  A component that is exactly the
  corners of one vertex w that stage (a) welded away is not given a new vertex: the weld of w is undone and w comes back
  with its own index order and bits, counted neither as welded nor as new.  So a repaired mesh needs nothing.
* `repair`: the stages in order, origin, target and the report (COUNT_KEYS; union_rounds, the launches and the bytes
  are the device's own and are held against the header's formulas in tests/test_gpu_repair.py).
* `manifold_counts`: what mm.mesh_manifold_report returns.
"""
import struct

import numpy as np

FLAGS = ("duplicate_vertices", "null_faces", "duplicate_faces", "nonmanifold_edges", "nonmanifold_vertices",
         "drop_unreferenced")
LAUNCHES = 28                   # the kernels of one call with at least one face, the union-find's jumping rounds apart
COUNT_KEYS = ("n_vertices", "n_faces", "n_welded_vertices", "n_degenerate_faces", "n_null_faces", "n_duplicate_faces",
              "n_nonmanifold_edges_before", "n_nonmanifold_edges_after", "n_faces_removed", "n_nonmanifold_vertices",
              "n_new_vertices", "n_unreferenced_dropped", "n_open_edges_before", "n_open_edges_after")


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def weld(v) -> np.ndarray:
    """rep[i] = the smallest index whose three coordinates compare equal to those of i."""
    first, rep = {}, np.zeros(len(v), dtype=np.int64)
    for i, p in enumerate(np.asarray(v, dtype=np.float64).reshape(-1, 3).tolist()):
        key = tuple(bits(c + 0.0) if c != 0.0 else 0 for c in p)      # -0.0 and +0.0: one key
        rep[i] = first.setdefault(key, i)
    return rep


def cross_q(v, f):
    """(cx, cy, cz, q) per face: (p1 - p0) x (p2 - p0) and q = (cx cx + cy cy) + cz cz, every operation rounded once."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        ux, uy, uz = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
        wx, wy, wz = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p2[:, 2] - p0[:, 2]
        cx = uy * wz - uz * wy
        cy = uz * wx - ux * wz
        cz = ux * wy - uy * wx
        q = (cx * cx + cy * cy) + cz * cz
    return cx, cy, cz, q


def edges_of(face):
    a, b, c = face
    return ((min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a)))


def edge_owners(f, alive) -> dict:
    """undirected edge -> its owners among the faces with alive[i], in face order."""
    own = {}
    for i, face in enumerate(f):
        if alive[i]:
            for e in edges_of(face):
                own.setdefault(e, []).append(i)
    return own


def edge_counts(f, alive):
    """(open, non-manifold) edges of the live faces."""
    own = edge_owners(f, alive)
    return sum(1 for o in own.values() if len(o) == 1), sum(1 for o in own.values() if len(o) > 2)


def remove_walk(f, alive, q) -> list:
    """Stage (d), literally: the faces with an edge of more than two owners, sorted by (q, index) ascending, each
    deleted when its turn comes iff it still has such an edge.  Returns the faces removed, as a sorted list."""
    own = edge_owners(f, alive)
    count = {e: len(o) for e, o in own.items()}
    bad = sorted({i for o in own.values() if len(o) > 2 for i in o}, key=lambda i: (q[i], i))
    gone = []
    for i in bad:
        es = edges_of(f[i])
        if any(count[e] > 2 for e in es):
            gone.append(i)
            for e in es:
                count[e] -= 1
    return sorted(gone)


def remove_closed(f, alive, q) -> list:
    """Stage (d), the closed form: a face goes iff on some edge with more than two owners it is not one of the two
    owners with the largest keys (q, index)."""
    gone = set()
    for o in edge_owners(f, alive).values():
        if len(o) > 2:
            gone.update(sorted(o, key=lambda i: (q[i], i))[:-2])
    return sorted(gone)


def corner_components(f, alive) -> dict:
    """Stage (e): corner id 3 i + k (i: the face's index in f) -> the smallest corner id of its component.  Two corners
    at one vertex are linked when their faces share an edge at that vertex with exactly two owners."""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, face in enumerate(f):
        if alive[i]:
            for k in range(3):
                parent[3 * i + k] = 3 * i + k
    for (u, w), o in edge_owners(f, alive).items():
        if len(o) == 2 and o[0] != o[1]:
            for x in (u, w):
                a, b = find(3 * o[0] + f[o[0]].index(x)), find(3 * o[1] + f[o[1]].index(x))
                parent[max(a, b)] = min(a, b)
    return {c: find(c) for c in parent}


def repair(v, f, duplicate_vertices=True, null_faces=True, duplicate_faces=True, nonmanifold_edges=True,
           nonmanifold_vertices=True, drop_unreferenced=False, closed_form=False):
    """(vertices, faces, origin, target, report) of the header's rule.  A stage that is switched off still counts what
    it finds (n_welded_vertices, n_null_faces, n_duplicate_faces, n_nonmanifold_vertices) and changes nothing;
    n_faces_removed, n_new_vertices and n_unreferenced_dropped count what was done."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    rep = dict.fromkeys(COUNT_KEYS, 0)
    # (a)
    found = weld(v)
    rep["n_welded_vertices"] = int((found != np.arange(nv)).sum())
    name = found if duplicate_vertices else np.arange(nv, dtype=np.int64)
    g = [tuple(int(name[x]) for x in face) for face in f.tolist()]
    # (b)
    cx, cy, cz, q = cross_q(v, np.array(g, dtype=np.int64).reshape(-1, 3))
    alive = [True] * nf
    for i, (a, b, c) in enumerate(g):
        if a == b or b == c or a == c:
            alive[i] = False
            rep["n_degenerate_faces"] += 1
        elif cx[i] == 0.0 and cy[i] == 0.0 and cz[i] == 0.0:
            rep["n_null_faces"] += 1
            alive[i] = not null_faces
    # (c)
    seen = set()
    for i, face in enumerate(g):
        if alive[i]:
            key = tuple(sorted(face))
            if key in seen:
                rep["n_duplicate_faces"] += 1
                alive[i] = not duplicate_faces
            seen.add(key)
    # (d)
    rep["n_open_edges_before"], rep["n_nonmanifold_edges_before"] = edge_counts(g, alive)
    if nonmanifold_edges:
        gone = (remove_closed if closed_form else remove_walk)(g, alive, q.tolist())
        for i in gone:
            alive[i] = False
        rep["n_faces_removed"] = len(gone)
    rep["n_open_edges_after"], rep["n_nonmanifold_edges_after"] = edge_counts(g, alive)
    # (e)
    root = corner_components(g, alive)
    keeper = {}
    for c in sorted(root):
        keeper.setdefault(g[c // 3][c % 3], root[c])                   # the smallest corner at a vertex is a root
    opened = sorted({r for c, r in root.items() if r != keeper[g[c // 3][c % 3]]})
    # a component that is exactly the corners of one welded input vertex w: the weld of w is undone, w comes back
    fin = f.tolist()
    members, roots_of = {}, {}
    for c, r in root.items():
        w = fin[c // 3][c % 3]
        members.setdefault(r, set()).add(w)
        roots_of.setdefault(w, set()).add(r)
    back = {}
    for r in opened:
        w = fin[r // 3][r % 3]
        if w != g[r // 3][r % 3] and members[r] == {w} and roots_of[w] == {r}:
            back[r] = w
    opened = [r for r in opened if r not in back]
    if duplicate_vertices:
        rep["n_welded_vertices"] -= len(back)
    rep["n_nonmanifold_vertices"] = len({g[r // 3][r % 3] for r in opened})
    if not nonmanifold_vertices:
        opened = []
    rep["n_new_vertices"] = len(opened)
    # (f) and the numbering: the vertices kept in order, then the new vertices in the order of their smallest corner
    used = {x for i, face in enumerate(g) if alive[i] for x in face}
    unwelded = set(back.values())
    survivors = [i for i in range(nv) if name[i] == i and (not drop_unreferenced or i in used)]
    rep["n_unreferenced_dropped"] = int((name == np.arange(nv)).sum()) - len(survivors)
    keep = sorted(survivors + list(unwelded))
    index = {old: new for new, old in enumerate(keep)}
    rank = {r: len(keep) + k for k, r in enumerate(opened)}
    origin = np.array(keep + [g[r // 3][r % 3] for r in opened], dtype=np.int64)
    target = np.array([index[j] if j in index else index.get(int(name[j]), -1) for j in range(nv)], dtype=np.int64)
    out_f = []
    for i, face in enumerate(g):
        if alive[i]:
            row = []
            for k in range(3):
                r = root[3 * i + k]
                row.append(rank[r] if r in rank else index[back[r]] if r in back else index[face[k]])
            out_f.append(row)
    out_v = v[origin] if origin.size else np.zeros((0, 3))
    rep["n_vertices"], rep["n_faces"] = int(origin.size), len(out_f)
    return np.ascontiguousarray(out_v), np.array(out_f, dtype=np.int64).reshape(-1, 3), origin, target, rep


def rounds_bound(nf: int) -> int:
    """What union_rounds stays within: 2 + ceil(log2(max(3 nf, 2)))."""
    n, l = max(3 * nf, 2), 0
    while (1 << l) < n:
        l += 1
    return 2 + l


def manifold_counts(v, f) -> dict:
    """What mm.mesh_manifold_report returns: the findings of repair with every switch off."""
    r = repair(v, f, False, False, False, False, False, False)[4]
    return {"n_vertices": len(np.asarray(v).reshape(-1, 3)), "n_faces": len(np.asarray(f).reshape(-1, 3)),
            "n_open_edges": r["n_open_edges_before"],
            "n_nonmanifold_edges": r["n_nonmanifold_edges_before"], "n_nonmanifold_vertices": r["n_nonmanifold_vertices"],
            "n_duplicate_vertices": r["n_welded_vertices"], "n_degenerate_faces": r["n_degenerate_faces"],
            "n_null_faces": r["n_null_faces"], "n_duplicate_faces": r["n_duplicate_faces"]}
