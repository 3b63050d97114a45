"""Plain Python / numpy restatement of the mesh refinement (include/mm_ccta.h, "mesh refinement"): the yardstick for
csrc/mm_refine_kernels.hip and csrc/mm_refine.cpp.  Dict insertion order serves as the order of first appearance.

* one pass: the undirected edge lo < hi is marked when ((dx dx + dy dy) + dz dz) > thr2, d = v[hi] - v[lo], unfused f64;
  an (a, a) edge never is.  Marked edges are numbered as the walk over the faces (ascending, corners 0, 1, 2 for the
  edges (c0, c1), (c1, c2), (c2, c0)) first meets them; the k-th gets vertex nv + k = (v[lo] + v[hi]) * 0.5 per
  component and the parents (lo, hi).  Every face is replaced in place by 1 .. 4 children of its winding (`children`).
* passes repeat until one marks nothing, `max_passes` have run, or one would pass `max_vertices` (it is then not run).
* the report: what mm_refine_report holds, the launch and byte counts as include/mm_ccta.h states them.
"""
import numpy as np

from . import smooth_mesh as SMO

PASS_LAUNCHES = 6               # edge table, marks, child counts, tile scan, offsets + midpoints, children
STOP_LAUNCHES = 4               # a pass that marks nothing or would pass max_vertices: no offsets, no children
STAT_LAUNCHES = 2               # the edge statistics alone (behind the last of max_passes passes): edge table, marks
LIST_LAUNCHES = 5               # mesh_edge_lengths: edge table, marks, counts, tile scan, the list
SPLIT_SLOTS = 16


def len_sq(p, q):
    """((dx dx + dy dy) + dz dz) of d = q - p, unfused f64."""
    with np.errstate(all="ignore"):
        dx, dy, dz = np.float64(q[0]) - np.float64(p[0]), np.float64(q[1]) - np.float64(p[1]), np.float64(q[2]) - np.float64(p[2])
        return (dx * dx + dy * dy) + dz * dz


def threshold_sq(target, ratio=4.0 / 3.0):
    t = np.float64(ratio) * np.float64(target)
    return float(t * t)


def edge_table(v, f):
    """{(lo, hi): [owners, squared length]} in order of first appearance, (a, a) edges included."""
    table = {}
    for a, b, c in f:
        for u, w in ((a, b), (b, c), (c, a)):
            key = (min(u, w), max(u, w))
            if key not in table:
                table[key] = [0, float(len_sq(v[key[0]], v[key[1]]))]
            table[key][0] += 1
    return table


def edge_stats(table):
    """n_edges (between different vertices), open (one owner), non-manifold (more than two), the longest squared length."""
    longest = 0.0
    for (lo, hi), (_, d2) in table.items():
        if lo != hi and d2 > longest:                       # NaN compares false: as the device's integer max of the bits
            longest = d2                                    # would not, so the tests keep their coordinates finite
    return {"n_edges": sum(1 for lo, hi in table if lo != hi),
            "n_open_edges": sum(1 for n, _ in table.values() if n == 1),
            "n_nonmanifold_edges": sum(1 for n, _ in table.values() if n > 2), "longest_sq": longest}


def edge_lengths(v, f):
    """(edges (E, 2) int64, squared lengths (E,)): the edges between different vertices in order of first appearance."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    table = edge_table(v, f.tolist())
    keys = [k for k in table if k[0] != k[1]]
    return (np.array(keys, dtype=np.int64).reshape(-1, 2), np.array([table[k][1] for k in keys], dtype=np.float64))


def children(face, mids, v):
    """The children of `face` = (a, b, c); mids[j] = the midpoint vertex of corner j's edge or -1; v: coordinates that
    hold the midpoints already."""
    marked = [j for j in range(3) if mids[j] >= 0]
    if not marked:
        return [tuple(face)]
    if len(marked) == 1:
        j = marked[0]
        a, b, c = face[j], face[(j + 1) % 3], face[(j + 2) % 3]
        m0 = mids[j]
        return [(a, m0, c), (m0, b, c)]
    if len(marked) == 2:
        u = [j for j in range(3) if mids[j] < 0][0]         # the unmarked edge becomes (c, a)
        a, b, c = face[(u + 1) % 3], face[(u + 2) % 3], face[u]
        m0, m1 = mids[(u + 1) % 3], mids[(u + 2) % 3]
        if len_sq(v[m0], v[c]) < len_sq(v[a], v[m1]):
            return [(m0, b, m1), (a, m0, c), (m0, m1, c)]
        return [(m0, b, m1), (a, m0, m1), (a, m1, c)]
    a, b, c = face
    m0, m1, m2 = mids
    return [(a, m0, m2), (m0, b, m1), (m2, m1, c), (m0, m1, m2)]


def one_pass(v, f, thr2):
    """(table, marked keys in first-appearance order) of the mesh (v: list of rows, f: list of triples)."""
    table = edge_table(v, f)
    return table, [k for k, (_, d2) in table.items() if k[0] != k[1] and d2 > thr2]


def emit(v, f, marked):
    """The mesh after the pass: (v, f, parents of the new vertices, faces by number of marked corners)."""
    nv = len(v)
    mid = {k: nv + i for i, k in enumerate(marked)}
    with np.errstate(all="ignore"):
        v = v + [[(np.float64(v[lo][c]) + np.float64(v[hi][c])) * 0.5 for c in range(3)] for lo, hi in marked]
    out, by = [], [0, 0, 0, 0]
    for face in f:
        a, b, c = face
        mids = [mid.get((min(u, w), max(u, w)), -1) for u, w in ((a, b), (b, c), (c, a))]
        by[sum(m >= 0 for m in mids)] += 1
        out += children(face, mids, v)
    return v, out, [list(k) for k in marked], by


def volume_launches(nf):
    return SMO.volume_launches(nf) if nf > 0 else 0


def refine(v, f, target, ratio=4.0 / 3.0, max_passes=10, max_vertices=None):
    """(vertices, faces, parents (n_new, 2), report)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv0, nf0 = v.shape[0], f.shape[0]
    thr2 = threshold_sq(target, ratio)
    cap = 2 ** 31 - 1 if max_vertices is None else int(max_vertices)
    rep = {"passes_run": 0, "splits_per_pass": [0] * SPLIT_SLOTS, "faces_by_template": [0, 0, 0, 0], "converged": 0,
           "stopped_by_cap": 0, "n_launches": 0, "volume_before": SMO.volume(v, f)}
    cv, cf, parents = v.tolist(), [tuple(t) for t in f.tolist()], []
    device = nv0 > 0 and nf0 > 0
    before = after = edge_stats({})
    first = True
    while device:
        table, marked = one_pass(cv, cf, thr2)
        after = edge_stats(table)
        if first:
            before, first = after, False
        if rep["passes_run"] == int(max_passes):
            rep["n_launches"] += STAT_LAUNCHES
            break
        if marked and len(cv) + len(marked) > cap:
            rep["stopped_by_cap"] = 1
            rep["n_launches"] += STOP_LAUNCHES
            break
        rep["splits_per_pass"][min(rep["passes_run"], SPLIT_SLOTS - 1)] += len(marked)
        rep["passes_run"] += 1
        if not marked:
            rep["faces_by_template"][0] += len(cf)
            rep["converged"] = 1
            rep["n_launches"] += STOP_LAUNCHES
            break
        cv, cf, par, by = emit(cv, cf, marked)
        parents += par
        for k in range(4):
            rep["faces_by_template"][k] += by[k]
        rep["n_launches"] += PASS_LAUNCHES
    out_v = np.array(cv, dtype=np.float64).reshape(-1, 3)
    out_f = np.array(cf, dtype=np.int64).reshape(-1, 3)
    if device:
        rep["n_launches"] += volume_launches(nf0) + volume_launches(len(cf))
    rep.update({"n_vertices": len(cv), "n_faces": len(cf), "n_edges_before": before["n_edges"],
                "n_edges_after": after["n_edges"], "longest_sq_before": before["longest_sq"],
                "longest_sq_after": after["longest_sq"], "n_open_edges_before": before["n_open_edges"],
                "n_open_edges_after": after["n_open_edges"], "n_nonmanifold_edges_before": before["n_nonmanifold_edges"],
                "n_nonmanifold_edges_after": after["n_nonmanifold_edges"], "volume_after": SMO.volume(out_v, out_f),
                "bytes_uploaded": 24 * nv0 + 12 * nf0 if device else 0,
                "bytes_downloaded": 24 * len(cv) + 8 * (len(cv) - nv0) + 12 * len(cf) if device else 0})
    return out_v, out_f, np.array(parents, dtype=np.int64).reshape(-1, 2), rep
