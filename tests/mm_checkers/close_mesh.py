"""Numpy / plain-Python restatement of the CCTA mesh closing (multimodars/ccta/fixing_functions.py:13-49,
multimodars/ccta/__init__.py:432-499, src/ccta/binding/ccta_py.rs:743-814): the yardstick for csrc/mm_close_kernels.hip
and csrc/mm_close.cpp.  trimesh is not available, so the loops are not its outline entities: the rules below are this
package's definition (include/mm_ccta.h states the same).

Hole filling:

* winding (fix_normals): stitch_mesh.fix_winding first.
* an undirected edge owned by exactly one face is open; its owner traverses it a -> b: the open half-edge.
* a vertex is regular iff exactly one open half-edge leaves it and exactly one enters it.  Half-edges with a common
  vertex belong to one component.  A component of regular vertices only is one cycle of succ(a) = b: a loop.  Loops come
  in increasing order of their smallest vertex, start there and follow succ; fewer than 3 vertices
  (fixing_functions.py:27): counted, skipped.  Every other component is irregular: counted, left open.
* loop k gets vertex nv + k = the sequential sum of its points in walk order divided by their number, and the faces
  (b, a, nv + k) for its half-edges a -> b in walk order, behind all input faces, loop after loop.
* orientation (fix_normals): stitch_mesh's volume over all faces of the result; volume < 0 reverses every face.

Label smoothing (ccta_py.rs:773-814): synchronous rounds; a vertex with at least one neighbour, all of them carrying
one label different from its own, takes it; a round without a flip ends the run.
"""
import numpy as np

from . import scale_coronary as SC
from . import stitch_mesh as SM
from . import trim_mesh as TM


def open_half_edges(f) -> list:
    """The open half-edges (a, b) of the faces, in face and corner order."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    count = {}
    for a, b, c in f.tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            k = (min(u, w), max(u, w))
            count[k] = count.get(k, 0) + 1
    out = []
    for a, b, c in f.tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            if count[(min(u, w), max(u, w))] == 1:
                out.append((u, w))
    return out


def hole_loops(half_edges):
    """(loops, n_irregular_components, n_irregular_edges, n_short_loops) of the module docstring."""
    n_out, n_in, succ, comp = {}, {}, {}, {}

    def find(x):
        while comp[x] != x:
            x = comp[x]
        return x

    for a, b in half_edges:
        for x in (a, b):
            comp.setdefault(x, x)
            n_out.setdefault(x, 0)
            n_in.setdefault(x, 0)
        n_out[a] += 1
        n_in[b] += 1
        succ[a] = b
        ra, rb = find(a), find(b)
        comp[max(ra, rb)] = min(ra, rb)
    bad = {find(x) for x in comp if n_out[x] != 1 or n_in[x] != 1}
    irregular_edges = sum(1 for a, _ in half_edges if find(a) in bad)
    loops, short, seen = [], 0, set()
    for x in sorted(comp):
        if x in seen or find(x) in bad:
            continue
        loop, y = [], x
        while True:
            seen.add(y)
            loop.append(y)
            y = succ[y]
            if y == x:
                break
        if len(loop) < 3:
            short += 1
        else:
            loops.append(loop)
    return loops, len(bad), irregular_edges, short


def centroid(v, loop):
    s = [0.0, 0.0, 0.0]
    for i in loop:
        for c in range(3):
            s[c] = s[c] + float(v[i][c])
    return [s[c] / float(len(loop)) for c in range(3)]


def fill_holes(v, f, fix_normals=True):
    """(vertices, faces, report); winding_rounds is not restated."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3).copy()
    nv, nf = v.shape[0], f.shape[0]
    report = dict.fromkeys(("n_loops_filled", "n_fan_faces", "n_open_edges_before", "n_short_loops",
                            "n_irregular_components", "n_irregular_edges", "n_open_edges", "n_nonmanifold_edges",
                            "n_flipped_faces", "inverted"), 0)
    report["volume"] = 0.0
    if nf and fix_normals:
        f, flipped, _ = SM.fix_winding(f)
        report["n_flipped_faces"] = int(flipped.sum())
    he = open_half_edges(f)
    loops, n_bad, bad_edges, short = hole_loops(he)
    new_v = [centroid(v, loop) for loop in loops]
    fan = [[loop[(i + 1) % len(loop)], loop[i], nv + k] for k, loop in enumerate(loops) for i in range(len(loop))]
    out_v = np.concatenate([v, np.array(new_v, dtype=np.float64).reshape(-1, 3)])
    out_f = np.concatenate([f, np.array(fan, dtype=np.int64).reshape(-1, 3)])
    _, n_open, n_nonmanifold = SM.face_adjacency(out_f) if out_f.shape[0] else (None, 0, 0)
    report.update(n_vertices=out_v.shape[0], n_faces=out_f.shape[0], n_loops_filled=len(loops), n_fan_faces=len(fan),
                  n_open_edges_before=len(he), n_short_loops=short, n_irregular_components=n_bad,
                  n_irregular_edges=bad_edges, n_open_edges=n_open, n_nonmanifold_edges=n_nonmanifold)
    if nf and fix_normals:
        with np.errstate(all="ignore"):
            volume = SM.pair_tree_sum(SM.volume_terms(out_v, out_f)) / 6.0
        report["volume"] = volume
        if volume < 0.0:
            report["inverted"] = 1
            out_f = out_f[:, ::-1]
    report["watertight"] = n_open == 0 and n_nonmanifold == 0
    return out_v, np.ascontiguousarray(out_f), report


# ---- label smoothing ------------------------------------------------------------------------------------------------------

def adjacency_of_faces(faces, nv) -> list:
    """Row i = the neighbours of vertex i as build_adjacency_map has them (_processing.py:1476-1505): every other corner
    of every face naming it, and itself where a face repeats a corner."""
    rows = [set() for _ in range(nv)]
    for face in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for i in range(3):
            for j in range(3):
                if i != j:
                    rows[face[i]].add(face[j])
    return rows


def smooth_labels(labels, rows, iterations):
    """(labels, info) over neighbour rows (any iterables of indices, read as given)."""
    cur = [int(x) for x in labels]
    info = {"iterations_run": 0, "n_flips": 0, "n_flips_last": 0}
    rows = [list(r) for r in rows]
    for _ in range(int(iterations)):
        nxt = list(cur)
        flips = 0
        for i, row in enumerate(rows):
            seen = {cur[j] for j in row}
            if len(seen) == 1:
                lab = next(iter(seen))
                if lab != cur[i]:
                    nxt[i] = lab
                    flips += 1
        cur = nxt
        info["iterations_run"] += 1
        info["n_flips"] += flips
        info["n_flips_last"] = flips
        if flips == 0:
            break
    return np.array(cur, dtype=np.uint8), info


# ---- wall mesh (ccta/__init__.py:432-499) ---------------------------------------------------------------------------------

def create_wall_mesh(results, cl_aorta, cl_rca, cl_lca, aortic_scaling, coronary_scaling=1.0):
    """(vertices, faces, fill report): the aortic sub-mesh kept, filled and morphed as a whole, the two coronary
    sub-meshes kept and morphed, stacked in that order.  Centerlines are (n, 3) arrays of points."""
    sub = TM.keep_labeled_points_from_mesh(results, ["aorta_points", "rca_removed_points", "lca_removed_points"])
    av, af = sub["mesh"]
    fv, ff, rep = fill_holes(av, af, True)
    parts = [(SC.diameter_morphing(cl_aorta, fv, aortic_scaling, SC.nearest_indices(cl_aorta, fv))[0], ff)]
    for key, cl in (("rca_points", cl_rca), ("lca_points", cl_lca)):
        s = TM.keep_labeled_points_from_mesh(results, [key])
        pv, pf = s["mesh"]
        parts.append((SC.scale_region_centerline_morphing(pv, SC.tuples(s[key]), cl, coronary_scaling), np.asarray(pf, dtype=np.int64)))
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    v = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1, 3) for p in parts])
    f = np.concatenate([np.asarray(p[1], dtype=np.int64).reshape(-1, 3) + o for p, o in zip(parts, off[:-1])])
    return v, f, rep
