"""CCTA mesh labelling and diameter search.  Labelling mirrors the reference's
``label_geometry`` (multimodars/ccta/labeling.py:23-280) and the entry points it composes
(src/ccta/binding/ccta_py.rs:52-262, implementation src/ccta/adjust_mesh/label_coronary.rs); the
diameter search mirrors the reference's entry points
``adjust_diameter_centerline_morphing_simple`` / ``find_proximal_distal_scaling`` /
``find_aortic_scaling`` / ``find_aortic_wall_scaling`` (src/ccta/binding/ccta_py.rs:263-481;
implementation src/ccta/adjust_mesh/scale_coronary.rs:8-261) and the wrapper
``find_distal_and_proximal_scaling`` of multimodars/ccta/scaling.py:84-145.

Same argument names, order and meaning; points are ``(N, 3)`` arrays (or lists of tuples).  Each
search scores its 41 scalings in one GPU batch (exact f64 nearest-neighbour minima,
csrc/mm_nn_kernels.hip); there is no CPU fallback.  The vessel discretisation mirrors ``discretize_vessel`` and
``discretize_vessel_tree`` (src/ccta/binding/ccta_py.rs:724-920, multimodars/_processing.py:1507,
multimodars/ccta/discretization_map.py:104-205; implementation src/ccta/discretizing).  The mesh morphing mirrors
``label_anomalous_region`` (multimodars/ccta/labeling.py:283-389), ``scale_region_centerline_morphing`` /
``sync_results_to_mesh`` (multimodars/ccta/scaling.py:16-80, 301-351) and ``scale`` (multimodars/ccta/__init__.py:171-258);
its nearest-centerline search runs on the device (csrc/mm_morph_kernels.hip).  The branch labelling mirrors
``label_branches`` (multimodars/ccta/labeling.py:415-487), ``label_branches_pair`` / ``find_sharp_angles``
(multimodars/ccta/discretization_map.py:216-306) and ``label`` (multimodars/ccta/__init__.py:22-168); which branches
reach a point comes from one launch (csrc/mm_branch_kernels.hip).
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _native as N
from . import geometry as G
from .centerline import Centerline

SCALING_STEPS = 41


def _p3(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def _engine(engine: Optional[N.Engine]) -> N.Engine:
    if engine is not None:
        return engine
    from .api import default_engine
    return default_engine()


def nn_min_sq(a, b, engine: Optional[N.Engine] = None) -> np.ndarray:
    """min_b |a_i - b|^2 for every a_i (the inner fold of symmetric_nn_distance / find_region_points)."""
    a, b = _p3(a), _p3(b)
    xyz = np.ascontiguousarray(np.concatenate([a, b], axis=0))
    set_off = np.array([0, a.shape[0], a.shape[0] + b.shape[0]], dtype=np.int64)
    q, p = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    out_off = np.array([0, a.shape[0]], dtype=np.int64)
    out = np.zeros(a.shape[0], dtype=np.float64)
    N.check(N.lib().mm_nn_min_sq_batch(_engine(engine).handle, 2, N._ptr(set_off), N._ptr(xyz), 1, N._ptr(q),
                                       N._ptr(p), N._ptr(out_off), N._ptr(out)), "nn_min_sq")
    return out


def nn_plan(sets, pairs, r2: float = 0.0, order_like=None) -> dict:
    """TEST HOOK (``mm_nn_plan``; host only, no engine): the work lists the nearest-neighbour launches build.  `sets`: (N, 3)
    arrays, or dicts {"xyz", "unit", "has", "adj"} for a set whose points are xyz moved by adj along unit where has;
    `pairs`: (query set, point set).  Returns every set's staging permutation ("perm": staged position -> original
    point), the items of pass A, pass B and the radius count for `r2` ("a", "b", "count": int arrays of (pair, q0, c0,
    n_chunks), "a_lb2" / "b_lb2" / "count_lb2" their bounds), and the block geometry ("qpb", "chunk", "span")."""
    xyz, unit, has, adj, derived, off = [], [], [], [], [], [0]
    for s in sets:
        d = s if isinstance(s, dict) else {"xyz": s}
        x = _p3(d["xyz"])
        xyz.append(x)
        derived.append(1 if "unit" in d else 0)
        unit.append(_p3(d["unit"]) if "unit" in d else np.zeros_like(x))
        has.append(np.asarray(d["has"], dtype=np.uint8).reshape(-1) if "unit" in d else np.zeros(len(x), dtype=np.uint8))
        adj.append(float(d.get("adj", 0.0)))
        off.append(off[-1] + len(x))
    xyz = np.ascontiguousarray(np.concatenate(xyz) if xyz else np.zeros((0, 3)))
    unit = np.ascontiguousarray(np.concatenate(unit) if unit else np.zeros((0, 3)))
    has = np.ascontiguousarray(np.concatenate(has) if has else np.zeros(0, dtype=np.uint8))
    adj, derived = np.array(adj, dtype=np.float64), np.array(derived, dtype=np.uint8)
    set_off = np.array(off, dtype=np.int64)
    q = np.array([p[0] for p in pairs], dtype=np.int32)
    p_ = np.array([p[1] for p in pairs], dtype=np.int32)
    ol = None if order_like is None else np.ascontiguousarray(order_like, dtype=np.int32)
    perm = np.zeros(max(int(set_off[-1]), 1), dtype=np.int32)
    info = np.zeros(6, dtype=np.int64)
    args = [len(sets), N._ptr(set_off), N._ptr(xyz), N._ptr(unit), N._ptr(has), N._ptr(derived), N._ptr(adj),
            N._ptr(ol), len(pairs), N._ptr(q), N._ptr(p_), float(r2), N._ptr(perm), N._ptr(info)]
    N.check(N.lib().mm_nn_plan(*args, None, None, 0), "nn_plan")
    cap = int(info[:3].sum())
    items, lb2 = np.zeros((max(cap, 1), 5), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.float64)
    N.check(N.lib().mm_nn_plan(*args, N._ptr(items), N._ptr(lb2), cap), "nn_plan")
    out = {"perm": [perm[off[s]:off[s + 1]].copy() for s in range(len(sets))],
           "qpb": int(info[3]), "chunk": int(info[4]), "span": int(info[5])}
    k = 0
    for l, name in enumerate(("a", "b", "count")):
        n = int(info[l])
        assert n == 0 or (items[k:k + n, 0] == l).all()
        out[name], out[name + "_lb2"] = items[k:k + n, 1:].copy(), lb2[k:k + n].copy()
        k += n
    return out


def symmetric_nn_distance(a, b, engine: Optional[N.Engine] = None) -> float:
    """scale_coronary.rs:188-216 (RMS of the two mean squared nearest-neighbour distances)."""
    a, b = _p3(a), _p3(b)
    out = C.c_double(0.0)
    N.check(N.lib().mm_symmetric_nn_distance(_engine(engine).handle, N._ptr(a), a.shape[0], N._ptr(b), b.shape[0],
                                             C.byref(out)), "symmetric_nn_distance")
    return out.value


def adjust_diameter_centerline_morphing_simple(centerline: Centerline, points, diameter_adjustment_mm: float) -> np.ndarray:
    """ccta_py.rs:263-278: every point moves by ``diameter_adjustment_mm`` along the direction from
    its closest centerline point."""
    p = _p3(points)
    out = np.zeros_like(p)
    N.check(N.lib().mm_diameter_morphing(N._ptr(centerline.points), len(centerline), N._ptr(p), p.shape[0],
                                         float(diameter_adjustment_mm), N._ptr(out)), "diameter_morphing")
    return out


def find_region_points(anomalous_points, reference_points, n_points: int, engine: Optional[N.Engine] = None):
    """scale_coronary.rs:133-183 -> (selected, remaining)."""
    a, r = _p3(anomalous_points), _p3(reference_points)
    sel, rem = np.zeros_like(a), np.zeros_like(a)
    k = N.lib().mm_find_region_points(_engine(engine).handle, N._ptr(a), a.shape[0], N._ptr(r), r.shape[0],
                                      int(n_points), N._ptr(sel), N._ptr(rem))
    if k < 0:
        N.check(int(k), "find_region_points")
    return sel[:k].copy(), rem[: a.shape[0] - k].copy()


def find_proximal_distal_scaling(anomalous_points, n_proximal: int, n_distal: int, centerline: Centerline,
                                 proximal_reference, distal_reference,
                                 engine: Optional[N.Engine] = None) -> Tuple[float, float]:
    """ccta_py.rs:389-407 / multimodars/_processing.py:1431-1473."""
    a, pr, dr = _p3(anomalous_points), _p3(proximal_reference), _p3(distal_reference)
    pb, db = C.c_double(0.0), C.c_double(0.0)
    N.check(N.lib().mm_diameter_optimization(_engine(engine).handle, N._ptr(a), a.shape[0], int(n_proximal),
                                             int(n_distal), N._ptr(centerline.points), len(centerline), N._ptr(pr),
                                             pr.shape[0], N._ptr(dr), dr.shape[0], C.byref(pb), C.byref(db)),
            "find_proximal_distal_scaling")
    return pb.value, db.value


def find_aortic_scaling(intramural_points, reference_points, centerline: Centerline,
                        engine: Optional[N.Engine] = None, return_distances: bool = False):
    """ccta_py.rs:428-442."""
    i, r = _p3(intramural_points), _p3(reference_points)
    best = C.c_double(0.0)
    d = np.zeros(SCALING_STEPS, dtype=np.float64)
    N.check(N.lib().mm_aortic_diameter_optimization(_engine(engine).handle, N._ptr(i), i.shape[0], N._ptr(r),
                                                    r.shape[0], N._ptr(centerline.points), len(centerline),
                                                    C.byref(best), N._ptr(d)), "find_aortic_scaling")
    return (best.value, d) if return_distances else best.value


def find_aortic_wall_scaling_raw(cl_aorta: Centerline, ref_pt_coronary, aortic_pts) -> float:
    """The binding ``find_aortic_wall_scaling`` (ccta_py.rs:467-481, host only)."""
    r = np.ascontiguousarray(np.asarray(ref_pt_coronary, dtype=np.float64).reshape(3))
    a = _p3(aortic_pts)
    out = C.c_double(0.0)
    N.check(N.lib().mm_wall_diameter_optimization(N._ptr(cl_aorta.points), len(cl_aorta), N._ptr(r), N._ptr(a),
                                                  a.shape[0], C.byref(out)), "find_aortic_wall_scaling")
    return out.value


def find_distal_and_proximal_scaling(geometry: G.FlatGeometry, centerline: Centerline, results: dict,
                                     dist_range: int = 3, prox_range: int = 2,
                                     engine: Optional[N.Engine] = None) -> Tuple[float, float]:
    """multimodars/ccta/scaling.py:84-145 with the frame list given as a FlatGeometry: the lumen
    points of the last ``dist_range`` / first ``prox_range`` frames are the references and a quarter
    of the anomalous points is compared on either side."""
    F = geometry.n_frames
    dist_pts = geometry.lumen[geometry.lumen_off[max(F - dist_range, 0)]:geometry.lumen_off[F]]
    prox_pts = geometry.lumen[geometry.lumen_off[0]:geometry.lumen_off[min(prox_range, F)]]
    n_section = int(math.ceil(0.25 * len(results["anomalous_points"])))
    return find_proximal_distal_scaling(results["anomalous_points"], n_section, n_section, centerline, prox_pts,
                                        dist_pts, engine=engine)


def _extract_wall_from_frames(geometry: G.FlatGeometry):
    """multimodars/ccta/scaling.py:239-297: the straight (coronary-side) half of the Wall contour, point
    indices below n/2, of the LAST frame that carries an aortic thickness; None if there is none."""
    from . import frames as FR
    fr = FR.to_frames(geometry)
    half = len(fr[0].lumen) // 2
    ref = None
    for f in fr:
        if f.lumen.aortic_thickness is None:
            continue
        wall = f.extras.get("wall")
        if wall is None:
            raise ValueError(f"No Wall extras found for frame {f.id}")
        if len(wall) == 0:
            raise ValueError(f"Empty Wall extras for frame {f.id}")
        ref = wall.points[:half].copy()
    return ref


def find_aorta_scaling(geometry: G.FlatGeometry, cl_aorta: Centerline, results: dict,
                       engine: Optional[N.Engine] = None) -> float:
    """multimodars/ccta/scaling.py:148-189: the removed RCA points are scaled radially about the aortic
    centerline against the straight wall of the intravascular frames."""
    ref = _extract_wall_from_frames(geometry)
    if ref is None:
        raise ValueError("No aortic wall points found in frames for scaling reference")
    return find_aortic_scaling(results["rca_removed_points"], ref, cl_aorta, engine=engine)


def find_aortic_wall_scaling(geometry_or_centerline, cl_aorta=None, results=None, aortic_pts=None):
    """Both spellings of the reference: the wrapper ``find_aortic_wall_scaling(frames, cl_aorta, results)``
    (multimodars/ccta/scaling.py:192-236: reference point = the point at index n/4 of the first lumen with
    an elliptic ratio < 1.3, scored against ``results["aorta_points"]``) when the first argument is a
    geometry, and the binding ``find_aortic_wall_scaling(cl_aorta, ref_pt_coronary, aortic_pts)``
    (ccta_py.rs:467-481) when it is a centerline."""
    if isinstance(geometry_or_centerline, Centerline):
        pts = aortic_pts if aortic_pts is not None else results
        return find_aortic_wall_scaling_raw(geometry_or_centerline, cl_aorta, pts)
    from .api import _elliptic_ratio
    g = geometry_or_centerline
    ref_point = None
    for i in range(g.n_frames):
        lum = g.frame_lumen(i)
        if _elliptic_ratio(lum) < 1.3:
            ref_point = lum[lum.shape[0] // 4].copy()
            break
    if ref_point is None:
        raise ValueError("No coronary reference point found")
    return find_aortic_wall_scaling_raw(cl_aorta, ref_point, results["aorta_points"])


def clean_outlier_points(points_to_cleanup, reference_points, neighborhood_radius: float, min_neigbor_ratio: float,
                         engine: Optional[N.Engine] = None):
    """ccta_py.rs:345-358 -> ``clean_up_non_section_points`` (scale_coronary.rs:342-409): a point of
    ``points_to_cleanup`` most of whose neighbours (within ``neighborhood_radius``) are reference points joins
    the reference set.  Returns (cleaned points, reference points + the moved ones in input order).  The
    neighbour counts run on the device in exact f64."""
    c, r = _p3(points_to_cleanup), _p3(reference_points)
    mv = np.zeros(c.shape[0], dtype=np.uint8)
    N.check(N.lib().mm_clean_outlier_points(_engine(engine).handle, N._ptr(c), c.shape[0], N._ptr(r), r.shape[0],
                                            float(neighborhood_radius), float(min_neigbor_ratio), N._ptr(mv)),
            "clean_outlier_points")
    return c[mv == 0].copy(), np.concatenate([r, c[mv == 1]], axis=0)


def find_points_by_cl_region(centerline: Centerline, frames, points, engine: Optional[N.Engine] = None,
                             cl_frame_index=None, return_labels: bool = False):
    """ccta_py.rs:304-319 -> ``find_points_by_cl_region_rs`` (scale_coronary.rs:263-312): the points whose
    closest centerline point lies within the imaged section (within the mean frame spacing of a frame
    centroid) are ``between``; the rest is proximal or distal of the last frame's centroid; two density
    clean-ups then move stray proximal / distal points into ``between``.  ``frames``: a FlatGeometry (its
    frame centroids are used) or an (F, 3) array of centroids.  Returns (proximal, distal, between) as
    (n, 3) arrays in the reference's order."""
    cen = frames.centroids if isinstance(frames, G.FlatGeometry) else np.asarray(frames, dtype=np.float64)
    cen = np.ascontiguousarray(cen.reshape(-1, 3))
    p = _p3(points)
    fi = None if cl_frame_index is None else np.ascontiguousarray(cl_frame_index, dtype=np.uint32)
    if fi is not None and fi.shape[0] != len(centerline):
        raise ValueError("cl_frame_index: one entry per centerline point")
    lab = np.zeros(p.shape[0], dtype=np.uint8)
    N.check(N.lib().mm_find_points_by_cl_region(_engine(engine).handle, N._ptr(centerline.points), N._ptr(fi),
                                                len(centerline), N._ptr(cen), cen.shape[0], N._ptr(p), p.shape[0],
                                                N._ptr(lab)), "find_points_by_cl_region")
    out = (p[lab == 0].copy(), p[lab == 1].copy(), np.concatenate([p[lab == 2], p[lab == 3], p[lab == 4]], axis=0))
    return out + (lab,) if return_labels else out


# ---- mesh labelling (src/ccta/adjust_mesh/label_coronary.rs, multimodars/ccta/labeling.py) -----------------------

def _mesh_parts(mesh):
    """(vertices, faces) of a ``(vertices, faces)`` pair or of any object with ``.vertices`` / ``.faces``."""
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return mesh.vertices, mesh.faces
    vertices, faces = mesh
    return vertices, faces


def _faces3(faces) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))


def _tris(faces) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(faces, dtype=np.float64).reshape(-1, 9))


def find_centerline_bounded_points_simple(centerline: Centerline, points, radius: float,
                                          engine: Optional[N.Engine] = None) -> np.ndarray:
    """ccta_py.rs:52-76 -> find_centerline_bounded_points (label_coronary.rs:201-235): the points within ``radius`` of
    some centerline point (squared distance <= radius * radius), in input order, duplicates kept.  An empty point set
    or centerline raises ValueError, as the reference does."""
    p = _p3(points)
    if p.shape[0] == 0 or len(centerline) == 0:
        raise ValueError("find_centerline_bounded_points failed because `Centerline` is empty")
    inside = np.zeros(p.shape[0], dtype=np.uint8)
    k = N.lib().mm_centerline_bounded_points(_engine(engine).handle, N._ptr(centerline.points), len(centerline),
                                             N._ptr(p), p.shape[0], float(radius), N._ptr(inside))
    if k < 0:
        N.check(int(k), "find_centerline_bounded_points_simple")
    return p[inside == 1].copy()


def find_faces_near_points(vertices, faces, points, tol: float = 1e-6, engine: Optional[N.Engine] = None) -> np.ndarray:
    """ccta_py.rs:176-207 -> label_coronary.rs:242-289: every face (in face order) with a corner within ``tol`` of one
    of ``points``, as an ``(F, 3, 3)`` array of its corner coordinates."""
    v, f, p = _p3(vertices), _faces3(faces), _p3(points)
    sel = np.zeros(f.shape[0], dtype=np.uint8)
    k = N.lib().mm_faces_near_points(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(p),
                                     p.shape[0], float(tol), N._ptr(sel))
    if k < 0:
        N.check(int(k), "find_faces_near_points")
    return v[f[sel == 1]].reshape(-1, 3, 3).copy()


def occluded_point_flags(centerline_coronary: Centerline, centerline_aorta: Centerline, range_mm: float, points, faces,
                         step_size_mm: float = 1.0, engine: Optional[N.Engine] = None):
    """The flags behind remove_occluded_points_ray_triangle: (removed per point, excluded per face) as uint8 arrays."""
    p, t = _p3(points), _tris(faces)
    removed = np.zeros(p.shape[0], dtype=np.uint8)
    excluded = np.zeros(t.shape[0], dtype=np.uint8)
    k = N.lib().mm_occluded_points(_engine(engine).handle, N._ptr(centerline_coronary.points), len(centerline_coronary),
                                   N._ptr(centerline_aorta.points), len(centerline_aorta), float(range_mm), N._ptr(p),
                                   p.shape[0], N._ptr(t), t.shape[0], float(step_size_mm), N._ptr(removed),
                                   N._ptr(excluded))
    if k < 0:
        N.check(int(k), "remove_occluded_points_ray_triangle")
    return removed, excluded


def remove_occluded_points_ray_triangle(centerline_coronary: Centerline, centerline_aorta: Centerline, range_mm: float,
                                        points, faces, step_size_mm: float = 1.0,
                                        engine: Optional[N.Engine] = None) -> np.ndarray:
    """ccta_py.rs:78-150 -> label_coronary.rs:70-197: rays from every aortic centerline point to the coronary points
    within ``range_mm`` of the ostium (every ``step_size_mm``); a ray that crosses at least 3 of ``faces`` (``(F, 3, 3)``
    triangles) excludes the face it hits first, and the points within squared distance 0.5 of a vertex of an excluded
    face are removed.  Returns the remaining points in input order.  The ray-triangle tests run on the device in
    exact f64 (csrc/mm_ray_kernels.hip)."""
    p = _p3(points)
    removed, _ = occluded_point_flags(centerline_coronary, centerline_aorta, range_mm, p, faces, step_size_mm, engine)
    return p[removed == 0].copy()


def find_aortic_points(vertices, points_a, points_b) -> np.ndarray:
    """ccta_py.rs:209-235 -> label_coronary.rs:296-313 (host): the vertices whose coordinates are bit for bit in
    neither ``points_a`` nor ``points_b``, in vertex order."""
    v, a, b = _p3(vertices), _p3(points_a), _p3(points_b)
    keep = np.zeros(v.shape[0], dtype=np.uint8)
    k = N.lib().mm_find_aortic_points(N._ptr(v), v.shape[0], N._ptr(a), a.shape[0], N._ptr(b), b.shape[0], N._ptr(keep))
    if k < 0:
        N.check(int(k), "find_aortic_points")
    return v[keep == 1].copy()


def final_reclassification(vertices, faces, rca_points, lca_points, rca_removed_points, lca_removed_points,
                           return_labels: bool = False):
    """ccta_py.rs:237-262 -> label_coronary.rs:337-640 (host): vertex labels from the four point lists, smoothed on
    the mesh adjacency (minority components join a neighbouring label, removed vertices are restored by majority
    votes).  Returns (aorta, rca, lca, rca_removed, lca_removed) vertices in vertex order (and the per-vertex labels
    0..4 with ``return_labels``).  Of equally large largest components the one holding the smallest vertex index is
    kept; the reference picks one of them in hash order, so this is one of its possible outcomes."""
    v, f = _p3(vertices), _faces3(faces)
    lists = [_p3(x) for x in (rca_points, lca_points, rca_removed_points, lca_removed_points)]
    lab = np.zeros(v.shape[0], dtype=np.uint8)
    args = []
    for x in lists:
        args += [N._ptr(x), x.shape[0]]
    N.check(N.lib().mm_final_reclassification(N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], *args, N._ptr(lab)),
            "final_reclassification")
    out = tuple(v[lab == k].copy() for k in range(5))
    return out + (lab,) if return_labels else out


def _apply_occlusion_removal(range_mm: float, step_size_mm: float, tol: float, cl_aorta: Centerline,
                             cl_coronary: Centerline, vertices, faces, found, engine):
    """labeling.py:252-280: (removed, kept) of the points ``found`` near a coronary centerline."""
    tris = find_faces_near_points(vertices, faces, found, tol, engine=engine)
    removed, _ = occluded_point_flags(cl_coronary, cl_aorta, range_mm, found, tris, step_size_mm, engine)
    kept = found[removed == 0].copy()
    # `[p for p in found if p not in set(kept)]`: a point with a NaN coordinate equals nothing, so it lands in both
    gone = (removed == 1) | np.isnan(found).any(axis=1)
    return found[gone].copy(), kept


def label_geometry(mesh, centerline_aorta: Centerline, centerline_rca: Centerline, centerline_lca: Centerline,
                   acute_takeoff_rca: bool = False, acute_takeoff_lca: bool = False, range_mm_takeoff_rca: float = 60.0,
                   range_mm_takeoff_lca: float = 60.0, step_size_mm: float = 1.0,
                   bounding_sphere_radius_mm_rca: float = 3.0, bounding_sphere_radius_mm_lca: float = 3.0,
                   tolerance_float: float = 1e-6, control_plot: bool = True,
                   engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/labeling.py:23-250: label the vertices of a CCTA surface mesh as aorta, RCA or LCA.

    ``mesh``: a ``(vertices, faces)`` pair or any object with ``.vertices`` / ``.faces`` (a ``trimesh.Trimesh``
    works; it is not read here).  The vertices within the bounding sphere radius of a coronary centerline are that
    coronary's; with an acute take-off the points behind the aortic wall are removed by ray casting; outliers are
    cleaned against the aorta and the labels smoothed on the mesh adjacency (final_reclassification).  No file is
    read and nothing is plotted (``control_plot`` is accepted and ignored).  Returns the reference's dict: ``"mesh"``
    (what was passed), ``"aorta_points"``, ``"rca_points"``, ``"lca_points"``, ``"rca_removed_points"``,
    ``"lca_removed_points"`` as ``(n, 3)`` arrays."""
    vertices, faces = _mesh_parts(mesh)
    v, f = _p3(vertices), _faces3(faces)
    eng = _engine(engine)
    rca_found = find_centerline_bounded_points_simple(centerline_rca, v, bounding_sphere_radius_mm_rca, engine=eng)
    lca_found = find_centerline_bounded_points_simple(centerline_lca, v, bounding_sphere_radius_mm_lca, engine=eng)
    empty = np.zeros((0, 3), dtype=np.float64)
    if acute_takeoff_rca:
        rca_removed, rca_kept = _apply_occlusion_removal(range_mm_takeoff_rca, step_size_mm, tolerance_float,
                                                         centerline_aorta, centerline_rca, v, f, rca_found, eng)
    else:
        rca_removed, rca_kept = empty, rca_found
    if acute_takeoff_lca:
        lca_removed, lca_kept = _apply_occlusion_removal(range_mm_takeoff_lca, step_size_mm, tolerance_float,
                                                         centerline_aorta, centerline_lca, v, f, lca_found, eng)
    else:
        lca_removed, lca_kept = empty, lca_found
    aortic = find_aortic_points(v, rca_kept, lca_kept)
    lca_pts, aortic2 = clean_outlier_points(lca_kept, aortic, 2.0, 0.4, engine=eng)      # labeling.py:184-189
    rca_pts, _ = clean_outlier_points(rca_kept, aortic2, 2.0, 0.4, engine=eng)
    aorta, rca, lca, rca_rm, lca_rm = final_reclassification(v, f, rca_pts, lca_pts, rca_removed, lca_removed)
    return {"mesh": mesh, "aorta_points": aorta, "rca_points": rca, "lca_points": lca, "rca_removed_points": rca_rm,
            "lca_removed_points": lca_rm}


# ---- branch labelling (multimodars/ccta/labeling.py:415-487, discretization_map.py:216-306, __init__.py:22-168) -------

_EMPTY_SEARCH = "find_centerline_bounded_points failed because `Centerline` is empty"


def branch_masks(centerline: Centerline, points, radius: float, engine: Optional[N.Engine] = None) -> np.ndarray:
    """One uint64 per point: bit b is set iff some point of ``centerline`` with ``branch_id`` b lies within ``radius``
    (squared distance <= radius * radius, the test of ``find_centerline_bounded_points_simple``): what one call of that
    function per branch answers, from one upload and one launch (csrc/mm_branch_kernels.hip).  An empty point set or
    centerline raises ValueError, as that function does; a ``branch_id`` of 64 or more raises RuntimeError."""
    p = _p3(points)
    if p.shape[0] == 0 or len(centerline) == 0:
        raise ValueError(_EMPTY_SEARCH)
    masks = np.zeros(p.shape[0], dtype=np.uint64)
    N.check(N.lib().mm_branch_masks(_engine(engine).handle, N._ptr(centerline.points), len(centerline), N._ptr(p),
                                    p.shape[0], float(radius), N._ptr(masks)), "branch_masks")
    return masks


def label_branches(centerline: Centerline, results: dict, results_key: str = "rca_points", branch_id=0,
                   bounding_sphere_radius_mm: float = 3.0, engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/labeling.py:415-487: split ``results[results_key]`` into ``"{key}_main"`` (the points within
    ``bounding_sphere_radius_mm`` of a main branch: ``branch_id``, an int or a list of ints), ``"{key}_side"`` (all
    others) and ``"{key}_side_{k}"`` for every other branch k of ``centerline`` (the side points within the radius of
    branch k; a point near two side branches is in both), all in input order with duplicates kept, as ``(n, 3)``
    arrays.  The reference searches the points once per branch; here every point's branches come from one launch
    (``branch_masks``) and the lists are read off the masks.  Mutates and returns ``results``.  Raises what the
    reference's sequence raises: ValueError for a branch the centerline does not have and for an empty point list or an
    empty remainder when a search would run on it (the keys written before that stay)."""
    branch_ids = [int(branch_id)] if isinstance(branch_id, (int, np.integer)) else [int(b) for b in branch_id]
    p = _p3(results[results_key])
    present = set(int(b) for b in np.unique(centerline.points["branch_id"]))

    def need(b):
        if b not in present:
            raise ValueError(f"branch_id {b} not found in centerline")        # get_branch

    for b in branch_ids:
        need(b)
        if p.shape[0] == 0:
            raise ValueError(_EMPTY_SEARCH)
    n, n_branches = p.shape[0], len(centerline.branch_start_indices)
    side_ids = [k for k in range(n_branches) if k not in set(branch_ids)]
    nb = min(n_branches, 64)
    main_idx, side_idx = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    off, counts = np.zeros(nb + 1, dtype=np.int64), np.zeros(3, dtype=np.int64)
    side_k = np.zeros(2 * n, dtype=np.int64)
    if n:
        ids = np.array(branch_ids, dtype=np.uint32)
        masks = np.zeros(n, dtype=np.uint64)
        L = N.lib()
        N.check(L.mm_label_branches(_engine(engine).handle, N._ptr(centerline.points), len(centerline), N._ptr(p), n,
                                    float(bounding_sphere_radius_mm), N._ptr(ids), len(ids), nb, N._ptr(masks),
                                    N._ptr(main_idx), N._ptr(side_idx), N._ptr(off), N._ptr(side_k), side_k.shape[0],
                                    N._ptr(counts)), "label_branches")
        if int(counts[2]) > side_k.shape[0]:                # many points near several side branches: fill from the masks
            side_k = np.zeros(int(counts[2]), dtype=np.int64)
            N.check(L.mm_branch_select(N._ptr(masks), n, N._ptr(ids), len(ids), nb, None, None, N._ptr(off),
                                       N._ptr(side_k), side_k.shape[0], N._ptr(counts)), "label_branches")
    main_points, side_points = p[main_idx[:int(counts[0])]], p[side_idx[:int(counts[1])]]
    results[f"{results_key}_main"] = main_points
    results[f"{results_key}_side"] = side_points
    print(f"\nBranch labeling for '{results_key}' (branch_ids={branch_ids}):")
    print(f"  {results_key}_main: {len(main_points)}")
    print(f"  {results_key}_side: {len(side_points)}")
    for k in side_ids:
        need(k)
        if side_points.shape[0] == 0:
            raise ValueError(_EMPTY_SEARCH)
        pts_k = p[side_k[int(off[k]):int(off[k + 1])]]
        results[f"{results_key}_side_{k}"] = pts_k
        print(f"  {results_key}_side_{k}: {len(pts_k)}")
    return results


def label_branches_pair(rca_cl: Centerline, lca_cl: Centerline, results_dict: dict, control_plot: bool = False,
                        engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/discretization_map.py:216-263: ``label_branches`` for ``"rca_points"`` along ``rca_cl``, then
    for ``"lca_points"`` along ``lca_cl`` (branch 0 the main vessel, radius 3 mm): the keys ``discretize_vessel_tree``
    reads.  The centerlines are expected prepared (``prepare_centerline``).  ``control_plot`` is accepted and ignored."""
    results_dict = label_branches(rca_cl, results_dict, engine=engine)
    results_dict = label_branches(lca_cl, results_dict, results_key="lca_points", engine=engine)
    return results_dict


def find_sharp_angles(cl: Centerline, branch_id: int, cos_threshold: float = 0.0, control_plot: bool = False) -> list:
    """multimodars/ccta/discretization_map.py:266-306: ``cl.find_sharp_angles`` with the reference's log line; the
    global point indices ``split_branch`` takes.  ``control_plot`` is accepted and ignored."""
    positions = cl.find_sharp_angles(branch_id, cos_threshold)
    print(f"Branch {branch_id}: {len(positions)} sharp angle(s) at point_index {positions}")
    return positions


def label(mesh, path_centerline_aorta, path_centerline_rca, path_centerline_lca, aligned_frames,
          acute_takeoff_rca: bool = False, acute_takeoff_lca: bool = False, range_mm_takeoff_rca: float = 60.0,
          range_mm_takeoff_lca: float = 60.0, step_size_mm: float = 1.0, bounding_sphere_radius_mm_rca: float = 3.0,
          bounding_sphere_radius_mm_lca: float = 3.0, tolerance_float: float = 1e-6, control_plot: bool = True,
          engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/__init__.py:22-168: load the three centerlines (``load_centerline``: a Centerline, an array, a
    ``.vtp`` or a comma-delimited file), orient the aorta by its highest point and the coronaries towards the aorta,
    ``label_geometry``, then ``label_anomalous_region`` along the RCA if its take-off is acute, else along the LCA if
    that one is.  ``mesh`` is what ``label_geometry`` takes (no mesh file is read); ``aligned_frames`` what
    ``label_anomalous_region`` takes; ``control_plot`` is accepted and ignored."""
    from .centerline import load_centerline
    ao_cl = load_centerline(path_centerline_aorta, "Aorta").orient_by_max_z()
    rca_cl = load_centerline(path_centerline_rca, "RCA").orient_to_reference(ao_cl)
    lca_cl = load_centerline(path_centerline_lca, "LCA").orient_to_reference(ao_cl)
    results = label_geometry(mesh, ao_cl, rca_cl, lca_cl, acute_takeoff_rca, acute_takeoff_lca, range_mm_takeoff_rca,
                             range_mm_takeoff_lca, step_size_mm, bounding_sphere_radius_mm_rca,
                             bounding_sphere_radius_mm_lca, tolerance_float, control_plot, engine=engine)
    if acute_takeoff_rca or acute_takeoff_lca:
        key, cl = ("rca_points", rca_cl) if acute_takeoff_rca else ("lca_points", lca_cl)
        results = label_anomalous_region(cl, aligned_frames, results, results_key=key, engine=engine)
    return results


# ---- vessel discretisation (src/ccta/discretizing) ------------------------------------------------------------------
def _discretize_jobs(jobs, step_size: float, n_points: int, engine: Optional[N.Engine]):
    """discretize_vessel_rs for every (centerline, points, branch_id) job in one device pass -> one contour list per
    job."""
    from .frames import Contour
    L = N.lib()
    cls = [c.points for c, _, _ in jobs]
    pts = [_p3(p) for _, p, _ in jobs]
    caps = []
    for c, _, b in jobs:
        k = L.mm_slice_anchor_count(N._ptr(c.points), len(c), int(b), float(step_size))
        if k < 0:
            N.check(int(k), "discretize_vessel")
        caps.append(int(k))
    nj = len(jobs)
    cl_off = np.concatenate([[0], np.cumsum([len(c) for c in cls])]).astype(np.int64)
    pt_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    cl_all, xyz = np.ascontiguousarray(np.concatenate(cls)), np.ascontiguousarray(np.concatenate(pts))
    bid = np.array([int(b) for _, _, b in jobs], dtype=np.uint32)
    total = int(out_off[-1])
    n_contours = np.zeros(nj, dtype=np.int64)
    ids = np.zeros(total, dtype=np.int32)
    cen = np.zeros((total, 3))
    out = np.zeros((total, max(int(n_points), 0), 3))
    N.check(L.mm_discretize_vessel_batch(_engine(engine).handle, nj, N._ptr(cl_all), N._ptr(cl_off), N._ptr(bid),
                                         N._ptr(xyz), N._ptr(pt_off), float(step_size), int(n_points), N._ptr(out_off),
                                         N._ptr(n_contours), N._ptr(ids), N._ptr(cen), N._ptr(out)), "discretize_vessel")
    res = []
    for j in range(nj):
        o = int(out_off[j])
        res.append([Contour(int(ids[o + k]), int(ids[o + k]), out[o + k].copy(), tuple(float(v) for v in cen[o + k]),
                            kind="lumen") for k in range(int(n_contours[j]))])
    return res


def discretize_vessel(centerline: Centerline, points, branch_id: int = 0, step_size: float = 0.5, n_points: int = 200,
                      engine: Optional[N.Engine] = None):
    """ccta_py.rs:724-741 -> discretize_vessel_rs (src/ccta/discretizing.rs:13-22): cut branch ``branch_id`` of
    ``centerline`` every ``step_size`` (arc length), give every point to its nearest slice anchor, project it onto that
    anchor's plane, drop empty slices and the partial ones at both ends, and resample each remaining slice to
    ``n_points`` points on a closed Catmull-Rom spline.  Returns ``frames.Contour`` objects (kind "lumen"); a
    contour's ``id`` and ``original_frame`` are its slice index, its centroid the anchor.  The nearest-anchor pass runs
    on the device in exact f64 (csrc/mm_slice_kernels.hip).  A ``step_size`` <= 0 or non-finite, or ``n_points`` < 2,
    raises RuntimeError."""
    return _discretize_jobs([(centerline, points, branch_id)], step_size, n_points, engine)[0]


@dataclass
class ReferenceTriplet:
    """discretized_tree.rs:4-9"""
    main_ref: Tuple[float, float, float]
    counter_clock_ref: Tuple[float, float, float]
    clock_ref: Tuple[float, float, float]


def _t3(v) -> Tuple[float, float, float]:
    return (float(v[0]), float(v[1]), float(v[2]))


def _norm3(v) -> float:
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _sub3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _try_normalize(v):
    """nalgebra try_normalize(1e-12), falling back to +z"""
    n = _norm3(v)
    return (v[0] / n, v[1] / n, v[2] / n) if n > 1e-12 else (0.0, 0.0, 1.0)


def _first_min(vals) -> int:
    k, best = 0, None
    for i, x in enumerate(vals):
        if best is None or x < best:
            k, best = i, x
    return k


def _assign_cc_clock(p1, p2, centroid, normal, up):
    """discretized_tree.rs:295-313: (counter_clock, clock) seen proximal -> distal"""
    dn = (up[0] * normal[0] + up[1] * normal[1]) + up[2] * normal[2]
    w = (up[0] - normal[0] * dn, up[1] - normal[1] * dn, up[2] - normal[2] * dn)
    n = _norm3(w)
    u = (w[0] / n, w[1] / n, w[2] / n) if n > 1e-12 else (0.0, 0.0, 0.0)
    right = (u[1] * normal[2] - u[2] * normal[1], u[2] * normal[0] - u[0] * normal[2], u[0] * normal[1] - u[1] * normal[0])
    d = _sub3(p1, centroid)
    return (p1, p2) if (d[0] * right[0] + d[1] * right[1]) + d[2] * right[2] < 0.0 else (p2, p1)


def _vessel_references(ao, main, branches):
    """discretized_tree.rs:148-293: the ostium triplet, then one per side branch, sorted by main-vessel contour index"""
    from .api import _find_closest_opposite_3d, _find_farthest_points
    mc = [_t3(c.centroid) for c in main]
    up = _try_normalize(_sub3(mc[0], ao))
    tagged = []
    first = main[0].points
    if first.shape[0] > 2:
        normal = _try_normalize(_sub3(mc[1], mc[0])) if len(main) > 1 else _try_normalize(_sub3(mc[0], ao))
        (i, j), _ = _find_closest_opposite_3d(first)
        pa, pb = _t3(first[i]), _t3(first[j])
        main_ref = pa if _norm3(_sub3(pa, ao)) <= _norm3(_sub3(pb, ao)) else pb
        (i, j), _ = _find_farthest_points(first)
        cc, cl = _assign_cc_clock(_t3(first[i]), _t3(first[j]), mc[0], normal, up)
        tagged.append((0, ReferenceTriplet(main_ref, cc, cl)))
    for br in branches:
        if not br:
            continue
        side = _t3(br[0].centroid)
        k = _first_min([_norm3(_sub3(m, side)) for m in mc])
        bc = mc[k]
        if k + 1 < len(main):
            normal = _try_normalize(_sub3(mc[k + 1], bc))
        elif k > 0:
            normal = _try_normalize(_sub3(bc, mc[k - 1]))
        else:
            normal = _try_normalize(_sub3(bc, ao))
        pts = main[k].points
        n = pts.shape[0]
        if n < 4:
            continue
        ci = _first_min([_norm3(_sub3(_t3(p), side)) for p in pts])
        q = n // 4
        cc, cl = _assign_cc_clock(_t3(pts[(ci + q) % n]), _t3(pts[(ci + n - q) % n]), bc, normal, up)
        tagged.append((k, ReferenceTriplet(side, cc, cl)))
    tagged.sort(key=lambda x: x[0])
    return [r for _, r in tagged]


@dataclass
class DiscretizedVesselTree:
    """types/native/discretized_tree.rs:11-32: the discretised aorta, main vessels and side branches (branch i + 1 at
    index i) with the orientation references of calculate_ref_pts."""
    discretized_aorta: list
    discretized_rca_main: list
    discretized_lca_main: list
    spacing: float
    rca_branches: list = field(default_factory=list)
    lca_branches: list = field(default_factory=list)
    rca_references: list = field(default_factory=list)
    lca_references: list = field(default_factory=list)
    ao_rca: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    ao_lca: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    pts_cusp_rcc: Optional[list] = None
    pts_cusp_lcc: Optional[list] = None
    pts_cusp_acc: Optional[list] = None
    index_stj_slice: Optional[int] = None
    index_aa: Optional[int] = None

    def calculate_ref_pts(self) -> "DiscretizedVesselTree":
        """discretized_tree.rs:95-145: ao_rca / ao_lca = the centroid of the aorta slice nearest to the first contour
        of the main vessel (the first of equal distances), and the reference triplets of each main vessel.  Updates
        the tree in place and returns it."""
        if not self.discretized_aorta:
            return self
        for main, branches, side in ((self.discretized_rca_main, self.rca_branches, "rca"),
                                     (self.discretized_lca_main, self.lca_branches, "lca")):
            if not main:
                continue
            c0 = _t3(main[0].centroid)
            k = _first_min([_norm3(_sub3(_t3(a.centroid), c0)) for a in self.discretized_aorta])
            ao = _t3(self.discretized_aorta[k].centroid)
            setattr(self, "ao_" + side, ao)
            setattr(self, side + "_references", _vessel_references(ao, main, branches))
        return self

    def get_summary(self, engine: Optional[N.Engine] = None) -> dict:
        """Lumen morphometry of every vessel of the tree (morphometry.tree_summary; no reference counterpart -- it
        composes the reference's contour measures and geometry-summary rule): ``{"aorta": (summary, table),
        "rca_main": ..., "lca_main": ..., "rca_branches": [...], "lca_branches": [...]}`` with summary = (mla,
        max_stenosis, stenosis_length) and one table row ``[id, area, elliptic_ratio, major, minor_3d, z]`` per slice,
        the slice centroid (anchor) standing in for the frame centroid.  The whole tree is measured in one launch."""
        from .morphometry import tree_summary
        return tree_summary(self, engine)


def discretize_vessel_tree_raw(ao_cl: Centerline, rca_cl: Centerline, lca_cl: Centerline, points_ao, points_rca_main,
                               points_lca_main, side_branches_rca, side_branches_lca, branch_id_rca: int = 0,
                               branch_id_lca: int = 0, step_size: float = 1.0, n_points: int = 100,
                               calculate_ref_pts: bool = True, engine: Optional[N.Engine] = None) -> DiscretizedVesselTree:
    """ccta_py.rs:874-920 -> DiscretizedVesselTree::from_results_dict (vessel_tree.rs:21-83): the aorta (branch 0),
    both main vessels and every side branch (``side_branches_rca[i]`` on branch i + 1 of ``rca_cl``, likewise LCA),
    all in one device pass; then calculate_ref_pts unless it is switched off."""
    jobs = [(ao_cl, points_ao, 0), (rca_cl, points_rca_main, branch_id_rca), (lca_cl, points_lca_main, branch_id_lca)]
    jobs += [(rca_cl, p, i + 1) for i, p in enumerate(side_branches_rca)]
    jobs += [(lca_cl, p, i + 1) for i, p in enumerate(side_branches_lca)]
    res = _discretize_jobs(jobs, step_size, n_points, engine)
    nr = len(side_branches_rca)
    tree = DiscretizedVesselTree(res[0], res[1], res[2], float(step_size), res[3:3 + nr], res[3 + nr:])
    return tree.calculate_ref_pts() if calculate_ref_pts else tree


def _extract_side_branches(results_dict: dict, prefix: str) -> list:
    """discretization_map.py:104-114"""
    out, i = [], 1
    while f"{prefix}_side_{i}" in results_dict:
        out.append(results_dict[f"{prefix}_side_{i}"])
        i += 1
    return out


def discretize_vessel_tree(ao_cl: Centerline, rca_cl: Centerline, lca_cl: Centerline, results_dict: dict,
                           branch_id_rca: int = 0, branch_id_lca: int = 0, step_size: float = 1.0, n_points: int = 100,
                           b_spline: bool = False, bspline_smoothing: float = 100.0, bspline_degree: int = 3,
                           control_plot: bool = False, engine: Optional[N.Engine] = None) -> DiscretizedVesselTree:
    """multimodars/ccta/discretization_map.py:117-205: discretise the aorta (``aorta_points`` + ``rca_removed_points``),
    the main vessels (``rca_points_main`` / ``lca_points_main``) and the side branches (``rca_points_side_1``, ...) of
    a labelled results dict, with reference points.  ``b_spline=True`` raises NotImplementedError here: the B-spline
    path is ``discretize_vessel_tree_bspline``; ``control_plot`` is accepted and ignored."""
    if b_spline:
        raise NotImplementedError("discretize_vessel_tree: b_spline contours are not implemented on this entry point; "
                                  "call discretize_vessel_tree_bspline")
    points_ao = np.concatenate([_p3(results_dict["aorta_points"]), _p3(results_dict["rca_removed_points"])])
    return discretize_vessel_tree_raw(ao_cl, rca_cl, lca_cl, points_ao, results_dict["rca_points_main"],
                                      results_dict["lca_points_main"], _extract_side_branches(results_dict, "rca_points"),
                                      _extract_side_branches(results_dict, "lca_points"), branch_id_rca, branch_id_lca,
                                      step_size, n_points, calculate_ref_pts=True, engine=engine)


# ---- closed B-spline contours (multimodars/ccta/discretization_map.py:16-101) ----------------------------------------
BSPLINE_STATUS = ("fitted", "interpolated", "collapsed", "unchanged_short", "unchanged_zero_chord",
                  "unchanged_nonfinite", "iteration_limit")


@dataclass
class BSplineReport:
    """What mm_bspline_fit_closed_batch says about one contour: ``status`` (a name of BSPLINE_STATUS; ``code`` its
    number), the residual sum of squares ``fp`` and the knot count (0 for an unchanged contour)."""
    status: str
    code: int
    fp: float
    n_knots: int


def bspline_max_points() -> int:
    """MM_BSPLINE_MAX_POINTS: the most points one contour of fit_bspline_contours may have."""
    return int(N.lib().mm_bspline_max_points())


def _bspline_batch(arrays, smoothing: float, degree: int, engine: Optional[N.Engine]):
    """(n, 3) arrays -> (new arrays, centroids (n, 3), reports) from one call of mm_bspline_fit_closed_batch"""
    nc = len(arrays)
    off = np.zeros(nc + 1, dtype=np.int64)
    if nc:
        off[1:] = np.cumsum([a.shape[0] for a in arrays])
    xyz = np.ascontiguousarray(np.concatenate(arrays)) if nc and off[-1] else np.zeros((0, 3))
    out = np.zeros_like(xyz)
    cen = np.zeros((nc, 3))
    status = np.zeros(nc, dtype=np.int32)
    fp = np.zeros(nc)
    nk = np.zeros(nc, dtype=np.int32)
    N.check(N.lib().mm_bspline_fit_closed_batch(_engine(engine).handle, nc, N._ptr(xyz), N._ptr(off), float(smoothing),
                                                int(degree), N._ptr(out), N._ptr(cen), N._ptr(status), N._ptr(fp),
                                                N._ptr(nk)), "fit_bspline_contours")
    new = [out[int(off[j]):int(off[j + 1])].copy() for j in range(nc)]
    reports = [BSplineReport(BSPLINE_STATUS[int(status[j])], int(status[j]), float(fp[j]), int(nk[j])) for j in range(nc)]
    return new, cen, reports


def fit_bspline_contours(contours, smoothing: float = 0.0, degree: int = 3, engine: Optional[N.Engine] = None):
    """_fit_bspline_contour (discretization_map.py:16-83) for a list of contours in one device pass
    (csrc/mm_bspline_kernels.hip): each contour is replaced by as many points on its closed smoothing B-spline --
    scipy's ``splprep(s=smoothing, k=degree, per=True)`` and ``splev`` at ``linspace(0, 1, n, endpoint=False)``,
    restated in exact f64.  ``contours``: ``(n, 3)`` arrays or ``frames.Contour`` objects.  Returns ``(new, reports)``:
    arrays for arrays; for Contour objects new Contour objects with the fitted points, the centroid ``np.mean`` of
    them, and id, original_frame, thicknesses, kind and aortic flags carried over.  ``reports[i]`` is a BSplineReport.
    A contour of fewer than ``degree + 1`` points, with two coinciding consecutive points or with a non-finite
    coordinate comes back with its own points and its status says why.  A degree outside 1..5 or more than
    ``bspline_max_points()`` points raises RuntimeError."""
    from .frames import Contour
    contours = list(contours)
    arrays = [_p3(c.points if isinstance(c, Contour) else c) for c in contours]
    new, cen, reports = _bspline_batch(arrays, smoothing, degree, engine)
    out = []
    for c, a, ce, r in zip(contours, new, cen, reports):
        if isinstance(c, Contour):
            if r.status.startswith("unchanged"):
                out.append(c)                                   # the reference returns the contour itself
            else:
                out.append(Contour(c.id, c.original_frame, a, _t3(ce), c.aortic_thickness, c.pulmonary_thickness, c.kind,
                                   None if c.aortic is None else c.aortic.copy()))
        else:
            out.append(a)
    return out, reports


def fit_bspline_contour(contour, smoothing: float = 0.0, degree: int = 3, engine: Optional[N.Engine] = None):
    """One contour through fit_bspline_contours: ``(new contour, report)``."""
    new, reports = fit_bspline_contours([contour], smoothing, degree, engine)
    return new[0], reports[0]


def replace_contours_with_bsplines(tree: "DiscretizedVesselTree", smoothing: float = 0.0, degree: int = 3,
                                   engine: Optional[N.Engine] = None) -> "DiscretizedVesselTree":
    """_replace_contours_with_bsplines (discretization_map.py:86-101): every contour of the aorta, both main vessels and
    every side branch replaced by its closed B-spline fit, all of them in ONE device pass.  In place; returns the tree.
    The reference points are not recomputed (call ``calculate_ref_pts``)."""
    groups = [tree.discretized_aorta, tree.discretized_rca_main, tree.discretized_lca_main]
    groups += list(tree.rca_branches) + list(tree.lca_branches)
    flat = [c for g in groups for c in g]
    new, _ = fit_bspline_contours(flat, smoothing, degree, engine)
    it = iter(new)
    fitted = [[next(it) for _ in g] for g in groups]
    nr = len(tree.rca_branches)
    tree.discretized_aorta, tree.discretized_rca_main, tree.discretized_lca_main = fitted[0], fitted[1], fitted[2]
    tree.rca_branches = fitted[3:3 + nr]
    tree.lca_branches = fitted[3 + nr:]
    return tree


def discretize_vessel_tree_bspline(ao_cl: Centerline, rca_cl: Centerline, lca_cl: Centerline, results_dict: dict,
                                   branch_id_rca: int = 0, branch_id_lca: int = 0, step_size: float = 1.0,
                                   n_points: int = 100, bspline_smoothing: float = 100.0, bspline_degree: int = 3,
                                   control_plot: bool = False, engine: Optional[N.Engine] = None) -> DiscretizedVesselTree:
    """The ``b_spline=True`` path of multimodars/ccta/discretization_map.py:117-205: discretise without reference
    points, replace every contour by its closed B-spline fit, then ``calculate_ref_pts``.  The defaults are the
    reference's (``bspline_smoothing=100`` collapses a contour whose squared distances to its mean sum to less than
    100 -- every coronary-sized contour of fewer than about 30 points -- to that mean, as the reference does)."""
    points_ao = np.concatenate([_p3(results_dict["aorta_points"]), _p3(results_dict["rca_removed_points"])])
    tree = discretize_vessel_tree_raw(ao_cl, rca_cl, lca_cl, points_ao, results_dict["rca_points_main"],
                                      results_dict["lca_points_main"], _extract_side_branches(results_dict, "rca_points"),
                                      _extract_side_branches(results_dict, "lca_points"), branch_id_rca, branch_id_lca,
                                      step_size, n_points, calculate_ref_pts=False, engine=engine)
    replace_contours_with_bsplines(tree, bspline_smoothing, bspline_degree, engine)
    return tree.calculate_ref_pts()


# ---- mesh morphing (src/ccta/adjust_mesh/scale_coronary.rs:218-260, multimodars/ccta/{labeling,scaling,__init__}.py) --

def _match(keys, queries) -> np.ndarray:
    """For every query row the index of the last key row equal to it by value, -1 if none: the reference's
    ``tuple(v) in set(...)`` / ``{tuple(v): i}`` lookups.  As with Python floats, -0.0 equals 0.0 (folded to +0.0 in
    both copies before the bit-pattern match of mm_match_points) and a row with a NaN equals nothing."""
    k, q = _p3(keys).copy(), _p3(queries).copy()
    k[k == 0.0] = 0.0
    q[q == 0.0] = 0.0
    idx = np.empty(q.shape[0], dtype=np.int64)
    r = N.lib().mm_match_points(N._ptr(k), k.shape[0], N._ptr(q), q.shape[0], N._ptr(idx))
    if r < 0:
        N.check(int(r), "match_points")
    idx[np.isnan(q).any(axis=1)] = -1
    return idx


def centerline_morph_batch(jobs, engine: Optional[N.Engine] = None):
    """centerline_based_diameter_morphing (scale_coronary.rs:218-260) for every (centerline, points, adjustment) job in
    one device pass (csrc/mm_morph_kernels.hip) -> [(moved (n, 3), nearest centerline index (n,) int32)] per job.  A job
    with points and an empty centerline raises RuntimeError (the reference panics)."""
    pts = [_p3(p) for _, p, _ in jobs]
    cls = [c.points for c, _, _ in jobs]
    pt_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int64)
    cl_off = np.concatenate([[0], np.cumsum([len(c) for c in cls])]).astype(np.int64)
    xyz = np.ascontiguousarray(np.concatenate(pts)) if pts else np.zeros((0, 3))
    cl_all = np.ascontiguousarray(np.concatenate(cls)) if cls else None
    adj = np.array([float(a) for _, _, a in jobs], dtype=np.float64)
    out = np.zeros_like(xyz)
    nearest = np.zeros(xyz.shape[0], dtype=np.int32)
    N.check(N.lib().mm_centerline_morph_batch(_engine(engine).handle, len(jobs), N._ptr(cl_all), N._ptr(cl_off),
                                              N._ptr(xyz), N._ptr(pt_off), N._ptr(adj), N._ptr(out), N._ptr(nearest)),
            "centerline_morph_batch")
    return [(out[pt_off[j]:pt_off[j + 1]], nearest[pt_off[j]:pt_off[j + 1]]) for j in range(len(jobs))]


def keep_largest_connected_component(vertices, faces, points) -> np.ndarray:
    """ccta_py.rs:541-580 (host): the vertices, ascending, of the largest connected component of the face adjacency
    restricted to the vertices matching ``points`` bit for bit (the last of duplicated vertices).  Fewer than 2 points,
    or none matching a vertex: the points unchanged.  Of equally large components the one holding the smallest vertex
    index is kept (the reference picks one in hash order and returns it in hash order).  Returns an ``(n, 3)`` array."""
    v, f, p = _p3(vertices), _faces3(faces), _p3(points)
    keep = np.zeros(p.shape[0], dtype=np.int64)
    k = N.lib().mm_keep_largest_component(N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(p), p.shape[0],
                                          N._ptr(keep))
    if k < 0:
        N.check(int(k), "keep_largest_connected_component")
    return p.copy() if k == 0 else v[keep[:k]].copy()


def label_anomalous_region(centerline: Centerline, frames, results: dict, results_key: str = "rca_points",
                           debug_plot: bool = False, engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/labeling.py:283-389: split ``results[results_key]`` into proximal, distal and anomalous points
    along ``centerline`` (find_points_by_cl_region; ``frames``: a FlatGeometry or an (F, 3) array of centroids), keep
    the largest mesh-connected component of each (against ``results["mesh"]``), drop the island points from
    ``results[results_key]`` (order kept) and make ``"aorta_points"`` the mesh vertices, in vertex order, in none of
    rca / lca / proximal / distal / anomalous.  Points are compared by value.  Mutates and returns ``results``, with
    ``"proximal_points"``, ``"distal_points"``, ``"anomalous_points"`` as ``(n, 3)`` arrays.  ``debug_plot`` is
    accepted and ignored."""
    raw = find_points_by_cl_region(centerline, frames, results[results_key], engine=engine)
    vertices, faces = _mesh_parts(results["mesh"])
    v = _p3(vertices)
    parts = [keep_largest_connected_component(v, faces, r) for r in raw]
    dropped = np.concatenate([r[_match(k, r) < 0] for r, k in zip(raw, parts)])
    if dropped.shape[0]:
        pts = _p3(results[results_key])
        results[results_key] = pts[_match(dropped, pts) < 0].copy()
    results["proximal_points"], results["distal_points"], results["anomalous_points"] = parts
    coronary = np.concatenate([_p3(results.get("rca_points", ())), _p3(results.get("lca_points", ())), *parts])
    results["aorta_points"] = v[_match(coronary, v) < 0].copy()
    return results


def _with_vertices(mesh, vertices: np.ndarray):
    """A mesh of the kind given with new vertices: a (vertices, faces) tuple, or a copy of the object (its own
    ``copy()`` where it has one, as trimesh does, else a shallow copy) with ``.vertices`` replaced."""
    if not (hasattr(mesh, "vertices") and hasattr(mesh, "faces")):
        return (vertices, mesh[1])
    m = mesh.copy() if callable(getattr(mesh, "copy", None)) else copy.copy(mesh)
    m.vertices = vertices
    return m


def scale_region_centerline_morphing(mesh, region_points, centerline: Centerline, diameter_adjustment_mm: float,
                                     engine: Optional[N.Engine] = None):
    """multimodars/ccta/scaling.py:16-80: every vertex equal by value to one of ``region_points`` (duplicated vertices
    all) moves by ``diameter_adjustment_mm`` along the direction from its nearest ``centerline`` point; the search and
    the move run on the device in exact f64 (csrc/mm_morph_kernels.hip).  Returns a new mesh of the kind given (see
    ``label_geometry``); the input is not modified.  Without a matching vertex the copy comes back unmoved and
    ``centerline`` is not read."""
    vertices, _ = _mesh_parts(mesh)
    v = _p3(vertices)
    moved = v.copy()
    sel = np.flatnonzero(_match(region_points, v) >= 0)
    if sel.size:
        moved[sel] = centerline_morph_batch([(centerline, v[sel], diameter_adjustment_mm)], engine)[0][0]
    return _with_vertices(mesh, moved)


SYNC_KEYS = ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "lca_removed_points", "proximal_points",
             "distal_points", "anomalous_points", "boundary_points")


def sync_results_to_mesh(results: dict, old_mesh, new_mesh) -> dict:
    """multimodars/ccta/scaling.py:301-351: a new dict with ``"mesh"`` = ``new_mesh`` and the point lists of
    SYNC_KEYS and of every ``boundary_points_*`` key remapped from their positions in ``old_mesh`` to the same vertices
    of ``new_mesh`` (points equal by value; the last old vertex wins; unmatched points are dropped).  Missing or empty
    keys and all other keys are left as they are."""
    ov, nv = _p3(_mesh_parts(old_mesh)[0]), _p3(_mesh_parts(new_mesh)[0])
    updated = dict(results)
    updated["mesh"] = new_mesh
    for key in SYNC_KEYS + tuple(sorted(k for k in updated if k.startswith("boundary_points_"))):
        pts = updated.get(key)
        if pts is None or len(pts) == 0:
            continue
        idx = _match(ov, pts)
        updated[key] = nv[idx[idx >= 0]].copy()
    return updated


def scale(results: dict, cl_vessel: Centerline, cl_aorta: Centerline, aligned_frames: G.FlatGeometry,
          engine: Optional[N.Engine] = None) -> dict:
    """multimodars/ccta/__init__.py:171-258: the proximal / distal scalings (find_distal_and_proximal_scaling) and the
    aortic one (find_aorta_scaling) against ``aligned_frames``, then three morph + sync rounds: the distal points about
    ``cl_vessel``, the aortic region (``aorta_points`` followed by ``rca_removed_points``) about ``cl_aorta``, the
    proximal points about ``cl_vessel``.  Returns the synced results with the scaled mesh."""
    prox_scaling, distal_scaling = find_distal_and_proximal_scaling(aligned_frames, cl_vessel, results, engine=engine)
    aortic_scaling = find_aorta_scaling(aligned_frames, cl_aorta, results, engine=engine)
    m = scale_region_centerline_morphing(results["mesh"], results["distal_points"], cl_vessel, distal_scaling, engine)
    results = sync_results_to_mesh(results, results["mesh"], m)
    aortic = np.concatenate([_p3(results["aorta_points"]), _p3(results["rca_removed_points"])])
    m = scale_region_centerline_morphing(results["mesh"], aortic, cl_aorta, aortic_scaling, engine)
    results = sync_results_to_mesh(results, results["mesh"], m)
    m = scale_region_centerline_morphing(results["mesh"], results["proximal_points"], cl_vessel, prox_scaling, engine)
    return sync_results_to_mesh(results, results["mesh"], m)


# ---- mesh trimming (multimodars/ccta/boundary.py, stitching.py:18-352, __init__.py:341-429) -------------------------

TRIM_KEYS = ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "lca_removed_points", "proximal_points",
             "distal_points")
BOUNDARY_RING_PREFIX = "boundary_points_"


def _checked_faces(faces, nv: int) -> np.ndarray:
    f = _faces3(faces)
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise ValueError(f"face index out of range [0, {nv})")
    return f


def _target(target_n) -> int:
    if target_n is None:
        return -1
    if int(target_n) < 1:
        raise ValueError("target_n must be at least 1 (or None)")
    return int(target_n)


def _rings(ring_len: np.ndarray, ring_idx: np.ndarray, n_rings: int) -> list:
    ends = np.cumsum(ring_len[:n_rings])
    return [ring_idx[e - n:e].copy() for n, e in zip(ring_len[:n_rings], ends)]


def build_adjacency_map(faces) -> dict:
    """_processing.py:1476-1505 / ccta_py.rs:507-525: every vertex of ``faces`` -> the set of vertices it shares an edge
    with (host, the labelling's adjacency builder).  ``build_adjacency_map([[0, 1, 2], [1, 2, 3]])[1] == {0, 2, 3}``."""
    f = _faces3(faces)
    if f.size == 0:
        return {}
    if f.min() < 0:
        raise ValueError("negative face index")
    nv = int(f.max()) + 1
    off = np.zeros(nv + 1, dtype=np.int64)
    nb = np.zeros(6 * f.shape[0], dtype=np.int64)
    N.check(N.lib().mm_build_adjacency(N._ptr(f), f.shape[0], nv, N._ptr(off), N._ptr(nb)), "build_adjacency_map")
    return {v: set(nb[off[v]:off[v + 1]].tolist()) for v in range(nv) if off[v + 1] > off[v]}


def open_boundary_edges(faces, engine: Optional[N.Engine] = None) -> np.ndarray:
    """boundary.py:26-43: the edges used by exactly one face, each as (smaller, larger), in lexicographic order (as
    ``np.unique(axis=0)`` gives them), ``(E, 2)`` int64.  A degenerate face's ``(v, v)`` edge counts like any other.
    The edges are counted on the device (csrc/mm_trim_kernels.hip)."""
    f = _faces3(faces)
    if f.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if f.min() < 0:
        raise ValueError("negative face index")
    out = np.zeros((3 * f.shape[0], 2), dtype=np.int64)
    k = N.lib().mm_open_boundary_edges(_engine(engine).handle, N._ptr(f), f.shape[0], int(f.max()) + 1, N._ptr(out))
    if k < 0:
        N.check(int(k), "open_boundary_edges")
    return out[:k].copy()


def boundary_rings_from_edges(edges, vertices, seeds=None, target_n=None, despike_cos: float = 0.0,
                              clean: bool = False):
    """The host rim logic on an open-edge list (no device): the rim graph, the rims touching ``seeds`` (all without
    seeds), the walk (DESIGN §4.11 for its fixed rule) and, without ``clean``, the reduction to ``target_n`` rings
    (order_boundary_rings).  With ``clean``, one round of clean_open_boundary.  Returns (rings, drop, rim): the rim
    vertices touching the seeds and the vertices that round culls (ascending); rings only where nothing is culled."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    v = _p3(vertices)
    s = np.ascontiguousarray(np.asarray(sorted(seeds) if seeds is not None else [], dtype=np.int64))
    cap = 2 * e.shape[0] + 1
    ring_len, ring_idx, drop, rim = (np.zeros(cap, dtype=np.int64) for _ in range(4))
    counts = np.zeros(4, dtype=np.int64)
    rc = N.lib().mm_boundary_rings(N._ptr(e), e.shape[0], N._ptr(s), s.shape[0], N._ptr(v), v.shape[0],
                                   _target(target_n), float(despike_cos), int(bool(clean)), N._ptr(ring_len),
                                   N._ptr(ring_idx), N._ptr(drop), N._ptr(rim), N._ptr(counts))
    if rc == -2 and e.size and (e.min() < 0 or e.max() >= v.shape[0]):
        raise ValueError("edge end out of range")
    N.check(rc, "boundary_rings_from_edges")
    return _rings(ring_len, ring_idx, int(counts[0])), drop[:counts[2]].copy(), rim[:counts[3]].copy()


def order_boundary_rings(faces, vertices, seeds=None, target_n=None, engine: Optional[N.Engine] = None) -> list:
    """boundary.py:223-254: the open boundary of ``faces`` ordered into rings (int64 vertex index arrays, largest
    first) without touching the mesh; only the rims holding one of ``seeds`` when given; reduced to ``target_n`` rings
    by joining nearest endpoints when given.  The reference's set-order walk is replaced by a fixed rule (DESIGN
    §4.11)."""
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    edges = open_boundary_edges(f, engine) if f.size else np.zeros((0, 2), dtype=np.int64)
    return boundary_rings_from_edges(edges, v, seeds, target_n)[0]


def clean_open_boundary(faces, vertices, seeds, target_n=1, despike_cos: float = 0.0, max_rounds: int = 64,
                        engine: Optional[N.Engine] = None):
    """boundary.py:257-325: cull the rim vertices of ``faces`` that cannot form a clean ring (degree != 2, then the
    bump spikes above ``despike_cos``), round by round, each round re-deriving the surviving faces and their open edges
    on the device.  Returns (drop, rings): the culled vertices as a sorted int64 array and the rings (int64 arrays,
    largest first, reduced to ``target_n``)."""
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    s = np.ascontiguousarray(np.asarray(sorted(seeds) if seeds is not None else [], dtype=np.int64))
    nv = v.shape[0]
    drop, ring_len, ring_idx = (np.zeros(nv + 1, dtype=np.int64) for _ in range(3))
    counts = np.zeros(3, dtype=np.int64)
    N.check(N.lib().mm_clean_open_boundary(_engine(engine).handle, N._ptr(f), f.shape[0], N._ptr(v), nv, N._ptr(s),
                                           s.shape[0], _target(target_n), float(despike_cos), int(max_rounds),
                                           N._ptr(drop), N._ptr(ring_len), N._ptr(ring_idx), N._ptr(counts)),
            "clean_open_boundary")
    return drop[:counts[2]].copy(), _rings(ring_len, ring_idx, int(counts[0]))


def _with_mesh(mesh, vertices: np.ndarray, faces: np.ndarray):
    """A mesh of the kind given with new vertices and faces (see _with_vertices)."""
    if not (hasattr(mesh, "vertices") and hasattr(mesh, "faces")):
        return (vertices, faces)
    m = mesh.copy() if callable(getattr(mesh, "copy", None)) else copy.copy(mesh)
    m.vertices = vertices
    m.faces = faces
    return m


def _trim(v: np.ndarray, f: np.ndarray, region: np.ndarray, mode: int, target_n, engine):
    """mm_trim_mesh: (kept vertices, remapped kept faces, rings in the old vertex indices)."""
    nv, nf = v.shape[0], f.shape[0]
    out_v = np.zeros((nv, 3), dtype=np.float64)
    out_f = np.zeros((nf, 3), dtype=np.int64)
    ring_len, ring_idx = np.zeros(nv + 1, dtype=np.int64), np.zeros(nv + 1, dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    N.check(N.lib().mm_trim_mesh(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), nf, N._ptr(region), mode,
                                 _target(target_n) if mode != 2 else 1, 0.0, 64, N._ptr(out_v), N._ptr(out_f),
                                 N._ptr(ring_len), N._ptr(ring_idx), N._ptr(counts)), "trim_mesh")
    return out_v[:counts[0]].copy(), out_f[:counts[1]].copy(), _rings(ring_len, ring_idx, int(counts[2]))


def _store_boundary_rings(updated: dict, vertices: np.ndarray, rings: list) -> None:
    """stitching.py:18-37: stale ``boundary_points_*`` keys go, then ``boundary_points_1..k`` (one ring each, walk
    order) and the flat ``boundary_points``."""
    for key in [k for k in updated if k.startswith(BOUNDARY_RING_PREFIX)]:
        del updated[key]
    per_ring = [vertices[r] for r in rings]
    for n, pts in enumerate(per_ring, start=1):
        updated[f"{BOUNDARY_RING_PREFIX}{n}"] = pts
    updated["boundary_points"] = np.concatenate(per_ring) if per_ring else np.zeros((0, 3), dtype=np.float64)


def _region_points(results: dict, keys) -> np.ndarray:
    parts = [_p3(results.get(k, ())) for k in keys]
    return np.concatenate(parts) if parts else np.zeros((0, 3), dtype=np.float64)


def _trim_results(results: dict, keys: list, mode: int, target_boundaries, engine) -> Optional[dict]:
    pts = _region_points(results, keys)
    if pts.shape[0] == 0:
        return None
    vertices, faces = _mesh_parts(results["mesh"])
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    idx = _match(v, pts)
    idx = idx[idx >= 0]
    if idx.size == 0:
        return None
    region = np.zeros(v.shape[0], dtype=np.uint8)
    region[idx] = 1
    new_v, new_f, rings = _trim(v, f, region, mode, target_boundaries, engine)
    updated = dict(results)
    updated["mesh"] = _with_mesh(results["mesh"], new_v, new_f)
    _store_boundary_rings(updated, v, rings)
    return updated


def _filter_to(points, vertices: np.ndarray) -> np.ndarray:
    p = _p3(points)
    return p[_match(vertices, p) >= 0].copy()


def remove_labeled_points_from_mesh(results: dict, region_keys="anomalous_points", target_boundaries: int = 1,
                                    engine: Optional[N.Engine] = None) -> dict:
    """stitching.py:110-240: delete the mesh vertices equal by value to the points under ``region_keys`` (a key or a
    list of keys) and every face touching them, clean the rim the cut leaves (clean_open_boundary seeded by the kept
    vertices that shared a face with a removed one; the vertices it culls go too) and remap the faces.  Returns a new
    dict: ``"mesh"`` the trimmed mesh (of the kind given), the region keys cleared to ``(0, 3)`` arrays, the rings in
    ``"boundary_points_1"``, ``"boundary_points_2"``, ... and flat in ``"boundary_points"``, and TRIM_KEYS filtered to
    the surviving vertices.  Nothing to remove, or nothing matching: ``results`` itself, unchanged.  Face membership,
    open edges and compaction run on the device (csrc/mm_trim_kernels.hip)."""
    keys = [region_keys] if isinstance(region_keys, str) else list(region_keys)
    updated = _trim_results(results, keys, 0, target_boundaries, engine)
    if updated is None:
        return results
    new_v = _p3(_mesh_parts(updated["mesh"])[0])
    for key in keys:
        updated[key] = np.zeros((0, 3), dtype=np.float64)
    for key in TRIM_KEYS:
        if key in updated and key not in keys:
            updated[key] = _filter_to(updated[key], new_v)
    return updated


def keep_labeled_points_from_mesh(results: dict, region_key, target_boundaries: int = 1,
                                  engine: Optional[N.Engine] = None) -> dict:
    """stitching.py:243-352: keep only the mesh vertices equal by value to the points under ``region_key`` (a key or a
    list of keys, their union) and the faces with all corners among them, clean the rim as
    remove_labeled_points_from_mesh does and filter TRIM_KEYS and the region keys to the surviving vertices.  Nothing
    to keep, or nothing matching: ``results`` itself, unchanged."""
    keys = [region_key] if isinstance(region_key, str) else list(region_key)
    updated = _trim_results(results, keys, 1, target_boundaries, engine)
    if updated is None:
        return results
    new_v = _p3(_mesh_parts(updated["mesh"])[0])
    for key in TRIM_KEYS + tuple(keys):
        if key in updated:
            updated[key] = _filter_to(updated[key], new_v)
    return updated


def extract_region_with_border_faces(mesh, region_points, engine: Optional[N.Engine] = None):
    """__init__.py:341-373: the sub-mesh of every face with a corner equal by value to one of ``region_points``, with
    the vertices those faces use (in vertex order) and the faces remapped.  No matching vertex: an empty mesh of the
    kind given."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    idx = _match(v, region_points)
    idx = idx[idx >= 0]
    if idx.size == 0:
        return _with_mesh(mesh, np.zeros((0, 3), dtype=np.float64), np.zeros((0, 3), dtype=np.int64))
    region = np.zeros(v.shape[0], dtype=np.uint8)
    region[idx] = 1
    new_v, new_f, _ = _trim(v, f, region, 2, None, engine)
    return _with_mesh(mesh, new_v, new_f)


def write_stl(path, vertices, faces) -> None:
    """A binary STL of the triangles: our own 80-byte header, float32 unit face normals (zero for a degenerate face,
    computed in f64) and float32 vertices."""
    v, f = _p3(vertices), _faces3(faces)
    tri = v[f] if f.size else np.zeros((0, 3, 3), dtype=np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) if f.size else np.zeros((0, 3))
    length = np.sqrt((n * n).sum(axis=1)) if f.size else np.zeros(0)
    unit = np.zeros_like(n)
    ok = length > 0
    unit[ok] = n[ok] / length[ok, None]
    rec = np.zeros(f.shape[0], dtype=np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    rec["n"] = unit
    rec["v"] = tri
    header = b"multimoda-rs_amd binary STL".ljust(80, b" ")
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(np.uint32(f.shape[0]).tobytes())
        fh.write(rec.tobytes())


def export_section_stl(results: dict, type: str = "all", output_dir=None, engine: Optional[N.Engine] = None) -> str:
    """__init__.py:376-429: write ``<type>.stl`` into ``output_dir`` (default: the working directory) as a binary STL
    (write_stl): ``"all"`` the whole mesh, ``"aorta"`` the mesh keep_labeled_points_from_mesh leaves of
    aorta_points, rca_removed_points and lca_removed_points, ``"rca"`` / ``"lca"`` extract_region_with_border_faces
    of rca_points / lca_points.  Returns the path written."""
    import os
    out_dir = "." if output_dir is None else str(output_dir)
    os.makedirs(out_dir, exist_ok=True)
    region_keys = {"aorta": "aorta_points", "rca": "rca_points", "lca": "lca_points"}
    mesh = results["mesh"]
    if type == "all":
        sub = mesh
    elif type == "aorta":
        sub = keep_labeled_points_from_mesh(results, ["aorta_points", "rca_removed_points", "lca_removed_points"],
                                            engine=engine)["mesh"]
    elif type in region_keys:
        sub = extract_region_with_border_faces(mesh, results.get(region_keys[type], ()), engine=engine)
    else:
        raise ValueError(f"Unknown export type {type!r}. Choose one of: 'all', 'aorta', 'rca', 'lca'.")
    path = os.path.join(out_dir, f"{type}.stl")
    write_stl(path, *_mesh_parts(sub))
    return path


# ---- stitching (multimodars/ccta/stitching.py:69-107, 355-481, 1148-1334; ccta/__init__.py:261-338) -----------------

ASSEMBLE_REPORT_KEYS = tuple(name for name, _ in N.MMAssembleReport._fields_)


def fix_mesh_winding(faces, engine: Optional[N.Engine] = None) -> np.ndarray:
    """ccta_py.rs:596-700: ``faces`` with a consistent winding, ``(F, 3)`` int64.  Two faces are adjacent when they share
    an edge that exactly two faces own; in every connected component the face with the smallest index keeps its corner
    order and every other face is reversed ``(a, b, c) -> (c, b, a)`` iff its parity to that face is odd.  For an
    orientable component that is the reference's BFS result; a component that is not orientable has no consistent
    answer and its flips are unspecified.  Runs on the device (csrc/mm_weld_kernels.hip: a union-find with parity, a
    logarithmic number of launches whatever the mesh's diameter)."""
    return _fix_winding(faces, engine)[0]


def _fix_winding(faces, engine):
    f = _faces3(faces)
    if f.size and (f.min() < 0 or f.max() >= 2 ** 31 - 1):
        raise ValueError("face index out of range [0, 2^31 - 1)")
    out = np.zeros_like(f)
    info = np.zeros(3, dtype=np.int64)
    N.check(N.lib().mm_fix_winding(_engine(engine).handle, N._ptr(f), f.shape[0], N._ptr(out), N._ptr(info)),
            "fix_mesh_winding")
    return out, {"n_flipped_faces": int(info[0]), "n_winding_conflicts": int(info[1]), "winding_rounds": int(info[2])}


def assemble_mesh(parts, merge_digits: int = 3, fix_winding: bool = True, fix_inversion: bool = True,
                  engine: Optional[N.Engine] = None):
    """The tail of stitch_ccta_to_intravascular (stitching.py:455-468) on the device: ``parts`` (``(vertices, faces)``
    pairs or meshes with ``.vertices`` / ``.faces``) concatenated, vertices welded where ``rint(c * 10**merge_digits)``
    agrees in every coordinate (the smallest index of a group stays, bit for bit; vertices no face names are dropped),
    faces with a repeated index and later repeats of a vertex set dropped, the winding made consistent
    (fix_mesh_winding) and, where the signed volume is negative, every face reversed.  Returns ``(vertices, faces,
    report)``; ``report`` holds ASSEMBLE_REPORT_KEYS and ``"watertight"``.  Holes are not filled: the report says
    whether any are left.  include/mm_ccta.h states every rule."""
    vs, fs = [], []
    for part in parts:
        pv, pf = _mesh_parts(part)
        pv = _p3(pv)
        vs.append(pv)
        fs.append(_checked_faces(pf, pv.shape[0]))
    voff = np.zeros(len(vs) + 1, dtype=np.int64)
    foff = np.zeros(len(vs) + 1, dtype=np.int64)
    if vs:
        voff[1:] = np.cumsum([a.shape[0] for a in vs])
        foff[1:] = np.cumsum([a.shape[0] for a in fs])
    v = np.ascontiguousarray(np.concatenate(vs)) if vs else np.zeros((0, 3), dtype=np.float64)
    f = np.ascontiguousarray(np.concatenate(fs)) if fs else np.zeros((0, 3), dtype=np.int64)
    out_v, out_f = np.zeros_like(v), np.zeros_like(f)
    rep = N.MMAssembleReport()
    N.check(N.lib().mm_mesh_assemble(_engine(engine).handle, len(vs), N._ptr(v), N._ptr(voff), N._ptr(f), N._ptr(foff),
                                     int(merge_digits), int(bool(fix_winding)), int(bool(fix_inversion)), N._ptr(out_v),
                                     N._ptr(out_f), C.byref(rep)), "assemble_mesh")
    report = {k: getattr(rep, k) for k in ASSEMBLE_REPORT_KEYS}
    report["watertight"] = report["n_open_edges"] == 0 and report["n_nonmanifold_edges"] == 0
    return out_v[:rep.n_vertices].copy(), out_f[:rep.n_faces].copy(), report


def assign_rings_to_ends(rings, prox_centroid, dist_centroid):
    """stitching.py:69-107: ``(i, j, leftover)``: the ring for the proximal end, the ring for the distal end (the
    ordered pair of distinct rings with the smallest summed centroid distance, the first minimum in loop order) and the
    indices of the other rings."""
    rs = [_p3(r) for r in rings]
    off = np.zeros(len(rs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in rs])
    flat = np.ascontiguousarray(np.concatenate(rs)) if rs else np.zeros((0, 3), dtype=np.float64)
    pair = np.zeros(2, dtype=np.int64)
    p, d = _p3(prox_centroid), _p3(dist_centroid)
    N.check(N.lib().mm_assign_rings_to_ends(N._ptr(flat), N._ptr(off), len(rs), N._ptr(p), N._ptr(d), N._ptr(pair)),
            "assign_rings_to_ends")
    i, j = int(pair[0]), int(pair[1])
    return i, j, [k for k in range(len(rs)) if k not in (i, j)]


def rotate_ring_start(boundary_pts, mode: str = "nearest_iv", iv_pt=None) -> np.ndarray:
    """_rotate_to_nearest_iv (stitching.py:1154-1159) / _adjust_start_point_by_z (:1148-1151): the ring rotated so that
    the first point nearest to ``iv_pt`` (``"nearest_iv"``) or the first point of largest z (``"highest_z"``) leads."""
    b = _p3(boundary_pts)
    if mode not in ("nearest_iv", "highest_z"):
        raise ValueError(f"unknown start mode {mode!r}")
    q = _p3(iv_pt) if mode == "nearest_iv" else None
    k = N.lib().mm_ring_start(N._ptr(b), b.shape[0], 0 if mode == "nearest_iv" else 1, N._ptr(q))
    if k < 0:
        N.check(int(k), "rotate_ring_start")
    return np.concatenate([b[k:], b[:k]])


def fix_ring_direction(boundary_pts, iv_pts, mode: str = "distance", point_step: int = 1) -> np.ndarray:
    """_fix_ring_direction_by_distance (stitching.py:1213-1239, ``mode="distance"``) / _fix_ring_direction_by_winding
    (:1242-1259, ``mode="winding"``): the ring as it is or reversed behind its first point."""
    b, iv = _p3(boundary_pts), _p3(iv_pts)
    if mode not in ("distance", "winding"):
        raise ValueError(f"unknown direction mode {mode!r}")
    rc = N.lib().mm_ring_direction(N._ptr(b), b.shape[0], N._ptr(iv), iv.shape[0], 0 if mode == "distance" else 1,
                                   int(point_step))
    if rc < 0:
        N.check(rc, "fix_ring_direction")
    return np.concatenate([b[:1], b[:0:-1]]) if rc else b


def stitch_rings(boundary_pts, iv_pts, outward_direction=None):
    """_stitch_rings (stitching.py:1262-1334): the closed strip between a boundary ring and an IV ring,
    ``(vertices, faces)`` with the boundary vertices first and exactly ``n_b + n_iv`` faces; the whole strip is reversed
    when its mean unit face normal points against ``outward_direction``."""
    b, iv = _p3(boundary_pts), _p3(iv_pts)
    if b.shape[0] < 3 or iv.shape[0] < 3:
        raise ValueError(f"Need at least 3 points per ring to stitch (got boundary={b.shape[0]}, iv={iv.shape[0]}).")
    faces = np.zeros((b.shape[0] + iv.shape[0], 3), dtype=np.int64)
    o = None if outward_direction is None else _p3(outward_direction)
    rc = N.lib().mm_stitch_rings(N._ptr(b), b.shape[0], N._ptr(iv), iv.shape[0], N._ptr(o), N._ptr(faces))
    if rc < 0:
        N.check(rc, "stitch_rings")
    return np.concatenate([b, iv]), faces


def _downsample_geometry(g: G.FlatGeometry, n: int):
    """PyGeometry.downsample (py_geometry.rs:394, contour.rs:47-58) of the lumen contours: a contour of more than ``n``
    points keeps the points ``int(i * (len / n))``.  Returns the list of per-frame ``(k, 3)`` arrays."""
    out = []
    for i in range(g.n_frames):
        pts = g.frame_lumen(i)
        if pts.shape[0] > n:
            idx = (np.arange(n, dtype=np.float64) * (pts.shape[0] / float(n))).astype(np.int64)
            pts = pts[idx]
        out.append(np.ascontiguousarray(pts, dtype=np.float64))
    return out


def geometry_tube(contours, centroid0):
    """geometry_to_trimesh (_converters.py:1018-1085): ``(vertices, faces)`` of the tube through ``contours`` (equally
    many points each), one quad strip per adjacent pair, reversed as a whole when its first face looks at
    ``centroid0``."""
    cs = [_p3(c) for c in contours]
    if len(cs) < 2:
        raise ValueError("Need at least two contours to build a mesh.")
    n = cs[0].shape[0]
    if n < 1 or any(c.shape[0] != n for c in cs):
        raise ValueError("every contour needs the same, positive number of points")
    v = np.ascontiguousarray(np.concatenate(cs))
    faces = np.zeros((2 * (len(cs) - 1) * n, 3), dtype=np.int64)
    rc = N.lib().mm_tube_faces(N._ptr(v), len(cs), n, N._ptr(_p3(centroid0)), N._ptr(faces))
    if rc < 0:
        N.check(rc, "geometry_tube")
    return v, faces


def _result_rings(results: dict, mesh, engine) -> list:
    """_boundary_rings (stitching.py:40-66): the rings under ``boundary_points_<n>``, or, failing that, those of the
    mesh's open edges that hold a point of the flat ``boundary_points``."""
    rings = []
    n = 1
    while f"{BOUNDARY_RING_PREFIX}{n}" in results:
        r = _p3(results[f"{BOUNDARY_RING_PREFIX}{n}"])
        if r.shape[0]:
            rings.append(r)
        n += 1
    if rings:
        return rings
    flat = _p3(results.get("boundary_points", ()) if results.get("boundary_points", None) is not None else ())
    if flat.shape[0] == 0:
        return []
    v, f = _mesh_parts(mesh)
    v = _p3(v)
    idx = _match(v, flat)
    seeds = set(int(i) for i in idx[idx >= 0])
    return [v[r] for r in order_boundary_rings(f, v, seeds, engine=engine)]


def stitch_ccta_to_intravascular(iv_geometry: G.FlatGeometry, mesh, results: dict, n_points_iv_cont: int = 100,
                                 prox_start_mode: str = "nearest_iv", dist_start_mode: str = "nearest_iv",
                                 condition_rims: bool = False, engine: Optional[N.Engine] = None) -> dict:
    """stitching.py:355-481 behind the rim conditioning: this function sews the rings it is given as they are.  The
    conditioning of _prepare_prox_dist_boundary_pts (:484-1064: plane flattening, smoothing, respacing, ostium clamp,
    densification) is a step of its own, ``condition_boundary_rings``, whose result goes straight in here as ``mesh`` and
    ``results``; ``stitch_conditioned`` runs the whole line.  ``condition_rims=True`` still raises NotImplementedError
    and the arguments that only steer the conditioning (``proximal_is_ostium``, ``clamp_overshoot``,
    ``boundary_point_ratio``) are not accepted here: they belong to ``condition_boundary_rings``.  The lumen contours are
    downsampled to
    ``n_points_iv_cont`` points, the two rims (``boundary_points_<n>`` of ``results``, else the mesh's open edges) are
    assigned to the ends as whole rings, rotated to their start (``"nearest_iv"`` | ``"highest_z"``; ``"highest_z"``
    also rotates every frame so that the first frame's highest point leads, the last of equal ones, as the reference's
    sort_frame_points does) and given the IV ring's direction, both strips are stitched, and ``[mesh, proximal strip,
    distal strip, IV tube]`` are assembled on the device (assemble_mesh).  Returns a new dict with the reference's keys
    ``prox_boundary_points``, ``dist_boundary_points``, ``anomalous_points``, ``rca_points``, ``mesh`` and
    ``stitch_report`` (the assembly's report; holes are not filled)."""
    if condition_rims:
        raise NotImplementedError("condition_rims=True: the rim conditioning of _prepare_prox_dist_boundary_pts "
                                  "(stitching.py:484-1060) is not part of this package yet")
    for m in (prox_start_mode, dist_start_mode):
        if m not in ("nearest_iv", "highest_z"):
            raise ValueError(f"unknown start mode {m!r}")
    frames = _downsample_geometry(iv_geometry, int(n_points_iv_cont))
    if len(frames) < 2:
        raise ValueError("Need at least two contours to build a mesh.")
    iv_points = np.concatenate(frames)
    prox_c, dist_c = iv_geometry.centroids[0].copy(), iv_geometry.centroids[-1].copy()
    prox_outward, dist_outward = prox_c - dist_c, dist_c - prox_c

    rings = _result_rings(results, mesh, engine)
    if len(rings) < 2:
        raise ValueError(f"Stitching needs a proximal and a distal boundary ring, but {len(rings)} were found. Re-run "
                         f"the removal with target_boundaries=2 so both rims are kept as separate rings.")
    i, j, _ = assign_rings_to_ends(rings, prox_c, dist_c)
    prox_b, dist_b = rings[i], rings[j]
    prox_step = max(1, frames[0].shape[0] // prox_b.shape[0])
    dist_step = max(1, frames[-1].shape[0] // dist_b.shape[0])

    if "highest_z" in (prox_start_mode, dist_start_mode):                  # sort_frame_points (geometry.rs:257-276)
        z = frames[0][:, 2]
        shift = int(z.shape[0] - 1 - np.argmax(z[::-1]))                   # max_by: the last of equal maxima
        frames = [np.concatenate([f[shift % f.shape[0]:], f[:shift % f.shape[0]]]) if f.shape[0] else f for f in frames]
    ends = ((prox_b, frames[0], prox_start_mode, prox_step), (dist_b, frames[-1], dist_start_mode, dist_step))
    fixed = []
    for ring, iv, mode, step in ends:
        ring = rotate_ring_start(ring, mode, iv[0])
        fixed.append(fix_ring_direction(ring, iv, "winding", 1) if mode == "highest_z"
                     else fix_ring_direction(ring, iv, "distance", step))
    prox_b, dist_b = fixed
    prox_patch = stitch_rings(prox_b, frames[0], prox_outward)
    dist_patch = stitch_rings(dist_b, frames[-1], dist_outward)
    lc = iv_geometry.lumen_centroids
    c0 = lc[0] if lc is not None and (iv_geometry.has_lumen_centroid is None or iv_geometry.has_lumen_centroid[0]) \
        else iv_geometry.centroids[0]
    tube = geometry_tube(frames, c0)
    mv, mf = _mesh_parts(mesh)
    new_v, new_f, report = assemble_mesh([(mv, mf), prox_patch, dist_patch, tube], engine=engine)

    out = dict(results)
    out["prox_boundary_points"] = prox_b
    out["dist_boundary_points"] = dist_b
    out["anomalous_points"] = iv_points
    out["rca_points"] = np.concatenate([iv_points, _p3(results.get("distal_points", ())),
                                        _p3(results.get("proximal_points", ()))])
    out["mesh"] = _with_mesh(mesh, new_v, new_f)
    out["stitch_report"] = report
    return out


def stitch(results: dict, geometry: G.FlatGeometry, region_remove=("anomalous_points", "proximal_points"),
           prox_start_mode: str = "highest_z", dist_start_mode: str = "nearest_iv",
           engine: Optional[N.Engine] = None, fill_holes: bool = False, smooth=False, refine=False, relax=False,
           flip=False, collapse=False, repair=False, check_intersections: bool = False) -> dict:
    """ccta/__init__.py:261-338: remove the labelled regions ``region_remove`` from the CCTA mesh and stitch what is left
    to the intravascular ``geometry``.  The reference's wrapper leaves ``target_boundaries`` of the removal at its
    default of 1 although its own stitch then asks for two rings; this one passes ``target_boundaries=2``.  The
    reference always ends with ``manual_hole_fill`` (:330); here that is ``fill_holes=True``: the
    stitched mesh goes through ``manual_hole_fill`` and the result carries ``fill_report`` beside ``stitch_report``.
    The default leaves the holes open, and ``stitch_report`` says whether the result is watertight.  ``smooth=True``, or
    a dict of ``smooth_mesh`` keywords (``band``, ``pinned``, ``iterations`` ...), then runs the smoothing half of the
    reference's post-processing (``smooth_mesh``; the remesh is not part of this package) on the mesh: the point lists
    follow the moved vertices (``sync_results_to_mesh``) and the result carries ``smooth_report``.  The default
    ``smooth=False`` changes nothing.  ``refine=True``, or a dict of ``refine_mesh`` keywords, splits the long edges
    (``refine_mesh``, the edge split of the reference's remesh) behind the hole fill and in front of the smoothing: a
    new vertex joins, in ascending order, every point list that holds both its parents, and the result carries
    ``refine_report``.  The default ``refine=False`` changes nothing.  ``relax=True``, or a dict of ``relax_mesh``
    keywords, evens the vertices out on the surface (``relax_mesh`` against the mesh itself) behind the refinement and in
    front of the smoothing: the point lists follow and the result carries ``relax_report``.  The default ``relax=False``
    changes nothing.  ``flip=True``, or a dict of ``flip_edges`` keywords, evens the valences the split left
    (``flip_edges``) behind the refinement and in front of the relaxation, which is where it pays; no vertex moves, so
    the point lists stay, and the result carries ``flip_report``.  Where ``pinned`` is not given, the vertices of the
    intravascular lumen (``anomalous_points``) are pinned: its triangulation stays.  The default ``flip=False`` changes
    nothing.  ``collapse=True``, or a dict of ``collapse_edges`` keywords, removes the short edges that the seam strips,
    the rim fans and the split leave (``collapse_edges``) behind the refinement and in front of the flips, the
    intravascular lumen pinned in the same way: a removed vertex leaves every point list that holds it by value, and the
    result carries ``collapse_report``.  The default ``collapse=False`` changes nothing.  ``repair=True``, or a dict of
    ``repair_mesh`` keywords, runs ``repair_mesh`` between the assembly and the hole filling, so that a rim with a pinch
    vertex or beside a non-manifold edge becomes a loop the fill closes; its report goes under ``"repair"``.  The default
    ``repair=False`` changes nothing.  ``check_intersections=True`` ends with the self-intersection check of the final
    mesh (``mesh_self_intersections``): the result carries its report under ``intersection_report``.  The default
    ``check_intersections=False`` changes nothing."""
    keys = [region_remove] if isinstance(region_remove, str) else list(region_remove)
    updated = remove_labeled_points_from_mesh(results, keys, target_boundaries=2, engine=engine)
    out = stitch_ccta_to_intravascular(geometry, updated["mesh"], updated, prox_start_mode=prox_start_mode,
                                       dist_start_mode=dist_start_mode, engine=engine)
    out = _repair_result(out, repair, engine)
    if fill_holes:
        v, f = _mesh_parts(out["mesh"])
        new_v, new_f, report = _fill(v, f, True, engine)
        out["mesh"] = _with_mesh(out["mesh"], new_v, new_f)
        out["fill_report"] = report
    out = _collapse_result(_refine_result(out, refine, engine), collapse, engine)
    out = _smooth_result(_relax_result(_flip_result(out, flip, engine), relax, engine), smooth, engine)
    if check_intersections:
        out = dict(out)
        out["intersection_report"] = _intersection_report(out["mesh"], engine)
    return out


def _intersection_report(mesh, engine) -> dict:
    """The ``check_intersections`` keyword of ``stitch``: the report of ``mesh_self_intersections`` on ``mesh``
    (imported here: intersect.py imports this module)."""
    from .intersect import mesh_self_intersections
    return mesh_self_intersections(mesh, engine=engine).report


def _refine_result(out: dict, refine, engine) -> dict:
    """The ``refine`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of refine_mesh keywords.  A
    new vertex is appended, in ascending vertex order, to every point list (SYNC_KEYS, ``boundary_points_*``) that holds
    both its parents by value; parents that are new vertices themselves count once they have joined."""
    if refine is False or refine is None:
        return out
    kw = dict(refine) if isinstance(refine, dict) else {}
    kw.setdefault("engine", engine)
    old = out["mesh"]
    new, parents, report = refine_mesh(old, **kw)
    nv0 = _p3(_mesh_parts(old)[0]).shape[0]
    v = _p3(_mesh_parts(new)[0])
    out = dict(out)
    out["mesh"] = new
    out["refine_report"] = report
    for key in SYNC_KEYS + tuple(sorted(k for k in out if k.startswith("boundary_points_"))):
        pts = out.get(key)
        if pts is None or len(pts) == 0 or parents.shape[0] == 0:
            continue
        member = np.zeros(v.shape[0], dtype=bool)
        member[:nv0] = _match(_p3(pts), v[:nv0]) >= 0
        for k in range(parents.shape[0]):                                # ascending: a parent's own membership is known
            member[nv0 + k] = member[parents[k, 0]] and member[parents[k, 1]]
        out[key] = np.concatenate([_p3(pts), v[nv0:][member[nv0:]]])
    return out


def _iv_lumen_vertices(out: dict) -> np.ndarray:
    """The vertices of ``out["mesh"]`` that are points of the intravascular lumen (``anomalous_points``), ascending."""
    iv = out.get("anomalous_points")
    at = _match(_p3(_mesh_parts(out["mesh"])[0]), _p3(iv)) if iv is not None and len(iv) else np.zeros(0, dtype=np.int64)
    return np.unique(at[at >= 0])


def _collapse_result(out: dict, collapse, engine) -> dict:
    """The ``collapse`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of collapse_edges keywords.
    Without ``pinned`` the vertices of the intravascular lumen are pinned.  A removed vertex leaves every point list
    (SYNC_KEYS, ``boundary_points_*``) that holds it by value, the counterpart of how ``_refine_result`` adds the new ones."""
    if collapse is False or collapse is None:
        return out
    kw = dict(collapse) if isinstance(collapse, dict) else {}
    kw.setdefault("engine", engine)
    if "pinned" not in kw:
        kw["pinned"] = _iv_lumen_vertices(out)
    old = out["mesh"]
    new, origin, _, report = collapse_edges(old, **kw)
    v = _p3(_mesh_parts(old)[0])
    gone = np.ones(v.shape[0], dtype=bool)
    gone[origin] = False
    out = dict(out)
    out["mesh"] = new
    out["collapse_report"] = report
    if gone.any():
        removed = np.ascontiguousarray(v[gone])
        for key in SYNC_KEYS + tuple(sorted(k for k in out if k.startswith("boundary_points_"))):
            pts = out.get(key)
            if pts is None or len(pts) == 0:
                continue
            out[key] = _p3(pts)[_match(removed, _p3(pts)) < 0]
    return out


def _flip_result(out: dict, flip, engine) -> dict:
    """The ``flip`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of flip_edges keywords.
    Without ``pinned`` the vertices that are points of the intravascular lumen (``anomalous_points``) are pinned."""
    if flip is False or flip is None:
        return out
    kw = dict(flip) if isinstance(flip, dict) else {}
    kw.setdefault("engine", engine)
    if "pinned" not in kw:
        kw["pinned"] = _iv_lumen_vertices(out)
    out = dict(out)
    out["mesh"], out["flip_report"] = flip_edges(out["mesh"], **kw)
    return out


def _relax_result(out: dict, relax, engine) -> dict:
    """The ``relax`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of relax_mesh keywords."""
    if relax is False or relax is None:
        return out
    kw = dict(relax) if isinstance(relax, dict) else {}
    kw.setdefault("engine", engine)
    old = out["mesh"]
    new, _, report = relax_mesh(old, kw.pop("reference", None), **kw)
    out = sync_results_to_mesh(out, old, new)
    out["relax_report"] = report
    return out


def _smooth_result(out: dict, smooth, engine) -> dict:
    """The ``smooth`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of smooth_mesh keywords."""
    if smooth is False or smooth is None:
        return out
    kw = dict(smooth) if isinstance(smooth, dict) else {}
    kw.setdefault("engine", engine)
    old = out["mesh"]
    new, report = smooth_mesh(old, **kw)
    out = sync_results_to_mesh(out, old, new)
    out["smooth_report"] = report
    return out


MM_ERR_TOO_LARGE = -3                    # include/mm_hausdorff.h


# ---- rim conditioning (multimodars/ccta/stitching.py:484-1064) -----------------------------------------------------------

RIM_REPORT_KEYS = ("n_vertices", "n_faces", "n_prox", "n_dist", "n_moved_prox", "n_moved_dist", "n_moved_ostium", "clamped",
                   "n_layer_vertices", "n_inserted_prox", "n_inserted_dist", "n_fanned_faces", "n_centroid_fans",
                   "ring_over_target", "ring_off_mesh", "n_launches", "bytes_uploaded", "bytes_downloaded",
                   "plane_shift_mm", "plane_angle_deg")


def _ring_call(rc: int, what: str):
    """MM_ERR_INVALID of a ring function is a ValueError (a NaN, a repeated ring vertex); everything else as check."""
    if rc == -2:
        raise ValueError(f"{what}: {N.last_error()}")
    if rc < 0:
        N.check(int(rc), what)
    return rc


def fit_ring_plane(points):
    """_plane_normal_svd (stitching.py:965-969): ``(centroid, normal)`` of the best-fit plane; the normal is the
    direction of least variance with its largest component positive (numpy leaves the sign to LAPACK)."""
    p = _p3(points)
    o, n = np.zeros(3), np.zeros(3)
    _ring_call(N.lib().mm_ring_fit_plane(N._ptr(p), p.shape[0], N._ptr(o), N._ptr(n)), "fit_ring_plane")
    return o, n


def project_to_best_fit_plane(points, origin=None, normal=None) -> np.ndarray:
    """_project_to_best_fit_plane (stitching.py:648-665); with ``origin`` and ``normal`` _project_onto_plane (:775-782)."""
    p = _p3(points)
    out = np.zeros_like(p)
    o = None if origin is None else _p3(origin)
    n = None if normal is None else _p3(normal)
    _ring_call(N.lib().mm_ring_project_to_plane(N._ptr(p), p.shape[0], N._ptr(o), N._ptr(n), N._ptr(out)),
               "project_to_best_fit_plane")
    return out


def smooth_ring_preserving_size(points, iterations: int = 5, alpha: float = 0.5) -> np.ndarray:
    """_smooth_ring_preserving_size (stitching.py:706-739): Laplacian smoothing of a closed ring, scaled back to the
    calibre it had."""
    p = _p3(points)
    out = np.zeros_like(p)
    _ring_call(N.lib().mm_ring_smooth_preserving_size(N._ptr(p), p.shape[0], int(iterations), float(alpha), N._ptr(out)),
               "smooth_ring_preserving_size")
    return out


def redistribute_ring_evenly(points, n_out: Optional[int] = None) -> np.ndarray:
    """_redistribute_ring_evenly (stitching.py:742-772): ``n_out`` points (default: as many as given) at equal arc
    lengths of the closed polyline; index 0 stays where it is."""
    p = _p3(points)
    if n_out is not None and int(n_out) < 0:
        raise ValueError("n_out must not be negative")
    k = -1 if n_out is None else int(n_out)
    out = np.zeros((max(p.shape[0], k, 1), 3), dtype=np.float64)
    m = _ring_call(N.lib().mm_ring_redistribute(N._ptr(p), p.shape[0], k, N._ptr(out)), "redistribute_ring_evenly")
    return out[:m].copy()


def shift_plane_clear_of(origin, normal, points, outward, overshoot: float):
    """_shift_plane_clear_of (stitching.py:785-813): ``(origin, normal, moved)`` of the plane turned along ``outward``
    and moved until every point lies ``overshoot`` behind it."""
    o, n, p, w = _p3(origin), _p3(normal), _p3(points), _p3(outward)
    so, sn, moved = np.zeros(3), np.zeros(3), C.c_double(0.0)
    _ring_call(N.lib().mm_plane_shift_clear_of(N._ptr(o), N._ptr(n), N._ptr(p), p.shape[0], N._ptr(w), float(overshoot),
                                               N._ptr(so), N._ptr(sn), C.byref(moved)), "shift_plane_clear_of")
    return so, sn, float(moved.value)


def clamp_to_plane(points, plane_origin, plane_normal, overshoot: float = 0.0) -> np.ndarray:
    """_clamp_to_plane (stitching.py:978-1011)."""
    p, o, n = _p3(points), _p3(plane_origin), _p3(plane_normal)
    out = np.zeros_like(p)
    _ring_call(N.lib().mm_ring_clamp_to_plane(N._ptr(p), p.shape[0], N._ptr(o), N._ptr(n), float(overshoot), N._ptr(out)),
               "clamp_to_plane")
    return out


def densify_plan(ring, target_n: int):
    """The insert counts of _densify_boundary (stitching.py:862-892): ``(counts, status)``, status 1 with a plan, 0 where
    nothing is to insert, 2 where the ring has more than ``target_n`` points."""
    p = _p3(ring)
    counts = np.zeros(max(p.shape[0], 1), dtype=np.int64)
    st = _ring_call(N.lib().mm_ring_densify_plan(N._ptr(p), p.shape[0], int(target_n), N._ptr(counts)), "densify_plan")
    return counts[:p.shape[0]].copy(), int(st)


def locate_points(vertices, points, engine: Optional[N.Engine] = None) -> np.ndarray:
    """The reference's ``{tuple(v): i}`` lookup on the device (csrc/mm_rim_kernels.hip): for every point the index of the
    last vertex equal to it by value (-0.0 equals 0.0; a NaN equals nothing), -1 without one."""
    v, p = _p3(vertices), _p3(points)
    idx = np.full(max(p.shape[0], 1), -1, dtype=np.int64)
    N.check(N.lib().mm_mesh_locate_points(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(p), p.shape[0], N._ptr(idx)),
            "locate_points")
    return idx[:p.shape[0]].copy()


def write_ring_to_mesh(mesh, old_pts, new_pts, engine: Optional[N.Engine] = None):
    """_write_ring_to_mesh (stitching.py:816-834): ``(mesh, moved)``, the mesh with the vertices at ``old_pts`` moved to
    ``new_pts`` and the sorted indices that moved.  The vertices are found on the device (locate_points)."""
    v, f = _mesh_parts(mesh)
    v = _p3(v).copy()
    new = _p3(new_pts)
    idx = locate_points(v, old_pts, engine)
    order = np.argsort(idx, kind="stable")
    for a, b in zip(order[:-1], order[1:]):
        if idx[a] >= 0 and idx[a] == idx[b] and new[a].tobytes() != new[b].tobytes():
            raise ValueError("two ring points with different targets sit on one mesh vertex")
    hit = idx >= 0
    v[idx[hit]] = new[hit]
    return _with_mesh(mesh, v, np.asarray(f)), sorted(set(idx[hit].tolist()))


def enforce_layer_gap_from_plane(mesh, seed_indices, plane_origin, plane_normal, layer_step_mm: float = 0.1,
                                 n_rings: int = 2, engine: Optional[N.Engine] = None, return_info: bool = False):
    """_enforce_layer_gap_from_plane (stitching.py:1014-1064) on the device: the vertices ``k <= n_rings`` edges away
    from the seeds move ``k * layer_step_mm`` along their radial direction in the plane.  ``return_info`` adds
    ``(layer, info)``: the layer of every vertex (-1 beyond ``n_rings``) and ``launches`` / ``rings_run`` /
    ``n_layer_vertices``."""
    v, f = _mesh_parts(mesh)
    v = _p3(v)
    f = _checked_faces(f, v.shape[0])
    seeds = np.ascontiguousarray(sorted(set(int(i) for i in seed_indices)), dtype=np.int64)
    if seeds.size and (seeds[0] < 0 or seeds[-1] >= v.shape[0]):
        raise ValueError("seed index out of range")
    out = np.zeros((max(v.shape[0], 1), 3), dtype=np.float64)
    layer = np.full(max(v.shape[0], 1), -1, dtype=np.int32)
    info = np.zeros(3, dtype=np.int64)
    o, n = _p3(plane_origin), _p3(plane_normal)
    N.check(N.lib().mm_mesh_layer_push(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(seeds),
                                       seeds.shape[0], N._ptr(o), N._ptr(n), float(layer_step_mm), int(n_rings),
                                       N._ptr(out), N._ptr(layer), N._ptr(info)), "enforce_layer_gap_from_plane")
    new = _with_mesh(mesh, out[:v.shape[0]].copy(), np.asarray(f))
    if not return_info:
        return new
    return new, layer[:v.shape[0]].copy(), {"launches": int(info[0]), "rings_run": int(info[1]),
                                            "n_layer_vertices": int(info[2])}


def split_rim_edges(vertices, faces, ring_idx, counts, engine: Optional[N.Engine] = None, vert_cap: Optional[int] = None,
                    face_cap: Optional[int] = None):
    """The mesh side of _densify_boundary (stitching.py:894-962) on the device for a ring of vertex indices and the
    points each ring edge receives: ``(vertices, faces, dense_ring_idx, info)``.  include/mm_ccta.h states the order
    of everything appended.  ``vert_cap`` / ``face_cap`` are the first sizes tried; too small, the call is repeated once
    with the sizes the first one reports."""
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    ring = np.ascontiguousarray(np.asarray(ring_idx, dtype=np.int64).ravel())
    cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int64).ravel())
    if ring.shape[0] != cnt.shape[0]:
        raise ValueError("one count per ring edge")
    if ring.shape[0] < 3:
        raise ValueError("a ring needs at least 3 vertices")
    if cnt.size and cnt.min() < 0:
        raise ValueError("insert counts must not be negative")
    total = int(cnt.sum())
    vert_cap = v.shape[0] + total + 8 if vert_cap is None else int(vert_cap)
    face_cap = f.shape[0] + total + 8 if face_cap is None else int(face_cap)
    dense = np.zeros(ring.shape[0] + total, dtype=np.int64)
    info = np.zeros(6, dtype=np.int64)
    for attempt in (0, 1):
        out_v = np.zeros((max(vert_cap, 1), 3), dtype=np.float64)
        out_f = np.zeros((max(face_cap, 1), 3), dtype=np.int64)
        rc = N.lib().mm_mesh_split_rim_edges(_engine(engine).handle, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0],
                                             N._ptr(ring), ring.shape[0], N._ptr(cnt), vert_cap, face_cap, N._ptr(out_v),
                                             N._ptr(out_f), N._ptr(dense), N._ptr(info))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and (info[0] > vert_cap or info[1] > face_cap):
            vert_cap, face_cap = int(info[0]), int(info[1])
            continue
        _ring_call(rc, "split_rim_edges")
        break
    rep = {"n_vertices": int(info[0]), "n_faces": int(info[1]), "n_inserted": int(info[2]), "n_fanned_faces": int(info[3]),
           "n_centroid_fans": int(info[4]), "launches": int(info[5]), "attempts": attempt + 1}
    return out_v[:info[0]].copy(), out_f[:info[1]].copy(), dense, rep


def densify_boundary(mesh, ring, target_n: int, engine: Optional[N.Engine] = None):
    """_densify_boundary (stitching.py:837-962): ``(mesh, dense_ring, info)``; the ring gets ``target_n`` points, the
    extra ones on its longest edges first, and every face that owns a subdivided edge becomes a fan.  A ring above the
    target or off the mesh comes back as it is (``info["over_target"]`` / ``info["off_mesh"]``)."""
    r = _p3(ring)
    v, f = _mesh_parts(mesh)
    v = _p3(v)
    info = {"n_inserted": 0, "n_fanned_faces": 0, "n_centroid_fans": 0, "over_target": 0, "off_mesh": 0, "launches": 0}
    counts, status = densify_plan(r, target_n)
    info["over_target"] = int(status == 2)
    if status != 1:
        return mesh, r.copy(), info
    idx = locate_points(v, r, engine)
    info["launches"] = 1
    if (idx < 0).any():
        info["off_mesh"] = 1
        return mesh, r.copy(), info
    nv, nf, dense, rep = split_rim_edges(v, f, idx, counts, engine)
    for k in ("n_inserted", "n_fanned_faces", "n_centroid_fans"):
        info[k] = rep[k]
    info["launches"] += rep["launches"]
    return _with_mesh(mesh, nv, nf), nv[dense], info


def _condition(v, f, prox_ring, dist_ring, iv_frame, prox_centroid, prox_outward, aorta, params: dict, engine,
               vert_cap=None, face_cap=None):
    """mm_condition_rims with the capacity retry: ``(vertices, faces, prox, dist, report)``."""
    v = _p3(v)
    f = _checked_faces(f, v.shape[0])
    pr, dr, iv, ao = _p3(prox_ring), _p3(dist_ring), _p3(iv_frame), _p3(aorta if aorta is not None else ())
    pc = _p3(prox_centroid)
    po = None if prox_outward is None else _p3(prox_outward)
    target = int(params["target_n"])
    ring_cap = max(pr.shape[0], dr.shape[0], target, 1)
    P = N.MMRimParams(int(bool(params["proximal_is_ostium"])), target, int(params.get("smooth_iterations", 5)),
                      int(params.get("n_rings", 2)), 0, 0, ring_cap, float(params.get("smooth_alpha", 0.5)),
                      float(params["angle_threshold_deg"]), float(params["clamp_overshoot"]),
                      float(params.get("layer_step_mm", 0.1)))
    vert_cap = v.shape[0] + 2 * target + 64 if vert_cap is None else int(vert_cap)
    face_cap = f.shape[0] + 4 * target + 64 if face_cap is None else int(face_cap)
    rep = N.MMRimReport()
    h = _engine(engine).handle
    attempts = 0
    while True:
        attempts += 1
        P.vert_cap, P.face_cap = vert_cap, face_cap
        out_v = np.zeros((max(vert_cap, 1), 3), dtype=np.float64)
        out_f = np.zeros((max(face_cap, 1), 3), dtype=np.int64)
        out_p, out_d = np.zeros((ring_cap, 3), dtype=np.float64), np.zeros((ring_cap, 3), dtype=np.float64)
        rc = N.lib().mm_condition_rims(h, N._ptr(v), v.shape[0], N._ptr(f), f.shape[0], N._ptr(pr), pr.shape[0], N._ptr(dr),
                                       dr.shape[0], N._ptr(iv), iv.shape[0], N._ptr(pc), N._ptr(po), N._ptr(ao), ao.shape[0],
                                       C.byref(P), N._ptr(out_v), N._ptr(out_f), N._ptr(out_p), N._ptr(out_d), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempts < 4 and (rep.n_vertices > vert_cap or rep.n_faces > face_cap):
            vert_cap, face_cap = max(vert_cap, int(rep.n_vertices)), max(face_cap, int(rep.n_faces))
            continue
        _ring_call(rc, "condition_boundary_rings")
        break
    report = {}
    for k in RIM_REPORT_KEYS:
        x = getattr(rep, k)
        report[k] = x if isinstance(x, (int, float)) else [int(y) for y in x]
    report["attempts"] = attempts
    return (out_v[:rep.n_vertices].copy(), out_f[:rep.n_faces].copy(), out_p[:rep.n_prox].copy(), out_d[:rep.n_dist].copy(),
            report)


def condition_boundary_rings(mesh, results: dict, iv_geometry: G.FlatGeometry, n_points_iv_cont: int = 100,
                             proximal_is_ostium: bool = True, clamp_overshoot: float = 0.5,
                             boundary_point_ratio: float = 1.0, ostium_angle_threshold_deg: float = 45.0,
                             engine: Optional[N.Engine] = None) -> dict:
    """_prepare_prox_dist_boundary_pts (stitching.py:484-556), the first stage of the reference's
    stitch_ccta_to_intravascular, as a step of its own: both rims of the cut mesh are flattened onto their best-fit
    plane, smoothed without shrinking, respaced evenly and written back into the mesh; an ostial proximal ring has its
    plane slid clear of the first IV frame, is clamped against the IV plane where the two meet at
    ``ostium_angle_threshold_deg`` or more (``clamp_overshoot`` mm of clearance; the two vertex layers behind a clamped
    ring move out by 0.1 and 0.2 mm); and both rims are densified to ``max(3, round(boundary_point_ratio * n))`` points,
    ``n`` the points of the first downsampled IV contour, every CCTA face on a subdivided rim edge being replaced by a
    fan, so that the strip of the stitch is point for point and the mesh has no T-junction.

    The rings are those the stitch would use (``boundary_points_<n>`` of ``results``, else the mesh's open edges) and are
    assigned to the ends as it assigns them.  Returns a new dict: ``mesh`` replaced (the same kind of container),
    ``boundary_points_1`` / ``boundary_points_2`` the conditioned proximal and distal ring, ``boundary_points`` both,
    ``rim_report`` what was done (RIM_REPORT_KEYS, ``n_leftover_rings``, ``target_n``).  It goes into
    ``stitch_ccta_to_intravascular(iv_geometry, out["mesh"], out, ...)`` unchanged.  The mesh makes one trip to the
    device and back (csrc/mm_rim.cpp, csrc/mm_rim_kernels.hip); include/mm_ccta.h states every rule."""
    frames = _downsample_geometry(iv_geometry, int(n_points_iv_cont))
    if not frames:
        raise ValueError("Need at least two contours to build a mesh.")
    prox_c, dist_c = iv_geometry.centroids[0].copy(), iv_geometry.centroids[-1].copy()
    rings = _result_rings(results, mesh, engine)
    if len(rings) < 2:
        raise ValueError(f"Stitching needs a proximal and a distal boundary ring, but {len(rings)} were found. Re-run "
                         f"the removal with target_boundaries=2 so both rims are kept as separate rings.")
    i, j, leftover = assign_rings_to_ends(rings, prox_c, dist_c)
    target_n = max(3, round(boundary_point_ratio * frames[0].shape[0]))
    params = {"proximal_is_ostium": proximal_is_ostium, "target_n": target_n,
              "angle_threshold_deg": ostium_angle_threshold_deg, "clamp_overshoot": clamp_overshoot}
    v, f = _mesh_parts(mesh)
    aorta = results.get("aorta_points", None)
    new_v, new_f, prox, dist, report = _condition(v, f, rings[i], rings[j], frames[0], prox_c, prox_c - dist_c, aorta,
                                                  params, engine)
    report["n_leftover_rings"] = len(leftover)
    report["target_n"] = target_n
    out = {k: val for k, val in results.items() if not k.startswith(BOUNDARY_RING_PREFIX)}
    out["mesh"] = _with_mesh(mesh, new_v, new_f)
    out[f"{BOUNDARY_RING_PREFIX}1"] = prox
    out[f"{BOUNDARY_RING_PREFIX}2"] = dist
    out["boundary_points"] = np.concatenate([prox, dist])
    out["rim_report"] = report
    return out


def stitch_conditioned(results: dict, geometry: G.FlatGeometry, region_remove=("anomalous_points", "proximal_points"),
                       prox_start_mode: str = "highest_z", dist_start_mode: str = "nearest_iv", fill_holes: bool = False,
                       engine: Optional[N.Engine] = None, smooth=False, refine=False, relax=False, flip=False,
                       collapse=False, repair=False, **conditioning) -> dict:
    """``stitch`` with the reference's rim conditioning in front of the seam: remove ``region_remove``
    (``target_boundaries=2``), ``condition_boundary_rings(**conditioning)``, ``stitch_ccta_to_intravascular`` and, with
    ``fill_holes``, ``manual_hole_fill``.  Together the middle two are the reference's stitching.py:355-481.  The result
    carries ``rim_report`` beside ``stitch_report`` (and ``fill_report``).  ``refine`` and ``smooth`` as in ``stitch``:
    the refinement runs behind the hole fill and adds ``refine_report``, the smoothing runs last and adds
    ``smooth_report``; ``relax`` as in ``stitch`` too, between the two, adding ``relax_report``, ``flip`` in front
    of it, adding ``flip_report``, and ``collapse`` in front of the flips, adding ``collapse_report``; ``repair`` as in
    ``stitch``, between the assembly and the hole filling, adding ``"repair"``."""
    keys = [region_remove] if isinstance(region_remove, str) else list(region_remove)
    updated = remove_labeled_points_from_mesh(results, keys, target_boundaries=2, engine=engine)
    cond = condition_boundary_rings(updated["mesh"], updated, geometry, engine=engine, **conditioning)
    n_iv = int(conditioning.get("n_points_iv_cont", 100))
    out = stitch_ccta_to_intravascular(geometry, cond["mesh"], cond, n_points_iv_cont=n_iv, prox_start_mode=prox_start_mode,
                                       dist_start_mode=dist_start_mode, engine=engine)
    out = _repair_result(out, repair, engine)
    if fill_holes:
        v, f = _mesh_parts(out["mesh"])
        new_v, new_f, report = _fill(v, f, True, engine)
        out["mesh"] = _with_mesh(out["mesh"], new_v, new_f)
        out["fill_report"] = report
    out = _collapse_result(_refine_result(out, refine, engine), collapse, engine)
    return _smooth_result(_relax_result(_flip_result(out, flip, engine), relax, engine), smooth, engine)


# ---- mesh closing (multimodars/ccta/fixing_functions.py:13-49, ccta/__init__.py:432-499, ccta_py.rs:743-814) -----------

FILL_REPORT_KEYS = ("n_vertices", "n_faces", "n_loops_filled", "n_fan_faces", "n_open_edges_before", "n_short_loops",
                    "n_irregular_components", "n_irregular_edges", "n_open_edges", "n_nonmanifold_edges",
                    "n_flipped_faces", "winding_rounds", "inverted", "volume")


def hole_loops(half_edges, vertices):
    """The host walk of the hole filling on a list of open half-edges ``(a, b)`` (no device): ``(loops, centroids,
    info)``, the regular loops of at least 3 vertices as int64 index arrays in increasing order of their smallest
    vertex, each starting there and following the half-edges, their centroids ``(L, 3)``, and ``info`` with
    ``n_irregular_components``, ``n_irregular_edges`` and ``n_short_loops``.  include/mm_ccta.h states the rules."""
    e = np.ascontiguousarray(np.asarray(half_edges, dtype=np.int64).reshape(-1, 2))
    v = _p3(vertices)
    ne = e.shape[0]
    loop_len, loop_idx = np.zeros(ne + 1, dtype=np.int64), np.zeros(ne + 1, dtype=np.int64)
    centroids = np.zeros(ne + 3, dtype=np.float64)
    counts = np.zeros(5, dtype=np.int64)
    rc = N.lib().mm_hole_loops(N._ptr(e), ne, N._ptr(v), v.shape[0], N._ptr(loop_len), N._ptr(loop_idx),
                               N._ptr(centroids), N._ptr(counts))
    if rc == -2 and e.size and (e.min() < 0 or e.max() >= v.shape[0]):
        raise ValueError("half-edge end out of range")
    N.check(rc, "hole_loops")
    info = {"n_irregular_components": int(counts[2]), "n_irregular_edges": int(counts[3]), "n_short_loops": int(counts[4])}
    return _rings(loop_len, loop_idx, int(counts[0])), centroids[:3 * counts[0]].reshape(-1, 3).copy(), info


def fill_holes(vertices, faces, fix_normals: bool = True, engine: Optional[N.Engine] = None):
    """manual_hole_fill (fixing_functions.py:13-49) on arrays: every hole whose rim is a regular loop is closed by a fan
    about the loop's centroid.  Returns ``(vertices, faces, report)``: the input vertices followed by one centroid per
    loop, the input faces (after the winding stage of fix_mesh_winding when ``fix_normals``) followed by the fans, and
    ``report`` with FILL_REPORT_KEYS and ``"watertight"`` (no open and no non-manifold edge, as assemble_mesh defines
    it).  An edge owned by one face is open and is followed the way its owner traverses it; a rim vertex is regular
    when one open half-edge leaves and one enters it; a loop runs through regular vertices only, starts at its
    smallest vertex, and loops come in increasing order of that vertex; loop ``k`` gets vertex ``nv + k`` and the
    faces ``(b, a, nv + k)`` for its half-edges ``a -> b``.  Rims with a pinch vertex, with faces that disagree in
    direction (possible only with ``fix_normals=False``) or beside a non-manifold edge are left open and counted
    (``n_irregular_components``, ``n_irregular_edges``).  With ``fix_normals`` the result is reversed as a whole when
    its signed volume is negative (the reference's closing ``fix_normals()``).

    Where this differs from the reference: that takes its loops from trimesh's outline entities, re-orders each by a
    walk over the mesh adjacency restricted to the loop's points (which can cut across a chord) with an angle sort
    as fall-back, and finds vertices by coordinate (the last duplicate wins).  This one follows the rim itself and
    works on indices; on a loop the reference walks without a chord the fan is the same set of triangles.  Everything
    proportional to the mesh runs on the device (csrc/mm_weld_kernels.hip, csrc/mm_close_kernels.hip); the walk over
    the rim is host code.  The outputs are allocated for a small rim first and, where that is too small, once more
    with the exact sizes the first call reports."""
    return _fill(vertices, faces, fix_normals, engine)


def _fill(vertices, faces, fix_normals, engine):
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    nv, nf = v.shape[0], f.shape[0]
    h = _engine(engine).handle
    rep = N.MMFillReport()
    vert_cap, face_cap = nv + 16, nf + 1024
    for attempt in (0, 1):
        out_v = np.zeros((vert_cap, 3), dtype=np.float64)
        out_f = np.zeros((face_cap, 3), dtype=np.int64)
        rc = N.lib().mm_fill_holes(h, N._ptr(v), nv, N._ptr(f), nf, int(bool(fix_normals)), vert_cap, face_cap,
                                   N._ptr(out_v), N._ptr(out_f), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and (rep.n_vertices > vert_cap or rep.n_faces > face_cap):
            vert_cap, face_cap = int(rep.n_vertices), int(rep.n_faces)
            continue
        N.check(rc, "fill_holes")
        break
    report = {k: getattr(rep, k) for k in FILL_REPORT_KEYS}
    report["watertight"] = report["n_open_edges"] == 0 and report["n_nonmanifold_edges"] == 0
    return out_v[:rep.n_vertices].copy(), out_f[:rep.n_faces].copy(), report


def manual_hole_fill(mesh, fix_normals: bool = True, engine: Optional[N.Engine] = None):
    """fixing_functions.py:13-49: ``mesh`` (a ``(vertices, faces)`` tuple or an object with ``.vertices`` / ``.faces``)
    with every regular hole closed by a fan about its centroid, as a new mesh of the kind given; the input is not
    modified.  ``fill_holes`` states the rules and the differences from the reference, and returns the report too."""
    v, f = _mesh_parts(mesh)
    new_v, new_f, _ = _fill(v, f, fix_normals, engine)
    return _with_mesh(mesh, new_v, new_f)


def smooth_mesh_labels_info(labels, adjacency_map=None, iterations: int = 1, faces=None,
                            engine: Optional[N.Engine] = None):
    """smooth_mesh_labels with what the run did: ``(labels, info)``, ``info`` holding ``iterations_run``,
    ``n_flips``, ``n_flips_last`` and ``launches`` (the kernels the call launched)."""
    lab = np.ascontiguousarray(np.asarray(labels, dtype=np.uint8).reshape(-1))
    if (adjacency_map is None) == (faces is None):
        raise ValueError("give exactly one of adjacency_map and faces")
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative")
    nv = lab.shape[0]
    out = np.zeros_like(lab)
    info = np.zeros(4, dtype=np.int64)
    h = _engine(engine).handle
    if faces is not None:
        f = _checked_faces(faces, nv)
        rc = N.lib().mm_smooth_labels_faces(h, N._ptr(lab), nv, N._ptr(f), f.shape[0], int(iterations), N._ptr(out),
                                            N._ptr(info))
    else:
        rows = [np.fromiter(adjacency_map.get(i, ()), dtype=np.int64) for i in range(nv)]
        off = np.zeros(nv + 1, dtype=np.int64)
        if nv:
            off[1:] = np.cumsum([r.shape[0] for r in rows])
        nb = np.ascontiguousarray(np.concatenate(rows)) if nv and off[-1] else np.zeros(0, dtype=np.int64)
        if nb.size and (nb.min() < 0 or nb.max() >= nv):
            raise ValueError(f"neighbour index out of range [0, {nv})")
        rc = N.lib().mm_smooth_labels_csr(h, N._ptr(lab), nv, N._ptr(off), N._ptr(nb), int(iterations), N._ptr(out),
                                          N._ptr(info))
    N.check(rc, "smooth_mesh_labels")
    return out, {"iterations_run": int(info[0]), "n_flips": int(info[1]), "n_flips_last": int(info[2]),
                 "launches": int(info[3])}


def smooth_mesh_labels(labels, adjacency_map=None, iterations: int = 1, faces=None,
                       engine: Optional[N.Engine] = None) -> np.ndarray:
    """ccta_py.rs:743-814: ``labels`` (one ``uint8`` per vertex) smoothed for ``iterations`` synchronous rounds: a
    vertex with at least one neighbour, all of whose neighbours carry the same label different from its own, takes that
    label; every round reads the labels of the round before only.  Only unanimous votes flip, so the reference's
    hash-order tie never matters and the result is exact.  A round that flips nothing ends the run.  Give exactly one
    of ``faces`` (recommended: the neighbours are those of build_adjacency_map, found on the device without building a
    dict of sets) and ``adjacency_map`` (the dict of build_adjacency_map, the reference's positional signature; read
    row by row as given, it need not be symmetric; a vertex without an entry has no neighbour).  The labels stay on
    the device across the rounds (csrc/mm_close_kernels.hip).  Returns a new ``uint8`` array."""
    return smooth_mesh_labels_info(labels, adjacency_map, iterations, faces, engine)[0]


WALL_AORTA_KEYS = ("aorta_points", "rca_removed_points", "lca_removed_points")


def _wall_sub_mesh(results: dict, keys, engine):
    """keep_labeled_points_from_mesh for the wall mesh: an empty region or one that matches no vertex is an error
    there (keep_labeled_points_from_mesh hands back its input, which would take the whole mesh as the sub-mesh)."""
    sub = keep_labeled_points_from_mesh(results, list(keys), engine=engine)
    if sub is results:
        raise ValueError(f"create_wall_mesh: {' + '.join(keys)} is empty or matches no vertex of the mesh")
    return sub


def create_wall_mesh(geometry, cl_aorta: Centerline, cl_rca: Centerline, cl_lca: Centerline, results: dict,
                     aortic_scaling: Optional[float] = None, coronary_scaling: float = 1.0,
                     engine: Optional[N.Engine] = None) -> dict:
    """ccta/__init__.py:432-499: a wall mesh from the labelled lumen mesh.  The aortic scaling is
    ``find_aortic_wall_scaling(geometry, cl_aorta, results)`` where ``geometry`` is given, else ``aortic_scaling``
    (both ``None``: ``ValueError("Either provide frames or aortic scaling")``, before anything else).  The aortic
    sub-mesh (``aorta_points``, ``rca_removed_points``, ``lca_removed_points`` kept) has its ostia filled
    (``manual_hole_fill``) and every vertex of the filled mesh, the new centres included, morphed about ``cl_aorta``;
    the ``rca_points`` and ``lca_points`` sub-meshes are kept and morphed about their centerlines by
    ``coronary_scaling``; the three are concatenated in that order without welding.  Returns a new dict (the input is
    not modified) with ``"mesh"`` replaced and ``"wall_report"`` = ``{"aortic_scaling", "coronary_scaling",
    "fill_report"}``.  A region that is empty or matches no vertex raises ``ValueError`` naming its key, where
    keep_labeled_points_from_mesh would hand the whole mesh back as the sub-mesh (what the reference does in that case
    was not checked)."""
    if geometry is None and aortic_scaling is None:
        raise ValueError("Either provide frames or aortic scaling")
    scaling = float(find_aortic_wall_scaling(geometry, cl_aorta, results)) if geometry is not None else float(aortic_scaling)
    mesh = results["mesh"]
    aorta = _wall_sub_mesh(results, WALL_AORTA_KEYS, engine)
    av, af = _mesh_parts(aorta["mesh"])
    fv, ff, fill_report = _fill(av, af, True, engine)
    parts = [(centerline_morph_batch([(cl_aorta, fv, scaling)], engine)[0][0], ff)]
    for key, cl in (("rca_points", cl_rca), ("lca_points", cl_lca)):
        sub = _wall_sub_mesh(results, (key,), engine)
        moved = scale_region_centerline_morphing(sub["mesh"], sub[key], cl, float(coronary_scaling), engine)
        pv, pf = _mesh_parts(moved)
        parts.append((_p3(pv), _faces3(pf)))
    off = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.int64)
    out = dict(results)
    out["mesh"] = _with_mesh(mesh, np.ascontiguousarray(np.concatenate([p[0] for p in parts])),
                             np.ascontiguousarray(np.concatenate([p[1] + o for p, o in zip(parts, off[:-1])])))
    out["wall_report"] = {"aortic_scaling": scaling, "coronary_scaling": float(coronary_scaling),
                          "fill_report": fill_report}
    return out


# ---- mesh smoothing (multimodars/ccta/fixing_functions.py:52-92; trimesh.smoothing.filter_taubin / filter_laplacian) ---

SMOOTH_REPORT_KEYS = ("n_vertices", "n_faces", "n_edges", "n_isolated", "n_pinned", "max_degree", "steps_run", "launches",
                      "volume_before", "volume_after", "max_displacement_sq")


def _n_vertices(faces: np.ndarray, n_vertices) -> int:
    nv = (int(faces.max()) + 1 if faces.size else 0) if n_vertices is None else int(n_vertices)
    if nv < 0:
        raise ValueError("n_vertices must not be negative")
    return nv


def mesh_adjacency_csr(faces, n_vertices=None, engine: Optional[N.Engine] = None):
    """The vertex adjacency the smoothing runs over, built on the device (csrc/mm_smooth_kernels.hip): ``(off, nb,
    info)``.  Row ``v`` = ``nb[off[v]:off[v + 1]]`` = the distinct vertices other than ``v`` that share a corner pair
    with it in some face, ascending (a face ``(a, a, b)`` gives ``a-b`` only; repeated faces add nothing).
    ``n_vertices`` defaults to the largest index + 1.  ``info``: ``entries``, ``max_degree``, ``n_isolated``,
    ``launches``.  Unlike ``build_adjacency_map`` there are no self entries and the order is fixed."""
    f = _faces3(faces)
    nv = _n_vertices(f, n_vertices)
    f = _checked_faces(f, nv)
    h = _engine(engine).handle
    off = np.zeros(nv + 1, dtype=np.int64)
    info = np.zeros(4, dtype=np.int64)
    cap = 3 * f.shape[0] + 64                                             # a closed surface needs 3 nf
    for attempt in (0, 1):
        nb = np.zeros(max(cap, 1), dtype=np.int64)
        rc = N.lib().mm_mesh_adjacency_csr(h, N._ptr(f), f.shape[0], nv, cap, N._ptr(off), N._ptr(nb), N._ptr(info))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and info[0] > cap:
            cap = int(info[0])
            continue
        N.check(rc, "mesh_adjacency_csr")
        break
    return off, nb[:info[0]].copy(), {"entries": int(info[0]), "max_degree": int(info[1]), "n_isolated": int(info[2]),
                                      "launches": int(info[3])}


def vertex_rings_info(faces, seeds, max_ring: int, n_vertices=None, engine: Optional[N.Engine] = None):
    """``vertex_rings`` with what the run did: ``(ring, info)``, ``info`` holding ``reached``, ``rounds``, ``launches``."""
    f = _faces3(faces)
    nv = _n_vertices(f, n_vertices)
    f = _checked_faces(f, nv)
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
    if s.size and (s.min() < 0 or s.max() >= nv):
        raise ValueError(f"seed index out of range [0, {nv})")
    if int(max_ring) < 0:
        raise ValueError("max_ring must not be negative")
    ring = np.full(nv, -1, dtype=np.int32)
    info = np.zeros(3, dtype=np.int64)
    N.check(N.lib().mm_mesh_vertex_rings(_engine(engine).handle, N._ptr(f), f.shape[0], nv, N._ptr(s), s.shape[0],
                                         int(max_ring), N._ptr(ring), N._ptr(info)), "vertex_rings")
    return ring, {"reached": int(info[0]), "rounds": int(info[1]), "launches": int(info[2])}


def vertex_rings(faces, seeds, max_ring: int, n_vertices=None, engine: Optional[N.Engine] = None) -> np.ndarray:
    """``ring[v]`` (int32) = the fewest mesh edges from vertex ``v`` to any of the seed vertices ``seeds`` (indices), 0 at
    a seed; -1 for a vertex farther than ``max_ring`` edges or not connected to a seed.  A level-synchronous search on
    the device over the adjacency of ``mesh_adjacency_csr``."""
    return vertex_rings_info(faces, seeds, max_ring, n_vertices, engine)[0]


def _seed_indices(seeds, vertices: np.ndarray) -> np.ndarray:
    """Seeds given as vertex indices (an integer array) or as xyz points (matched to the vertices by value as
    sync_results_to_mesh matches; a point that is no vertex is dropped)."""
    a = np.asarray(seeds)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.bool_):
        return np.flatnonzero(a) if a.dtype == np.bool_ else a.astype(np.int64).reshape(-1)
    idx = _match(vertices, a)
    return np.unique(idx[idx >= 0])


def _pin_mask(pinned, band, v: np.ndarray, f: np.ndarray, engine):
    """The uint8 mask of ``smooth_mesh`` / ``relax_mesh`` from their ``pinned`` and ``band`` keywords (None: no mask)."""
    nv = v.shape[0]
    mask = None
    if pinned is not None:
        p = np.asarray(pinned)
        if p.dtype == np.bool_:
            if p.reshape(-1).shape[0] != nv:
                raise ValueError("a pinned mask has one entry per vertex")
            mask = p.reshape(-1).copy()
        else:
            p = p.astype(np.int64).reshape(-1)
            if p.size and (p.min() < 0 or p.max() >= nv):
                raise ValueError(f"pinned index out of range [0, {nv})")
            mask = np.zeros(nv, dtype=bool)
            mask[p] = True
    if band is not None:
        seeds, k = band
        ring = vertex_rings(f, _seed_indices(seeds, v), int(k), nv, engine)
        mask = (ring < 0) if mask is None else (mask | (ring < 0))
    return None if mask is None else np.ascontiguousarray(mask.astype(np.uint8))


def smooth_mesh(mesh, factors=None, *, lamb: float = 0.5, nu: float = 0.5, iterations: int = 10, pinned=None, band=None,
                engine: Optional[N.Engine] = None):
    """Laplacian / Taubin smoothing of ``mesh`` (a ``(vertices, faces)`` tuple or an object with ``.vertices`` /
    ``.faces``) on the device: ``(mesh, report)``, the mesh of the kind given with new vertices and the same faces; the
    input is not modified.  One step with factor ``f`` moves every vertex with a neighbour by ``f`` times the difference
    between the equal-weight mean of its neighbours and itself; ``factors`` lists the steps' factors, and where it is
    None the Taubin schedule ``lamb, -nu, lamb, ...`` of ``iterations`` steps is used
    (trimesh.smoothing.filter_taubin, as fixing_functions.py:52-92 ends the post-processing).  The neighbours are summed
    in ascending index order in unfused f64 (include/mm_ccta.h, "mesh smoothing"), so the result has one bit pattern
    whatever the scheduling; against trimesh, whose row order is a graph library's insertion order, it agrees up to the
    order of that sum.  A vertex without a face stays where it is (trimesh pulls it towards the origin).

    ``pinned``: a bool mask over the vertices or an array of indices that do not move (they still pull their
    neighbours).  ``band=(seeds, k)`` frees only the vertices within ``k`` edges of the seed vertices (indices, or xyz
    points matched to the vertices by value) and pins everything else; with both, a vertex pinned by either stays.
    ``report``: SMOOTH_REPORT_KEYS (``launches``: the kernels of the call; ``volume_before`` / ``volume_after``: the
    signed volume assemble_mesh reports, before and after) and ``volume_ratio``."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    if factors is None:
        if int(iterations) < 0:
            raise ValueError("iterations must not be negative")
        factors = [float(lamb) if i % 2 == 0 else -float(nu) for i in range(int(iterations))]
    fac = np.ascontiguousarray(np.asarray(factors, dtype=np.float64).reshape(-1))
    m8 = _pin_mask(pinned, band, v, f, engine)
    out = np.zeros_like(v)
    rep = N.MMSmoothReport()
    N.check(N.lib().mm_mesh_smooth(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), f.shape[0], N._ptr(fac),
                                   fac.shape[0], N._ptr(m8), N._ptr(out), C.byref(rep)), "smooth_mesh")
    report = {k: getattr(rep, k) for k in SMOOTH_REPORT_KEYS}
    report["volume_ratio"] = report["volume_after"] / report["volume_before"] if report["volume_before"] != 0.0 \
        else float("nan")
    return _with_vertices(mesh, out), report


def filter_taubin(mesh, lamb: float = 0.5, nu: float = 0.5, iterations: int = 10, **kw):
    """trimesh.smoothing.filter_taubin with equal weights: ``iterations`` steps alternating ``lamb`` and ``-nu``
    (step 0 takes ``lamb``).  Returns the new mesh only; keywords as ``smooth_mesh`` (``pinned``, ``band``,
    ``engine``)."""
    return smooth_mesh(mesh, None, lamb=lamb, nu=nu, iterations=iterations, **kw)[0]


def filter_laplacian(mesh, lamb: float = 0.5, iterations: int = 10, **kw):
    """trimesh.smoothing.filter_laplacian with equal weights and without volume constraint: ``iterations`` steps of
    factor ``lamb``.  Returns the new mesh only; keywords as ``smooth_mesh``."""
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative")
    return smooth_mesh(mesh, [float(lamb)] * int(iterations), **kw)[0]


# ---- mesh relaxation (multimodars/ccta/fixing_functions.py:192-219: smoothing and reprojection of the isotropic remesh) --

RELAX_REPORT_KEYS = ("n_vertices", "n_faces", "n_ref_faces", "n_free", "n_pinned", "n_border", "n_isolated",
                     "iterations_run", "n_reverted", "n_flipped_faces", "items_run", "items_skipped", "items_skipped_step0",
                     "n_launches", "bytes_uploaded", "bytes_downloaded", "initial_distance_sq", "max_displacement_sq", "volume_before",
                     "volume_after")


def relax_mesh(mesh, reference=None, *, iterations: int = 5, lamb: float = 0.5, pinned=None, band=None,
               engine: Optional[N.Engine] = None):
    """Tangential relaxation of ``mesh`` reprojected onto ``reference`` (a mesh of either kind; None: ``mesh`` as it
    comes in), on the device: ``(mesh, ref_face, report)``.  Every free vertex is first put on the closest point of the
    reference; each of the ``iterations`` Jacobi steps then moves it by ``lamb`` times the part of (mean of its
    neighbours - itself) that is tangent to the reference face it lies on, and puts it back on the closest point of
    the reference; a step that would turn a face's normal is taken back at that face's vertices (include/mm_ccta.h,
    "mesh relaxation").  The faces do not change and the result has one bit pattern.  Free are the vertices with a
    neighbour that are neither pinned nor on a border or non-manifold edge; all others keep their bits.

    ``pinned`` and ``band`` as in ``smooth_mesh``.  ``ref_face[v]``: the reference face vertex ``v`` lies on, -1 where it
    is not free.  ``report``: RELAX_REPORT_KEYS and ``volume_ratio``; ``initial_distance_sq`` is the largest squared
    distance a free vertex had from the reference, ``n_reverted`` the moves taken back, ``n_flipped_faces`` the faces
    that ended turned against their input normal."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative")
    if not np.isfinite(float(lamb)):
        raise ValueError("lamb must be finite")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinate")
    rv = rf = None
    if reference is not None:
        rvert, rfaces = _mesh_parts(reference)
        rv = _p3(rvert)
        rf = _checked_faces(rfaces, rv.shape[0])
        if not np.isfinite(rv).all():
            raise ValueError("non-finite reference coordinate")
    m8 = _pin_mask(pinned, band, v, f, engine)
    out = np.zeros_like(v)
    ref_face = np.full(nv, -1, dtype=np.int64)
    rep = N.MMRelaxReport()
    N.check(N.lib().mm_mesh_relax(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), f.shape[0], N._ptr(rv),
                                  0 if rv is None else rv.shape[0], N._ptr(rf), 0 if rf is None else rf.shape[0],
                                  N._ptr(m8), int(iterations), float(lamb), N._ptr(out), N._ptr(ref_face), C.byref(rep)),
            "relax_mesh")
    report = {k: getattr(rep, k) for k in RELAX_REPORT_KEYS}
    report["volume_ratio"] = report["volume_after"] / report["volume_before"] if report["volume_before"] != 0.0 \
        else float("nan")
    return _with_vertices(mesh, out), ref_face, report


def project_to_mesh(mesh, reference, **kw):
    """``mesh`` with every free vertex on the closest point of ``reference``: ``relax_mesh(..., iterations=0)``."""
    return relax_mesh(mesh, reference, iterations=0, **kw)


# ---- mesh refinement (multimodars/ccta/fixing_functions.py:114-239: the edge split of the isotropic remesh) -----------

REFINE_REPORT_KEYS = ("n_vertices", "n_faces", "n_edges_before", "n_edges_after", "passes_run", "converged",
                      "stopped_by_cap", "n_open_edges_before", "n_open_edges_after", "n_nonmanifold_edges_before",
                      "n_nonmanifold_edges_after", "n_launches", "bytes_uploaded", "bytes_downloaded", "longest_sq_before",
                      "longest_sq_after", "volume_before", "volume_after")


def _edge_lengths_sq(v: np.ndarray, f: np.ndarray, engine):
    nv, nf = v.shape[0], f.shape[0]
    h = _engine(engine).handle
    info = np.zeros(4, dtype=np.int64)
    cap = 3 * nf // 2 + 64                                                # a closed surface has 3 nf / 2 edges
    for attempt in (0, 1):
        edges = np.zeros((max(cap, 1), 2), dtype=np.int64)
        len_sq = np.zeros(max(cap, 1), dtype=np.float64)
        rc = N.lib().mm_mesh_edge_lengths(h, N._ptr(v), nv, N._ptr(f), nf, cap, N._ptr(edges), N._ptr(len_sq), N._ptr(info))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and info[0] > cap:
            cap = int(info[0])
            continue
        N.check(rc, "mesh_edge_lengths")
        break
    return edges[:info[0]].copy(), len_sq[:info[0]].copy(), info


def mesh_edge_lengths(mesh, engine: Optional[N.Engine] = None):
    """``(edges, lengths)`` of ``mesh`` (a ``(vertices, faces)`` tuple or an object with ``.vertices`` / ``.faces``):
    the distinct undirected edges ``(lo, hi)`` between different vertices, in the order in which a walk over the faces
    (corners 0, 1, 2 for the edges (c0, c1), (c1, c2), (c2, c0)) first meets them, and their lengths, the ``sqrt`` of
    the squares the device computes as ``refine_mesh`` marks with them (csrc/mm_refine_kernels.hip)."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    edges, len_sq, _ = _edge_lengths_sq(v, f, engine)
    return edges, np.sqrt(len_sq)


def edge_length_target(mesh, q: float = 25.0, engine: Optional[N.Engine] = None) -> float:
    """The reference's automatic ``target_edge_length_mm`` (fixing_functions.py:161-162): the ``q``-th percentile of
    the unique edge lengths, 25 keeping the fine intravascular resolution."""
    lengths = mesh_edge_lengths(mesh, engine)[1]
    if lengths.size == 0:
        raise ValueError("a mesh without an edge has no edge length target")
    return float(np.percentile(lengths, q))


def refine_mesh(mesh, target_edge_length_mm: Optional[float] = None, *, ratio: float = 4.0 / 3.0, passes: int = 10,
                max_vertices: Optional[int] = None, engine: Optional[N.Engine] = None):
    """Split every edge of ``mesh`` longer than ``ratio * target_edge_length_mm`` at its midpoint, pass after pass,
    on the device: ``(mesh, parents, report)``, the mesh of the kind given, the input not modified.  This is the edge
    split of the isotropic remesh with which the reference's post-processing (fixing_functions.py:114-239, MeshLab)
    brings the coarse CCTA triangles down to the intravascular resolution; its collapse is ``collapse_edges``, its flip
    ``flip_edges``, its tangential relaxation and reprojection ``relax_mesh``, the four together ``isotropic_remesh``;
    its repair step is ``repair_mesh``.  No existing vertex moves or changes its index: new
    vertices follow the old ones, ``parents[k]`` = the ends ``(lo, hi)`` of the edge whose midpoint vertex
    ``nv + k`` is, and every face is replaced in place by 1 to 4 children of its winding (include/mm_ccta.h, "mesh
    refinement", states the rule; it has one bit pattern whatever the scheduling).  A closed manifold mesh stays closed
    and manifold, and its volume changes by rounding only.

    ``target_edge_length_mm=None`` takes ``edge_length_target(mesh)``, the 25th percentile of the edge lengths as the
    reference does; ``ratio`` = 4/3 is the split threshold of Botsch and Kobbelt and of MeshLab's filter.  At most
    ``passes`` passes run (the reference's ``remesh_iterations``); they end on their own once no edge is too long
    (``converged``).  A pass that would bring the vertices above ``max_vertices`` is not run (``stopped_by_cap``).
    ``report``: REFINE_REPORT_KEYS, ``splits_per_pass`` (16 entries), ``faces_by_template`` (faces by their number of
    split edges, 0 .. 3, over all passes), ``target_edge_length_mm``, ``threshold_mm`` and ``watertight`` (no open and no
    non-manifold edge afterwards).  The outputs are allocated for a fourfold mesh first and, where that is too small,
    once more with the sizes the first call reports."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    nf = f.shape[0]
    if int(passes) < 0:
        raise ValueError("passes must not be negative")
    if max_vertices is not None and int(max_vertices) < 0:
        raise ValueError("max_vertices must not be negative")
    if target_edge_length_mm is None:
        lengths = np.sqrt(_edge_lengths_sq(v, f, engine)[1])
        if lengths.size == 0:
            raise ValueError("a mesh without an edge has no edge length target")
        target_edge_length_mm = float(np.percentile(lengths, 25.0))
    target, ratio = float(target_edge_length_mm), float(ratio)
    if not (np.isfinite(target) and target > 0.0 and np.isfinite(ratio) and ratio > 0.0):
        raise ValueError("target_edge_length_mm and ratio must be finite and greater than 0")
    h = _engine(engine).handle
    rep = N.MMRefineReport()
    cap_v = 2 ** 31 - 1 if max_vertices is None else int(max_vertices)
    vert_cap, face_cap = 4 * nv + 64, 4 * nf + 64
    for attempt in (0, 1):
        out_v = np.zeros((vert_cap, 3), dtype=np.float64)
        out_f = np.zeros((face_cap, 3), dtype=np.int64)
        out_p = np.zeros((max(vert_cap - nv, 1), 2), dtype=np.int64)
        rc = N.lib().mm_mesh_refine(h, N._ptr(v), nv, N._ptr(f), nf, target, ratio, int(passes), cap_v, vert_cap, face_cap,
                                    N._ptr(out_v), N._ptr(out_f), N._ptr(out_p), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and (rep.n_vertices > vert_cap or rep.n_faces > face_cap):
            vert_cap, face_cap = int(rep.n_vertices), int(rep.n_faces)
            continue
        N.check(rc, "refine_mesh")
        break
    report = {k: getattr(rep, k) for k in REFINE_REPORT_KEYS}
    report["splits_per_pass"] = list(rep.splits_per_pass)
    report["faces_by_template"] = list(rep.faces_by_template)
    report["target_edge_length_mm"] = target
    report["threshold_mm"] = ratio * target
    report["watertight"] = report["n_open_edges_after"] == 0 and report["n_nonmanifold_edges_after"] == 0
    new = _with_mesh(mesh, out_v[:rep.n_vertices].copy(), out_f[:rep.n_faces].copy())
    return new, out_p[:rep.n_vertices - nv].copy(), report


# ---- mesh edge flips (multimodars/ccta/fixing_functions.py:207-219: the swap of the isotropic remesh) -----------------

FLIP_REPORT_KEYS = ("n_vertices", "n_faces", "n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges",
                    "n_masked_edges", "passes_run", "converged", "n_flips", "blocked_existing", "blocked_normal",
                    "blocked_crease", "blocked_quality", "deviation_before", "deviation_after", "n_launches",
                    "bytes_uploaded", "bytes_downloaded", "volume_before", "volume_after")


def mesh_valence(mesh, *, engine: Optional[N.Engine] = None):
    """``(degree, border, info)`` of ``mesh``: per vertex the number of distinct edges to other vertices and whether it
    ends an edge that does not have exactly two owning corners, as ``flip_edges`` counts them (include/mm_ccta.h, "mesh
    edge flips").  ``info``: ``n_edges``, ``n_open_edges``, ``n_nonmanifold_edges``, ``n_inconsistent_edges``,
    ``deviation`` (the sum over the vertices of (degree - target)^2, the target 4 on the border and 6 elsewhere) and
    ``n_launches``."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    deg = np.zeros(nv, dtype=np.int32)
    border = np.zeros(nv, dtype=np.uint8)
    info = np.zeros(6, dtype=np.int64)
    N.check(N.lib().mm_mesh_valence(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), f.shape[0], N._ptr(deg), N._ptr(border),
                                    N._ptr(info)), "mesh_valence")
    names = ("n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "deviation", "n_launches")
    return deg, border.astype(bool), dict(zip(names, info.tolist()))


def flip_edges(mesh, *, crease_deg: float = 30.0, quality_keep: float = 0.5, passes: int = 50, pinned=None, band=None,
               engine: Optional[N.Engine] = None):
    """Flip the edges of ``mesh`` whose flip brings the valences of their four vertices closer to 6 (4 on a border),
    pass after pass, on the device: ``(mesh, report)``, the mesh of the kind given with the same vertices and new faces,
    the input not modified.  This is the swap of the isotropic remesh of the reference's post-processing
    (fixing_functions.py:207-219); it runs behind ``refine_mesh``, whose midpoints have valence 4, and
    ``collapse_edges``, and in front of ``relax_mesh``; ``isotropic_remesh`` runs the four in turn.  A flip is made only where the new edge does not exist yet, no normal turns, the two faces meet at
    less than ``crease_deg`` (30 degrees, MeshLab's default crease angle) and the worse of the two new triangles keeps
    at least ``quality_keep``^2 of the quality of the worse old one.  In a pass the flips share no vertex, chosen by a
    priority and no order of visits, so the result has one bit pattern (include/mm_ccta.h, "mesh edge flips"); every
    pass lowers ``deviation`` and at most ``passes`` run.  No vertex moves; the other faces keep their place.

    ``pinned`` and ``band`` as in ``smooth_mesh``: an edge with a pinned end does not flip.  ``report``:
    FLIP_REPORT_KEYS, ``flips_per_pass`` and ``candidates_per_pass`` (16 entries each), ``crease_deg``,
    ``quality_keep`` and ``volume_ratio``."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    if int(passes) < 0:
        raise ValueError("passes must not be negative")
    crease_deg, quality_keep = float(crease_deg), float(quality_keep)
    if not 0.0 <= crease_deg <= 90.0:
        raise ValueError("crease_deg must lie in [0, 90]")
    if not 0.0 <= quality_keep <= 1.0:
        raise ValueError("quality_keep must lie in [0, 1]")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinate")
    m8 = _pin_mask(pinned, band, v, f, engine)
    out = np.zeros_like(f)
    rep = N.MMFlipReport()
    crease_cos = min(1.0, max(0.0, math.cos(math.radians(crease_deg))))
    N.check(N.lib().mm_mesh_flip_edges(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), f.shape[0], N._ptr(m8), crease_cos,
                                       quality_keep, int(passes), N._ptr(out), C.byref(rep)), "flip_edges")
    report = {k: getattr(rep, k) for k in FLIP_REPORT_KEYS}
    report["flips_per_pass"] = list(rep.flips_per_pass)
    report["candidates_per_pass"] = list(rep.candidates_per_pass)
    report["crease_deg"], report["quality_keep"] = crease_deg, quality_keep
    report["volume_ratio"] = report["volume_after"] / report["volume_before"] if report["volume_before"] != 0.0 \
        else float("nan")
    return _with_mesh(mesh, v.copy(), out), report


# ---- mesh edge collapse (multimodars/ccta/fixing_functions.py:207-219: the collapse of the isotropic remesh) ----------

COLLAPSE_REPORT_KEYS = ("n_vertices", "n_faces", "n_vertices_out", "n_faces_out", "n_edges", "n_open_edges",
                        "n_nonmanifold_edges", "n_inconsistent_edges", "n_short_before", "n_short_after", "passes_run",
                        "converged", "n_collapses", "blocked_fixed", "blocked_link", "blocked_valence", "blocked_long",
                        "blocked_normal", "blocked_quality", "n_launches", "bytes_uploaded", "bytes_downloaded",
                        "volume_before", "volume_after")


def _target_length(v: np.ndarray, f: np.ndarray, target_edge_length_mm, engine) -> float:
    """``target_edge_length_mm``, or where it is None the 25th percentile of the edge lengths as ``refine_mesh`` takes it."""
    if target_edge_length_mm is None:
        lengths = np.sqrt(_edge_lengths_sq(v, f, engine)[1])
        if lengths.size == 0:
            raise ValueError("a mesh without an edge has no edge length target")
        target_edge_length_mm = float(np.percentile(lengths, 25.0))
    target = float(target_edge_length_mm)
    if not (np.isfinite(target) and target > 0.0):
        raise ValueError("target_edge_length_mm must be finite and greater than 0")
    return target


def collapse_edges(mesh, target_edge_length_mm: Optional[float] = None, *, min_ratio: float = 4.0 / 5.0,
                   max_ratio: float = 4.0 / 3.0, crease_deg: float = 30.0, quality_keep: float = 0.5, passes: int = 50,
                   pinned=None, band=None, engine: Optional[N.Engine] = None):
    """Remove the edges of ``mesh`` shorter than ``min_ratio * target_edge_length_mm`` by half-edge collapses, pass after
    pass, on the device: ``(mesh, origin, target, report)``, the mesh of the kind given, the input not modified.  This is
    the collapse of the isotropic remesh of the reference's post-processing (fixing_functions.py:207-219); it runs
    behind ``refine_mesh`` and in front of ``flip_edges``.  A collapse removes one end of the edge and the two faces at
    it and puts the other end in its place: no surviving vertex moves, and survivors keep their order
    (``origin[new] = old``; ``target[old]`` = the new index of the vertex an old one ended in).  The half-edge form is
    this project's choice and not MeshLab's, which collapses onto the midpoint: here no measured vertex moves.
    ``quality_keep`` is ours too.  MeshLab's ``checksurfdist`` bound is not part of this project; its repair is ``repair_mesh``
    (``surface_distance`` between input and result measures what the bound would limit).

    A collapse is made only where the removed end is neither pinned nor on a border, the two ends share exactly the two
    opposite corners as neighbours (the link condition), no valence falls below 3, no new edge is longer than
    ``max_ratio * target_edge_length_mm`` (so the split does not undo it), no normal turns by more than ``crease_deg``
    and the worst new triangle keeps ``quality_keep``^2 of the worst old one.  In a pass the neighbourhoods of the
    removed vertices are disjoint, chosen by a priority (the shortest edge first) and no order of visits, so the result
    has one bit pattern (include/mm_ccta.h, "mesh edge collapse").  ``target_edge_length_mm=None`` takes
    ``edge_length_target(mesh)`` as ``refine_mesh`` does; 4/5 and 4/3 are the thresholds of Botsch and Kobbelt and of
    MeshLab's filter.

    ``pinned`` and ``band`` as in ``flip_edges``: a pinned vertex is never removed; it may be the end that stays.
    ``report``: COLLAPSE_REPORT_KEYS, ``collapses_per_pass`` and ``candidates_per_pass`` (16 entries each),
    ``target_edge_length_mm``, ``min_ratio``, ``max_ratio``, ``crease_deg``, ``quality_keep`` and ``volume_ratio``."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    nv = v.shape[0]
    f = _checked_faces(faces, nv)
    nf = f.shape[0]
    if int(passes) < 0:
        raise ValueError("passes must not be negative")
    crease_deg, quality_keep, min_ratio, max_ratio = float(crease_deg), float(quality_keep), float(min_ratio), float(max_ratio)
    if not 0.0 <= crease_deg <= 90.0:
        raise ValueError("crease_deg must lie in [0, 90]")
    if not 0.0 <= quality_keep <= 1.0:
        raise ValueError("quality_keep must lie in [0, 1]")
    if not 0.0 < min_ratio <= 1.0:
        raise ValueError("min_ratio must lie in (0, 1]")
    if not (np.isfinite(max_ratio) and max_ratio >= 1.0):
        raise ValueError("max_ratio must be finite and at least 1")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinate")
    target = _target_length(v, f, target_edge_length_mm, engine)
    m8 = _pin_mask(pinned, band, v, f, engine)
    out_v = np.zeros((max(nv, 1), 3), dtype=np.float64)
    out_f = np.zeros((max(nf, 1), 3), dtype=np.int64)
    origin = np.zeros(max(nv, 1), dtype=np.int64)
    tgt = np.zeros(max(nv, 1), dtype=np.int64)
    rep = N.MMCollapseReport()
    crease_cos = min(1.0, max(0.0, math.cos(math.radians(crease_deg))))
    N.check(N.lib().mm_mesh_collapse_edges(_engine(engine).handle, N._ptr(v), nv, N._ptr(f), nf, N._ptr(m8), target, min_ratio,
                                           max_ratio, crease_cos, quality_keep, int(passes), N._ptr(out_v), N._ptr(out_f),
                                           N._ptr(origin), N._ptr(tgt), C.byref(rep)), "collapse_edges")
    report = {k: getattr(rep, k) for k in COLLAPSE_REPORT_KEYS}
    report["collapses_per_pass"] = list(rep.collapses_per_pass)
    report["candidates_per_pass"] = list(rep.candidates_per_pass)
    report["target_edge_length_mm"], report["min_ratio"], report["max_ratio"] = target, min_ratio, max_ratio
    report["crease_deg"], report["quality_keep"] = crease_deg, quality_keep
    report["volume_ratio"] = report["volume_after"] / report["volume_before"] if report["volume_before"] != 0.0 \
        else float("nan")
    kv, kf = int(rep.n_vertices_out), int(rep.n_faces_out)
    return _with_mesh(mesh, out_v[:kv].copy(), out_f[:kf].copy()), origin[:kv].copy(), tgt[:nv].copy(), report


def _edge_share(v: np.ndarray, f: np.ndarray, lo: float, hi: float, engine) -> float:
    """The share of the edges of (v, f) whose length lies in [lo, hi]; NaN without an edge."""
    if v.shape[0] == 0 or f.shape[0] == 0:
        return float("nan")
    lengths = np.sqrt(_edge_lengths_sq(v, f, engine)[1])
    return float(((lengths >= lo) & (lengths <= hi)).mean()) if lengths.size else float("nan")


def isotropic_remesh(mesh, target_edge_length_mm: Optional[float] = None, *, iterations: int = 10, reference=None,
                     pinned=None, band=None, crease_deg: float = 30.0, quality_keep: float = 0.5, relax=None,
                     engine: Optional[N.Engine] = None):
    """The isotropic explicit remesh of the reference's post-processing (fixing_functions.py:207-219: ``splitflag``,
    ``collapseflag``, ``swapflag``, ``smoothflag``, ``reprojectflag``) as a composition of this project's four calls:
    ``(mesh, report)``.  Each of the ``iterations`` runs one pass of ``refine_mesh``, ``collapse_edges``,
    ``flip_edges`` and ``relax_mesh`` onto ``reference`` (None: ``mesh`` as it comes in), all at
    ``target_edge_length_mm`` (None: ``edge_length_target(mesh)``), every call from its own upload: a composite that
    stays on the device is not offered.  ``pinned`` and ``band`` as in ``flip_edges``, evaluated once on the input; the
    pin mask is carried through the index changes: the midpoints of the split are free, the survivors of the collapse
    are followed through its ``origin``.  ``relax``: a dict of further ``relax_mesh`` keywords (``iterations``,
    ``lamb``).  The collapse is a half-edge collapse and ``quality_keep`` guards flips and collapses: both are this
    project's choices, not MeshLab's; its midpoint collapse and its ``checksurfdist`` bound are not here, its repair is
    ``repair_mesh``, and ``fix_and_remesh_stitched_mesh`` runs repair, hole fill and this remesh in turn.

    ``report``: ``iterations`` (one dict a round with the reports ``refine``, ``collapse``, ``flip``, ``relax``),
    ``target_edge_length_mm``, ``share_in_range_before`` / ``_after`` (the share of the edges with a length within
    [4/5, 4/3] of the target), ``n_vertices_before`` / ``_after`` and ``n_faces_before`` / ``_after``."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinate")
    target = _target_length(v, f, target_edge_length_mm, engine)
    lo, hi = 4.0 / 5.0 * target, 4.0 / 3.0 * target
    mask = _pin_mask(pinned, band, v, f, engine)
    mask = None if mask is None else mask.astype(bool)
    ref = (v.copy(), f.copy()) if reference is None else reference
    relax_kw = dict(relax) if relax else {}
    report = {"iterations": [], "target_edge_length_mm": target, "share_in_range_before": _edge_share(v, f, lo, hi, engine),
              "n_vertices_before": v.shape[0], "n_faces_before": f.shape[0]}
    cur = (v, f)
    for _ in range(int(iterations)):
        cur, parents, r_split = refine_mesh(cur, target, passes=1, engine=engine)
        if mask is not None:
            mask = np.concatenate([mask, np.zeros(parents.shape[0], dtype=bool)])
        cur, origin, _, r_col = collapse_edges(cur, target, crease_deg=crease_deg, quality_keep=quality_keep, pinned=mask,
                                               engine=engine)
        if mask is not None:
            mask = mask[origin]
        cur, r_flip = flip_edges(cur, crease_deg=crease_deg, quality_keep=quality_keep, pinned=mask, engine=engine)
        cur, _, r_relax = relax_mesh(cur, ref, pinned=mask, engine=engine, **relax_kw)
        report["iterations"].append({"refine": r_split, "collapse": r_col, "flip": r_flip, "relax": r_relax})
    report.update(share_in_range_after=_edge_share(cur[0], cur[1], lo, hi, engine), n_vertices_after=cur[0].shape[0],
                  n_faces_after=cur[1].shape[0])
    return _with_mesh(mesh, cur[0], cur[1]), report


# ---- mesh repair (multimodars/ccta/fixing_functions.py:114-239: MeshLab's five repair filters; the composite) ---------

REPAIR_REPORT_KEYS = ("n_vertices", "n_faces", "n_welded_vertices", "n_degenerate_faces", "n_null_faces",
                      "n_duplicate_faces", "n_nonmanifold_edges_before", "n_nonmanifold_edges_after", "n_faces_removed",
                      "n_nonmanifold_vertices", "n_new_vertices", "n_unreferenced_dropped", "n_open_edges_before",
                      "n_open_edges_after", "union_rounds", "n_launches", "bytes_uploaded", "bytes_downloaded")
MANIFOLD_REPORT_KEYS = ("n_vertices", "n_faces", "n_open_edges", "n_nonmanifold_edges", "n_nonmanifold_vertices",
                        "n_duplicate_vertices", "n_degenerate_faces", "n_null_faces", "n_duplicate_faces")
REPAIR_FLAGS = (("duplicate_vertices", 1), ("null_faces", 2), ("duplicate_faces", 4), ("nonmanifold_edges", 8),
                ("nonmanifold_vertices", 16), ("drop_unreferenced", 32))


def _repair_arrays(mesh):
    """The checked arrays of a mesh for the repair: ValueError before the engine is touched."""
    vertices, faces = _mesh_parts(mesh)
    v = _p3(vertices)
    f = _checked_faces(faces, v.shape[0])
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinate")
    return v, f


def _repair(v: np.ndarray, f: np.ndarray, flags: int, engine):
    """mm_mesh_repair on checked arrays: the outputs sized for a few new vertices first and, where they do not fit,
    once more with the exact size the first call reports (the protocol of ``fill_holes``)."""
    nv, nf = v.shape[0], f.shape[0]
    h = _engine(engine).handle
    rep = N.MMRepairReport()
    vert_cap = nv + 16
    out_f = np.zeros((max(nf, 1), 3), dtype=np.int64)
    tgt = np.zeros(max(nv, 1), dtype=np.int64)
    for attempt in (0, 1):
        out_v = np.zeros((vert_cap, 3), dtype=np.float64)
        origin = np.zeros(vert_cap, dtype=np.int64)
        rc = N.lib().mm_mesh_repair(h, N._ptr(v), nv, N._ptr(f), nf, int(flags), vert_cap, N._ptr(out_v), N._ptr(out_f),
                                    N._ptr(origin), N._ptr(tgt), C.byref(rep))
        if rc == MM_ERR_TOO_LARGE and attempt == 0 and rep.n_vertices > vert_cap:
            vert_cap = int(rep.n_vertices)
            continue
        N.check(rc, "repair_mesh")
        break
    kv, kf = int(rep.n_vertices), int(rep.n_faces)
    return out_v[:kv].copy(), out_f[:kf].copy(), origin[:kv].copy(), tgt[:nv].copy(), rep


def repair_mesh(mesh, *, duplicate_vertices: bool = True, null_faces: bool = True, duplicate_faces: bool = True,
                nonmanifold_edges: bool = True, nonmanifold_vertices: bool = True, drop_unreferenced: bool = False,
                engine: Optional[N.Engine] = None):
    """The repair that stands in front of the hole filling in the reference's ``fix_and_remesh_stitched_mesh``
    (fixing_functions.py:168-177, five MeshLab filters), on the device: ``(mesh, origin, target, report)``, the mesh of
    the kind given, the input not modified.  MeshLab is not available to this project; the rules are its own
    (include/mm_ccta.h, "mesh repair"), deterministic, and run in this order, each behind its switch:

    (a) ``duplicate_vertices``: vertices whose three coordinates compare equal (``+0.0 == -0.0``; nothing is rounded,
        unreferenced vertices take part) become the one with the smallest index;
    (b) a face with a repeated index always goes; ``null_faces``: so does one whose cross product is exactly zero;
    (c) ``duplicate_faces``: of the faces with one vertex set the first stays;
    (d) ``nonmanifold_edges``: on an edge with more than two owners the two largest faces (by squared area, then index)
        stay and every other owner is removed -- MeshLab's "remove faces", its area order made total;
    (e) ``nonmanifold_vertices``: a vertex whose faces do not hang together across edges with two owners is split, one
        new vertex with the same coordinates (MeshLab's displacement 0) per further fan;
    (f) ``drop_unreferenced`` (off, as MeshLab's five filters leave them): a vertex no face names is dropped.

    The order is not the reference's, which welds behind the split and so merges again what the split has made.  A
    weld that the split would only undo is not made: a vertex whose faces would form a fan of their own at the vertex
    it equals stays as it is, so a repaired mesh comes back from a second call bit for bit, with ``origin`` and
    ``target`` the identity and every count zero.  A switched-off stage still counts what it finds.  Survivors keep their order and their bits; new vertices follow
    them.  ``origin[new]`` = the input vertex whose bits the output vertex carries, ``target[old]`` = the output vertex
    of an input vertex (-1 where (f) dropped it).  After (d) no edge has more than two owners, after (e) every rim is a
    regular loop that ``fill_holes`` closes.  ``report``: REPAIR_REPORT_KEYS and ``watertight`` (no open and no
    non-manifold edge, as ``fill_holes`` defines it)."""
    flags = 0
    for (name, bit), on in zip(REPAIR_FLAGS, (duplicate_vertices, null_faces, duplicate_faces, nonmanifold_edges,
                                              nonmanifold_vertices, drop_unreferenced)):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False")
        flags |= bit if on else 0
    v, f = _repair_arrays(mesh)
    out_v, out_f, origin, tgt, rep = _repair(v, f, flags, engine)
    report = {k: getattr(rep, k) for k in REPAIR_REPORT_KEYS}
    report["watertight"] = report["n_open_edges_after"] == 0 and report["n_nonmanifold_edges_after"] == 0
    return _with_mesh(mesh, out_v, out_f), origin, tgt, report


def mesh_manifold_report(mesh, engine: Optional[N.Engine] = None) -> dict:
    """What ``repair_mesh`` would find in ``mesh``, as counts only (MANIFOLD_REPORT_KEYS and ``watertight``): the
    same kernels with every switch off, so nothing is changed and every stage counts the mesh as given -- a weld would
    change what the later stages see.  Faces with a repeated index are counted and left out of the edge counts."""
    v, f = _repair_arrays(mesh)
    rep = _repair(v, f, 0, engine)[4]
    report = {"n_vertices": v.shape[0], "n_faces": f.shape[0], "n_open_edges": rep.n_open_edges_before,
              "n_nonmanifold_edges": rep.n_nonmanifold_edges_before, "n_nonmanifold_vertices": rep.n_nonmanifold_vertices,
              "n_duplicate_vertices": rep.n_welded_vertices, "n_degenerate_faces": rep.n_degenerate_faces,
              "n_null_faces": rep.n_null_faces, "n_duplicate_faces": rep.n_duplicate_faces}
    report["watertight"] = report["n_open_edges"] == 0 and report["n_nonmanifold_edges"] == 0
    return report


def fix_and_remesh_stitched_mesh(mesh, *, target_edge_length_mm: Optional[float] = None, remesh_iterations: int = 10,
                                 verbose: bool = False, pinned=None, band=None, return_report: bool = False,
                                 engine: Optional[N.Engine] = None):
    """fixing_functions.py:114-239 as a composition of this project's public calls: ``repair_mesh``, ``fill_holes``,
    ``isotropic_remesh`` and, where the result is not watertight, ``repair_mesh(duplicate_vertices=False)`` and
    ``fill_holes`` once more, as the reference's third block does.  Returns the mesh of the kind given, with
    ``return_report`` ``(mesh, report)``.  ``target_edge_length_mm=None``: ``edge_length_target`` of the input, taken
    before anything changes (the reference's P25).  ``pinned`` and ``band`` as in ``flip_edges``, evaluated on the
    input; the mask follows the vertices through every step's ``origin``: a vertex the split makes inherits its
    parent's pin, the centroids of the hole fans are free.  ``verbose`` prints the reference's line (vertices, faces,
    watertight) per stage.

    Where this differs from the reference: the holes are closed by fans about the rim's centroid instead of MeshLab's
    ear cut, and there is no ``maxholesize``; the collapse of the remesh is a half-edge collapse; there is no
    ``checksurfdist`` bound; and the repair welds first and splits last (``repair_mesh``), where the reference's order
    merges again what its split has made.

    ``report``: ``target_edge_length_mm``, ``repair``, ``fill``, ``remesh``, ``manifold`` (``mesh_manifold_report`` behind
    the remesh), ``post_repair`` and ``post_fill`` (None where the remesh left the mesh watertight), ``watertight``."""
    v, f = _repair_arrays(mesh)
    if int(remesh_iterations) < 0:
        raise ValueError("remesh_iterations must not be negative")
    target = _target_length(v, f, target_edge_length_mm, engine)
    mask = _pin_mask(pinned, band, v, f, engine)
    mask = None if mask is None else mask.astype(bool)

    def log(label, m, watertight):
        if verbose:
            print(f"[{label:35s}] verts={len(m[0]):>7,}  faces={len(m[1]):>7,}  watertight={watertight}")

    if verbose:
        log("input", (v, f), mesh_manifold_report((v, f), engine)["watertight"])
        print(f"  target edge length = {target:.4f} mm")
    cur, origin, _, r_repair = repair_mesh((v, f), engine=engine)
    if mask is not None:
        mask = mask[origin]
    fv, ff, r_fill = _fill(cur[0], cur[1], True, engine)
    if mask is not None:
        mask = np.concatenate([mask, np.zeros(fv.shape[0] - mask.shape[0], dtype=bool)])
    log("after hole fill", (fv, ff), r_fill["watertight"])
    cur, r_remesh = isotropic_remesh((fv, ff), target, iterations=int(remesh_iterations), pinned=mask, engine=engine)
    r_manifold = mesh_manifold_report(cur, engine)
    log("after remesh", cur, r_manifold["watertight"])
    report = {"target_edge_length_mm": target, "repair": r_repair, "fill": r_fill, "remesh": r_remesh,
              "manifold": r_manifold, "post_repair": None, "post_fill": None, "watertight": r_manifold["watertight"]}
    if not r_manifold["watertight"]:
        cur, _, _, report["post_repair"] = repair_mesh(cur, duplicate_vertices=False, engine=engine)
        fv, ff, report["post_fill"] = _fill(cur[0], cur[1], True, engine)
        cur = (fv, ff)
        report["watertight"] = report["post_fill"]["watertight"]
        log("after post-remesh fix", cur, report["watertight"])
    out = _with_mesh(mesh, cur[0], cur[1])
    return (out, report) if return_report else out


def _repair_result(out: dict, repair, engine) -> dict:
    """The ``repair`` keyword of ``stitch`` / ``stitch_conditioned``: False, True, or a dict of repair_mesh keywords.  The
    mesh is repaired between the assembly and the hole filling; its report goes under ``"repair"``.  No vertex moves
    and the new vertices repeat their parents' coordinates, so the point lists, which hold coordinates, stay."""
    if repair is False or repair is None:
        return out
    kw = dict(repair) if isinstance(repair, dict) else {}
    kw.setdefault("engine", engine)
    out = dict(out)
    out["mesh"], _, _, out["repair"] = repair_mesh(out["mesh"], **kw)
    return out


def postprocess_stitched_mesh(mesh, *, postprocessing: bool = False, lamb: float = 0.5, nu: float = 0.5,
                              iterations: int = 10, **kw):
    """fixing_functions.py:52-92 by the reference's name and flag.  ``postprocessing=False`` hands the mesh back as it
    is.  ``True`` runs the Taubin smoothing that ends the reference's post-processing (``filter_taubin``); the repair,
    the hole fill and the isotropic remesh in front of it are a call of their own, ``fix_and_remesh_stitched_mesh``
    (or ``isotropic_remesh`` alone), to be made in front of this function, so ``target_edge_length_mm`` or
    ``remesh_iterations`` raise NotImplementedError.  Other keywords go to ``smooth_mesh``."""
    for name in ("target_edge_length_mm", "remesh_iterations"):
        if name in kw:
            raise NotImplementedError(f"{name}: the isotropic remesh of the reference's post-processing is not part of "
                                      "this function, only its Taubin smoothing runs here; call mm.isotropic_remesh "
                                      "(or mm.fix_and_remesh_stitched_mesh) in front of it")
    if not postprocessing:
        return mesh
    return filter_taubin(mesh, lamb, nu, iterations, **kw)
